// The M355_* environment switches of libmi355yolo.so, declared once.  switches.hip is the only file of the library that reads
// the environment; it gives every name its default and its history.  tools/README.md has the table of all of them
// (tests/test_switches_host.py keeps the two in step).  A switch has exactly one of three lifetimes:
//   process          ProcSwitches, read at the first use in the process: launchers and *_ok predicates are on the hot path.
//   engine creation  PlanSwitches, read once by m355_engine_create and kept in the engine: the A/B tests and bench.py --serial
//                    set a variable, create an engine and unset it, many times in one process.
//   per call         the live_*() functions: a test or a tool changes them between two calls of one process.
#pragma once

namespace m355 {

struct ProcSwitches {
  // conv_igemm.hip, conv3x3_halo.hip, misc_kernels.hip, the engine's forward
  bool no_fast_epi, no_wide, no_m32, no_bias_lds, static_tiles, no_persist, stem_gather;
  int persist, halo_variant, smallm;
  // c2f_c32.hip, conv3x3_c32.hip, conv3x3_m32.hip, conv3x3_wide.hip (slots / stagger: -1 = unset, the launcher computes)
  bool c2f_noprio;
  const char* c2f_stamps;
  int c32_waste, c32_slots, m32_slots, wide_slots, wide_stagger;
  // conv3x3_s2c32.hip, conv3x3_s2c64.hip, proto_phase_wreg.hip
  int s2c32_dbg, s2c32_ring, s2c64_prio, protor_prio;
  const char *s2c32_stamps, *s2c64_stamps, *protor_stamps;
  // conv_stem_c2.hip, conv_stem_s2c32.hip.  M355_NO_STEMFUSE has two lifetimes: this one refuses the launch (stem_s2c32_ok) for
  // the whole process, PlanSwitches::no_stemfuse keeps the fusion pass of one engine from planning it.
  int stem2_nxb;
  bool no_stemfuse;
  // misc_kernels.hip, postprocess.hip
  int sppf_minblocks, mask_dbg, mask_tile;
  // the training step: conv_dgrad_s2c32.hip, conv_wgrad.hip, conv_wgrad3.hip, m355_train_conv (op_entries.hip)
  bool no_dgrad_s2c32, no_wgrad_stem, no_wgrad_s2c32, no_wgrad3, no_train_w1, no_train_c32;
  int wgrad_blocks, w2_blocks_x2, wgrad3_shrink, wgrad3_blocks, wgrad3_mintiles;
  long wgrad3_slabmb;
};
const ProcSwitches& proc_switches();

struct PlanSwitches {
  // graph builders
  bool no_c2f32, no_pair, no_protofuse, no_protofuse3, no_upfuse;
  bool no_headdiag, headdiag_l0;   // (no_headdiag is read by the fusion pass of annotate_ops)
  int lane_plan[4];   // stream lane of Proto and of the three segment head levels
  // passes over the built graph (fuse_conv_cv1, fuse_decode, plan_lanes, plan_sub_batches, the stem fusion of annotate_ops)
  bool no_cvfuse, decfuse, no_lanes, no_subbatch;
  bool no_stemfuse;   // (also a process switch: ProcSwitches::no_stemfuse)
  int subbatch, subbatch_ops;
  // plan_route
  bool no_protor, no_halo, no_c32, no_w1_split, no_w1, no_slab, no_planes_s2, no_planes_m64, no_planes, no_headtail, no_s2c32,
      no_s2c64;
  int k1_tile;          // -1 = unset
  long headtail_maxm;   // 0 = unset
};
PlanSwitches read_plan_switches();

// Read on every call, never cached: each is changed inside one process.
bool live_no_stem2();             // tests/test_engine_gpu.py runs one engine's forward with and without it
bool live_no_dgrad_phases();      // tests/test_backward_ops_gpu.py compares the two forms of m355_conv2d_dgrad in one process
bool live_pair64();               // tests/test_c2f_fused_gpu.py sets it around one engine's creation and its m355_bneck_pair_fwd calls
const char* live_stamps_path();   // nullptr = unset.  tools/stamps_*.py and tools/bneck_bench.py set it (and the next) after the
int live_bneck_reps();            // 0 = unset.        library is loaded, for the entry calls that follow

}  // namespace m355
