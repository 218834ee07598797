// The one reader of the M355_* environment switches (switches.h).  Host code only.  One line per switch: field, name, default.
#include "switches.h"

#include <limits.h>
#include <stdlib.h>

namespace m355 {

namespace {

bool env_set(const char* name) { return getenv(name) != nullptr; }
long env_int(const char* name, long unset) {
  const char* v = getenv(name);
  return v ? atol(v) : unset;
}

ProcSwitches read_proc_switches() {
  ProcSwitches v{};
  v.no_fast_epi = env_set("M355_NO_FAST_EPI");
  v.no_wide = env_set("M355_NO_WIDE");
  v.no_m32 = env_set("M355_NO_M32");
  v.no_bias_lds = env_set("M355_NO_BIAS_LDS");
  v.static_tiles = env_set("M355_STATIC_TILES");   // persistent kernels: static tile walk instead of the queue
  v.no_persist = env_set("M355_NO_PERSIST");
  v.stem_gather = env_set("M355_STEM_GATHER");
  v.persist = env_int("M355_PERSIST", 0);            // bit 0: 1x1 convs, bit 1: the others, on the persistent im2col kernel
  v.halo_variant = env_int("M355_HALO_VARIANT", 2);
  v.smallm = env_int("M355_SMALLM", 300);
  v.c2f_noprio = env_set("M355_C2F_NOPRIO");         // experiment: no s_setprio(1) around the K loops
  v.c2f_stamps = getenv("M355_C2F_STAMPS");          // diagnostic: <file> -> per-wave section cycles of the LAST launch, written after a stream sync [sync]
  // covered / real pixels allowed, in tenths: 3.0 since round 3 (was 1.3) -- the 32 -> 32 convs of the smaller head levels
  // (40 x 40: 1.44, 20 x 20: 2.56) are latency-bound launches of a few MFLOP per CU, where empty tile area costs less than the
  // im2col kernel's prologue: 16.5 -> 8.6 us and 16.3 -> 7.8 us at batch 32
  v.c32_waste = env_int("M355_C32_WASTE", 30);
  v.c32_slots = env_int("M355_C32_SLOTS", -1);       // resident blocks; unset: two per CU
  v.m32_slots = env_int("M355_M32_SLOTS", -1);       // unset: as many per CU as the LDS and the register budget take
  v.wide_slots = env_int("M355_WIDE_SLOTS", -1);     // unset: two per CU
  v.wide_stagger = env_int("M355_WIDE_STAGGER", -1); // unset: 0
  v.s2c32_dbg = env_int("M355_S2C32_DBG", 0);
  // diagnostic: per-wave section cycles.  M355_S2C32_STAMPS=<file>: the LAST launch, written after a stream sync [sync];
  // M355_S2C32_RING=<n> with it: the last n launches into a device ring, no sync, written at process exit.
  v.s2c32_stamps = getenv("M355_S2C32_STAMPS");
  v.s2c32_ring = env_int("M355_S2C32_RING", 0);
  v.s2c64_prio = env_int("M355_S2C64_PRIO", 0);      // experiment: s_setprio(1) around the K loop
  v.s2c64_stamps = getenv("M355_S2C64_STAMPS");      // diagnostic: as M355_C2F_STAMPS [sync]
  v.protor_prio = env_int("M355_PROTOR_PRIO", 0);    // experiment: s_setprio(1) around the K loop
  v.protor_stamps = getenv("M355_PROTOR_STAMPS");    // diagnostic: as M355_C2F_STAMPS [sync]
  v.stem2_nxb = env_int("M355_STEM2_NXB", 7);        // stem blocks per wave of team X (of 9; the rest go to team Y), clamped to 5..9
  v.no_stemfuse = env_set("M355_NO_STEMFUSE");
  v.sppf_minblocks = env_int("M355_SPPF_MINBLOCKS", 256);   // one block per CU
  v.mask_dbg = env_int("M355_MASK_DBG", 0);          // timing ablations: 1 zero fill only, 2 no stores
  v.mask_tile = env_int("M355_MASK_TILE", 0);        // 1: the 16 x 16-cell tile (experiments)
  v.no_dgrad_s2c32 = env_set("M355_NO_DGRAD_S2C32");
  v.no_wgrad_stem = env_set("M355_NO_WGRAD_STEM");
  v.no_wgrad_s2c32 = env_set("M355_NO_WGRAD_S2C32");
  v.no_wgrad3 = env_set("M355_NO_WGRAD3");
  // 1x1 convs of the training step on conv1x1_wreg.hip: 27.4-27.5 -> 27.2-27.3 ms per s-seg b64 step on one box
  v.no_train_w1 = env_set("M355_NO_TRAIN_W1");
  v.no_train_c32 = env_set("M355_NO_TRAIN_C32");     // 32 -> 32 3x3 layers on conv3x3_c32.hip: a further -0.1 ms
  v.wgrad_blocks = env_int("M355_WGRAD_BLOCKS", 384);   // measured (s-seg b64 @640 step): 256 -> 49.0 ms, 384 -> 46.1, 512 -> 47.7, 1024 -> 49.3
  v.w2_blocks_x2 = env_int("M355_W2_BLOCKS_X2", 4);  // blocks per CU x 2 (tuning)
  v.wgrad3_shrink = env_int("M355_WGRAD3_SHRINK", 0);   // experiments: 1 halve ci, 2 halve co, 3 both when the layer is one tile
  v.wgrad3_blocks = env_int("M355_WGRAD3_BLOCKS", 512);
  v.wgrad3_mintiles = env_int("M355_WGRAD3_MINTILES", 8);
  v.wgrad3_slabmb = env_int("M355_WGRAD3_SLABMB", 96);
  return v;
}

}  // namespace

const ProcSwitches& proc_switches() {
  static const ProcSwitches v = read_proc_switches();
  return v;
}

PlanSwitches read_plan_switches() {
  PlanSwitches v{};
  v.no_c2f32 = env_set("M355_NO_C2F32");
  v.no_pair = env_set("M355_NO_PAIR");
  v.no_protofuse = env_set("M355_NO_PROTOFUSE");
  v.no_protofuse3 = env_set("M355_NO_PROTOFUSE3");
  v.no_upfuse = env_set("M355_NO_UPFUSE");
  // the second 3x3 stage of head levels 1 and 2 (cv2.l.1 + cv3.l.1 + cv4.l.1) as three launches instead of one block-diagonal launch
  v.no_headdiag = env_set("M355_NO_HEADDIAG");
  v.headdiag_l0 = env_set("M355_HEADDIAG_L0");   // experiment: also the 80 x 80 level
  // digits 0..3, Proto first; a shorter string or a bad digit keeps the rest.  Default measured best on MI355X at batch 32
  const int lanes[4] = {1, 2, 2, 0};
  const char* lp = getenv("M355_LANE_PLAN");
  for (int i = 0; i < 4; ++i) {
    if (lp && (lp[i] < '0' || lp[i] > '3')) lp = nullptr;
    v.lane_plan[i] = lp ? lp[i] - '0' : lanes[i];
  }
  v.no_cvfuse = env_set("M355_NO_CVFUSE");
  // measured at batch 32: 179 us for the three launches against 93 + 39 us separately, -1 % end to end (two serial 64-pixel
  // passes with four barriers each behind every tile): opt-in
  v.decfuse = env_set("M355_DECFUSE");
  v.no_lanes = env_set("M355_NO_LANES");
  v.no_subbatch = env_set("M355_NO_SUBBATCH");
  v.no_stemfuse = env_set("M355_NO_STEMFUSE");
  v.subbatch = env_int("M355_SUBBATCH", 0);   // images per pass; measured at batch 32 with two engines in flight: 8 -> -5 %, 16 -> -2 %: off by default
  v.subbatch_ops = env_int("M355_SUBBATCH_OPS", INT_MAX);   // at most this many leading ops
  v.no_protor = env_set("M355_NO_PROTOR");
  v.no_halo = env_set("M355_NO_HALO");
  v.no_c32 = env_set("M355_NO_C32");
  v.no_w1_split = env_set("M355_NO_W1_SPLIT");
  v.no_w1 = env_set("M355_NO_W1");
  v.no_slab = env_set("M355_NO_SLAB");
  v.no_planes_s2 = env_set("M355_NO_PLANES_S2");
  v.no_planes_m64 = env_set("M355_NO_PLANES_M64");
  v.no_planes = env_set("M355_NO_PLANES");
  v.no_headtail = env_set("M355_NO_HEADTAIL");
  v.no_s2c32 = env_set("M355_NO_S2C32");
  v.no_s2c64 = env_set("M355_NO_S2C64");
  v.k1_tile = env_int("M355_K1_TILE", -1);           // im2col tile id of the 1x1 convs the heuristic gives 128x128
  v.headtail_maxm = env_int("M355_HEADTAIL_MAXM", 0);   // testing: a head level with more pixels than this counts as ineligible
  return v;
}

bool live_no_stem2() { return env_set("M355_NO_STEM2"); }
bool live_no_dgrad_phases() { return env_set("M355_NO_DGRAD_PHASES"); }
bool live_pair64() { return env_set("M355_PAIR64"); }
const char* live_stamps_path() { return getenv("M355_STAMPS"); }
int live_bneck_reps() { return env_int("M355_BNECK_REPS", 0); }

}  // namespace m355
