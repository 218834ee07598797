// Host-side weight packing (weight_pack.hip), shared by m355_set_conv_weights (engine.hip) and the per-op entries
// (op_entries.hip): fp32 PyTorch weights -> the fp16 row and MFMA-fragment layouts the kernels read.  Each layout is written
// once, so a parity entry packs exactly what the engine runs.  Host only: no kernel file includes this header.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace m355 {

// the error text of the C-ABI calls made without an engine (m355_last_error(nullptr)), set in engine.hip and, through
// set_err, by the per-op entries (op_entries.hip, dfine_entries.hip)
extern thread_local std::string g_err;
inline int set_err(int code, const std::string& m) {
  g_err = m;
  return code;
}

using FragList = std::vector<std::pair<int, int>>;   // (first row of a 32-row block, first K element of a 16-deep slice)

// fp16 rows
void pack_conv_rows(const float* w, int cout, int cin, int k, int Kpad, int row0, std::vector<half_t>& dst, int koff = 0);
void pack_convt2x2_rows(const float* w, int cin, int cout, int Kpad, std::vector<half_t>& dst);
std::vector<half_t> pack_stem3x3(const float* w, int cout);
std::vector<half_t> to_half_vec(const float* w, size_t n);
void compose_proto_phases(int n, const float* wtp, const float* btp, const float* w3p, const float* b3p, int cout_pad, int Kpad,
                          std::vector<half_t>& rows, std::vector<float>& btab);

// MFMA A-fragment copies of packed rows, and the fragment lists of the kernels that read them
std::vector<half_t> frag_pack(const half_t* rows, int Kpad, const FragList& frags, bool operand);
FragList frag_grid(int rows, int K);
FragList frag_list(int k, int cin, int cout);
FragList head_level_frags(int nc);
FragList epilogue_frags(int cout2, int k);

// row-slab 3x3 kernels (conv3x3_planes.hip): a conv of cout channels occupies planes_cblocks(cout) 32-channel blocks
std::vector<half_t> planes_frag_pack(const half_t* rows, int Kpad, int cin, int cblocks);
inline int planes_cblocks(int cout) { return (cout + 63) / 64 * 2; }
std::vector<half_t> planes_frag_pack_padded(const half_t* rows, int cout, int Kpad, int cin);
std::vector<half_t> planes_frag_pack_diag(const half_t* const* rows, const int* cout, const int* kpad, const int* cin, int n);

}  // namespace m355
