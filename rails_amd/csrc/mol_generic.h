// The shape-generic fp32 scoring route (mol_generic.hip): runtime-shape kernels for the MoL shapes that have no fused kernel.
//
// Layouts (all fp32, row-major, padded to the kernels' vector width):
//   item index   per item  [P_X][dp] Ex (dp = d rounded up to 8, pad = 0), then [Lq] gi (Lq = L rounded up to 4, pad = 0);
//                the buffer holds a whole number of 32-item tiles, rows beyond n_items are zeros
//   query pack   per query [P_Q][dp] Eq / tau (pad = 0), then [Lq] gq
//   gate pack    W1 and W2 in the A-operand order of v_mfma_f32_32x32x2_f32 (zero-padded to Hp = H rounded up to 32 and
//                Lp = L rounded up to 32), then b1 [Hp], b2 [Lp]
// Eq, Ex, gq and gi are computed by the prologue / index-build kernels of the fused route (mol_query.hip, mol_index.hip), which
// only write them in this layout instead of fragment order: the same values on both routes.
#pragma once
#include "mol_kernels.h"

namespace mol {

constexpr int kGenericMaxL = 256, kGenericMaxD = 256, kGenericMaxH = 512;

inline int gen_dp(const Shape& s) { return (s.dot_product_dimension + 7) / 8 * 8; }
inline int gen_lq(const Shape& s) { return (num_logits(s) + 3) / 4 * 4; }
inline int gen_lp(const Shape& s) { return (num_logits(s) + 31) / 32 * 32; }
inline int gen_hp(const Shape& s) { return (s.gating_qi_hidden_dim + 31) / 32 * 32; }
inline int64_t gen_item_floats(const Shape& s) { return (int64_t)s.item_dot_product_groups * gen_dp(s) + gen_lq(s); }
inline int64_t gen_query_floats(const Shape& s) { return (int64_t)s.query_dot_product_groups * gen_dp(s) + gen_lq(s); }
inline size_t gen_gate_pack_floats(const Shape& s) { return 2 * (size_t)gen_hp(s) * gen_lp(s) + gen_hp(s) + gen_lp(s); }

// LDS of the prologue / index-build kernels for a shape (the limits the generic route inherits from them)
size_t index_build_lds_bytes(const Shape& s);
size_t query_prologue_lds_bytes(const Shape& s);
constexpr size_t kQueryPrologueMaxLds = 64 * 1024;
constexpr size_t kIndexBuildMaxLds = 160 * 1024;

// mol_index.hip / mol_query.hip: the fused route's arithmetic, written row-major (`ld` floats per item / query)
int index_build_plain(const Shape& s, const Weights& w, const float* items, int64_t n, float* out, int64_t ld, int dp, int lq, hipStream_t stream);
int index_update_plain(const Shape& s, const Weights& w, const float* items, int64_t n, const int64_t* positions, float* out, int64_t n_index, int64_t ld,
                       int dp, int lq, hipStream_t stream);
int query_prologue_plain(const Shape& s, const Weights& w, const float* q, const int64_t* user_ids, int B, float* qpack, int64_t ld, int dp,
                         float* eq_out, float* gq_out, hipStream_t stream);

struct GenericScoreArgs {
  const float* wpack;
  const float* qpack;
  const float* ipack;
  float* logits;
  int64_t ld;
  int64_t n_items;      // shared corpus: items of the index; per-row candidates: candidates per row
  int B;
  int per_row;          // 1: candidate j of row b is item row b * n_items + j
  const int32_t* run_if;
  // candidates scored in place (the indexed mode): candidate j of row b is item cand_pos[b * n_items + j] of the shared index `ipack` of
  // index_items items, clamped into it; cand_count (optional): only the first cand_count[b] slots of row b are scored and written
  const int64_t* cand_pos;
  const int32_t* cand_count;
  int64_t index_items;
  // the explaining mode (both non-NULL, per_row or cand_pos, cand_count NULL): the L cross logits and the L mixture weights of every scored pair,
  // (B, n_items, L) row-major each
  float* cl_out;
  float* pi_out;
};
int generic_pack_gate_weights(const Shape& s, const Weights& w, float* wpack, hipStream_t stream);
int generic_index_unpack(const Shape& s, const float* ipack, int64_t n, float* ex, float* gi, hipStream_t stream);
int generic_score(const Shape& s, const GenericScoreArgs& a, int n_cu, hipStream_t stream);

// The backward of the per-row-candidates launch (mol_generic_bwd.hip): gradients of sum(dy * logits).
//   wtpack      W2^T and W1^T in the A-operand orders of W1 and W2 (generic_pack_gate_weights_t), gen_gate_pack_t_floats floats
//   d_qpack     (B, query_floats): dEq (of the UNSCALED Eq: the 1/tau of the pack is applied) and dgq in the query pack's layout, pads zero; or NULL
//   d_ipack     (B * n_cand, item_floats): dEx and dgi in the item pack's layout, pads zero; or NULL
//   dw1 .. db2  (H, L), (H), (L, H), (L) row-major, all four or none; with them `workspace` of generic_backward_workspace_floats(chunk_pairs)
//               floats: the rows run in chunks of at most chunk_pairs pairs (whole rows; a row longer than the chunk is refused)
constexpr int kGenericBwdMaxQTiles = 4;
inline size_t gen_gate_pack_t_floats(const Shape& s) { return 2 * (size_t)gen_hp(s) * gen_lp(s); }
struct GenericBackwardArgs {
  const float *wpack, *wtpack, *qpack, *ipack, *dy;
  int64_t ld_dy, n_cand;
  int B;
  float *d_qpack, *d_ipack, *dw1, *db1, *dw2, *db2, *workspace;
  int64_t chunk_pairs;
};
int generic_pack_gate_weights_t(const Shape& s, const Weights& w, float* wtpack, hipStream_t stream);
bool generic_backward_supported(const Shape& s);      // sets the error text when not
size_t generic_backward_workspace_floats(const Shape& s, int64_t chunk_pairs);
int generic_pair_backward(const Shape& s, const GenericBackwardArgs& a, int n_cu, hipStream_t stream);

// The bf16 candidate tables of the two-pass algorithms, cut from the generic index (mol_coarse.hip): rows of gen_table_width(s) columns,
// the columns d .. width exact zeros, so that the bf16 scans run their d = 32 / 64 / 128 instantiations on them.  0: d > 128, no table.
inline int gen_table_width(const Shape& s) {
  const int d = s.dot_product_dimension;
  return d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : 0;
}
// positions == NULL: the build of an n-row table from the n items of `ipack`; else rows positions[0 .. m) of a table of n rows, each from the
// item of the same position
int generic_coarse_table(const Shape& s, const float* ipack, const int64_t* positions, int64_t m, void* table, int64_t n, hipStream_t stream);
int generic_component_table(const Shape& s, const float* ipack, const int64_t* positions, int64_t m, void* table, int64_t n, hipStream_t stream);
// eq (rows, d) fp32 -> out (rows, width) fp32, the columns d .. width zeros
int generic_eq_pad(const Shape& s, const float* eq, int64_t rows, float* out, hipStream_t stream);

}  // namespace mol
