// extern "C" entry points declared in include/rails_amd.h: argument validation + dispatch.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>

#include "mol_generic.h"
#include "mol_kernels.h"
#include "mol_layout.h"

namespace mol {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int fail(int code, const char* what) {
  if (code == kOk) return code;
  if (code == kErrLaunch) {
    const hipError_t e = hipGetLastError();
    set_error("%s: HIP launch failed (%s)", what, hipGetErrorString(e));
  } else if (g_err[0] == '\0' || code == kErrInvalid) {
    if (g_err[0] == '\0') set_error("%s: error %d", what, code);
  }
  return code;
}

static bool shape_ok(const Shape* s) {
  if (!s) { set_error("shape is NULL"); return false; }
  if (s->query_embedding_dim <= 0 || s->item_embedding_dim <= 0 || s->dot_product_dimension <= 0 ||
      s->query_dot_product_groups <= 0 || s->item_dot_product_groups <= 0) {
    set_error("shape has a non-positive dimension");
    return false;
  }
  if (s->num_uid_tables < 0 || s->num_uid_tables > RAILS_MAX_UID_TABLES ||
      s->num_uid_tables >= s->query_dot_product_groups) {
    set_error("num_uid_tables = %d out of range", s->num_uid_tables);
    return false;
  }
  if (!(s->temperature > 0.0f)) { set_error("temperature must be > 0"); return false; }
  return true;
}

static bool shape_supported(const Shape* s) {
  if (!shape_ok(s)) return false;
  if (s->gating_qi_hidden_dim <= 0 && (s->precision != RAILS_PRECISION_FP32 || !score_extra_shape(*s))) {
    set_error("a pair gate without hidden layer (gating_qi_hidden_dim <= 0) is built in precision fp32 for P_Q x P_X x d = 8x8x32, 8x4x64, 16x4x32 "
              "(mol_score_extra_shapes.h)");
    return false;
  }
  if (s->gating_combination != RAILS_COMBINE_GLU_SILU && s->gating_combination != RAILS_COMBINE_NONE) {
    set_error("gating_combination must be RAILS_COMBINE_GLU_SILU or RAILS_COMBINE_NONE, got %d", s->gating_combination);
    return false;
  }
  if (s->gating_combination == RAILS_COMBINE_GLU_SILU && (!s->gating_has_query || !s->gating_has_item)) {
    set_error("gating_combination glu_silu needs the query-only and the item-only gate part (the reference multiplies them)");
    return false;
  }
  if ((s->gating_has_query && s->gating_query_hidden_dim <= 0) || (s->gating_has_item && s->gating_item_hidden_dim <= 0)) {
    set_error("gating hidden dims must be > 0 for the gate parts that exist");
    return false;
  }
  if (s->precision != RAILS_PRECISION_FP32 && s->precision != RAILS_PRECISION_F16X3 && s->precision != RAILS_PRECISION_F16X1) {
    set_error("precision must be RAILS_PRECISION_FP32, _F16X3 or _F16X1, got %d", s->precision);
    return false;
  }
  if (is_split(*s) && !s->dot_product_l2_norm) {
    set_error("precision f16x3 needs dot_product_l2_norm = 1 (cross logits bounded by 1/temperature keep the f16 operands in range)");
    return false;
  }
  if (!score_supported(*s)) {
    set_error("no fused scoring kernel for P_Q x P_X x d = %dx%dx%d with gating_qi_hidden_dim = %d "
              "(built: 8x4x64, 8x4x128, 8x8x32, 16x16x64 with 128)",
              s->query_dot_product_groups, s->item_dot_product_groups, s->dot_product_dimension,
              s->gating_qi_hidden_dim);
    return false;
  }
  return true;
}

// The generic route's envelope (mol_generic.h): answered without a device.
static bool generic_supported(const Shape* s) {
  if (!shape_ok(s)) return false;
  if (s->precision != RAILS_PRECISION_FP32) {
    set_error("the generic scoring route is exact fp32 only (precision RAILS_PRECISION_FP32), got precision %d", s->precision);
    return false;
  }
  if (s->gating_qi_hidden_dim <= 0) {
    set_error("the generic scoring route needs a pair gate with a hidden layer (gating_qi_hidden_dim >= 1)");
    return false;
  }
  if (s->gating_qi_hidden_dim > kGenericMaxH) {
    set_error("the generic scoring route takes gating_qi_hidden_dim <= %d, got %d", kGenericMaxH, s->gating_qi_hidden_dim);
    return false;
  }
  if ((int64_t)s->query_dot_product_groups * s->item_dot_product_groups > kGenericMaxL) {
    set_error("the generic scoring route takes P_Q * P_X <= %d, got %dx%d = %lld", kGenericMaxL, s->query_dot_product_groups,
              s->item_dot_product_groups, (long long)s->query_dot_product_groups * s->item_dot_product_groups);
    return false;
  }
  if (s->dot_product_dimension > kGenericMaxD) {
    set_error("the generic scoring route takes dot_product_dimension <= %d, got %d", kGenericMaxD, s->dot_product_dimension);
    return false;
  }
  if (s->gating_combination != RAILS_COMBINE_GLU_SILU && s->gating_combination != RAILS_COMBINE_NONE) {
    set_error("gating_combination must be RAILS_COMBINE_GLU_SILU or RAILS_COMBINE_NONE, got %d", s->gating_combination);
    return false;
  }
  if (s->gating_combination == RAILS_COMBINE_GLU_SILU && (!s->gating_has_query || !s->gating_has_item)) {
    set_error("gating_combination glu_silu needs the query-only and the item-only gate part (the reference multiplies them)");
    return false;
  }
  if ((s->gating_has_query && s->gating_query_hidden_dim <= 0) || (s->gating_has_item && s->gating_item_hidden_dim <= 0)) {
    set_error("gating hidden dims must be > 0 for the gate parts that exist");
    return false;
  }
  if (index_build_lds_bytes(*s) > kIndexBuildMaxLds) {
    set_error("index build needs %zu B of LDS (> 160 KiB) for this shape", index_build_lds_bytes(*s));
    return false;
  }
  if (query_prologue_lds_bytes(*s) > kQueryPrologueMaxLds) {
    set_error("query prologue needs %zu B of LDS (> 64 KiB) for this shape", query_prologue_lds_bytes(*s));
    return false;
  }
  return true;
}

static int compute_units() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
  return n;
}

}  // namespace mol

using namespace mol;

extern "C" {

const char* rails_last_error(void) { return g_err; }

int rails_device_compute_units(void) {
  const int n = compute_units();
  if (n < 0) { set_error("no HIP device"); return RAILS_ELAUNCH; }
  return n;
}

int rails_mol_shape_supported(const rails_mol_shape* shape) { return shape_supported(shape) ? 1 : 0; }

size_t rails_mol_gate_pack_floats(const rails_mol_shape* s) {
  if (!shape_ok(s)) return 0;
  // the small-unit kernel's shapes carry the pair-gate weights twice: 32x32x2 fragment order, then 16x16x4 fragment order
  return gate_pack32_floats(*s) * (score_small_shape(*s) ? 2 : 1);
}

int rails_mol_pack_gate_weights(const rails_mol_shape* s, const rails_mol_weights* w, float* gate_pack, void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (!w || !gate_pack || !w->gqi_w1 || !w->gqi_b1 || (s->gating_qi_hidden_dim > 0 && (!w->gqi_w2 || !w->gqi_b2))) {
    set_error("pack_gate_weights: NULL pointer");
    return RAILS_EINVAL;
  }
  if (is_split(*s)) return fail(pack_gate_weights_split(*s, *w, gate_pack, (hipStream_t)stream), "pack_gate_weights");
  return fail(pack_gate_weights(*s, *w, gate_pack, (hipStream_t)stream), "pack_gate_weights");
}

size_t rails_mol_index_floats(const rails_mol_shape* s, int64_t n_items) {
  if (!shape_ok(s) || n_items < 0) return 0;
  return (size_t)(num_tiles(n_items) * tile_floats(*s));
}

int rails_mol_index_build(const rails_mol_shape* s, const rails_mol_weights* w, const float* items, int64_t n_items,
                          float* index, void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (n_items < 0) { set_error("index_build: n_items < 0"); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!w || !items || !index || !w->i_proj_w || !w->i_proj_b || (s->gating_has_item && (!w->gi_w1 || !w->gi_b1 || !w->gi_w2)) ||
      (s->item_hidden_dim > 0 && (!w->i_glu_w || !w->i_glu_b))) {
    set_error("index_build: NULL pointer");
    return RAILS_EINVAL;
  }
  int r = index_build(*s, *w, items, n_items, index, (hipStream_t)stream);
  if (r == kOk && is_split(*s)) r = index_split_inplace(*s, index, n_items, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "index_build");
}

static bool build_weights_ok(const rails_mol_shape* s, const rails_mol_weights* w) {
  return w && w->i_proj_w && w->i_proj_b && !(s->gating_has_item && (!w->gi_w1 || !w->gi_b1 || !w->gi_w2)) &&
         !(s->item_hidden_dim > 0 && (!w->i_glu_w || !w->i_glu_b));
}

int rails_mol_index_update(const rails_mol_shape* s, const rails_mol_weights* w, const float* items, int64_t n_new, const int64_t* positions,
                           float* index, int64_t n_items, void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (n_new < 0 || n_items < 0) { set_error("index_update: negative size"); return RAILS_EINVAL; }
  if (n_new == 0) return RAILS_OK;
  if (!items || !positions || !index || !build_weights_ok(s, w)) { set_error("index_update: NULL pointer"); return RAILS_EINVAL; }
  const int r = index_update(*s, *w, items, n_new, positions, index, n_items, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "index_update");
}

int rails_mol_index_rows_update(const rails_mol_shape* s, const float* index, int64_t n_items, const int64_t* positions, int64_t n_new, float* rows,
                                void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (is_split(*s)) { set_error("index_rows_update: exact-fp32 index only"); return RAILS_ENOTSUP; }
  if (n_new < 0 || n_items < 0) { set_error("index_rows_update: negative size"); return RAILS_EINVAL; }
  if (n_new == 0) return RAILS_OK;
  if (!index || !positions || !rows) { set_error("index_rows_update: NULL pointer"); return RAILS_EINVAL; }
  return fail(index_rows_update(*s, index, n_items, positions, n_new, rows, (hipStream_t)stream), "index_rows_update");
}

int rails_mol_index_clear_tail(const rails_mol_shape* s, float* index, int64_t n_items, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (n_items < 0) { set_error("index_clear_tail: n_items < 0"); return RAILS_EINVAL; }
  if (n_items % 32 == 0) return RAILS_OK;
  if (!index) { set_error("index_clear_tail: NULL pointer"); return RAILS_EINVAL; }
  return fail(tile_clear_tail(index, n_items, tile_floats(*s), (hipStream_t)stream), "index_clear_tail");
}

int rails_mol_index_unpack(const rails_mol_shape* s, const float* index, int64_t n_items, float* ex_out, float* gi_out,
                           void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (n_items <= 0 || (!ex_out && !gi_out)) return RAILS_OK;
  if (!index) { set_error("index_unpack: NULL index"); return RAILS_EINVAL; }
  return fail(index_unpack(*s, index, n_items, ex_out, gi_out, (hipStream_t)stream), "index_unpack");
}

int rails_mol_index_gather(const rails_mol_shape* s, const float* index, int64_t n_items, const int64_t* cand_idx,
                           int64_t n_rows, int64_t n_cand, float* out_index, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (n_rows < 0 || n_cand < 0) { set_error("index_gather: negative size"); return RAILS_EINVAL; }
  if (n_rows == 0 || n_cand == 0) return RAILS_OK;
  if (!index || !cand_idx || !out_index) { set_error("index_gather: NULL pointer"); return RAILS_EINVAL; }
  const int r = index_gather(*s, index, n_items, cand_idx, n_rows, n_cand, out_index, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "index_gather");
}

size_t rails_mol_query_pack_floats(const rails_mol_shape* s, int32_t batch) {
  if (!shape_ok(s) || batch < 0) return 0;
  const int QT = queries_per_group(*s);
  const size_t groups = (size_t)((batch + QT - 1) / QT);
  return groups * 32 * (size_t)s->dot_product_dimension + (size_t)batch * (size_t)num_logits(*s) +
         query_scratch_floats(*s, batch);   // + the prologue's own scratch rows (GLU output, first gate layer)
}

static int query_prologue_checked(const rails_mol_shape* s, const rails_mol_weights* w, const float* queries, const int64_t* user_ids,
                                  int32_t batch, float* query_pack, float* query_pack_other, float* eq_out, float* gq_out, void* stream);

int rails_mol_query_prologue(const rails_mol_shape* s, const rails_mol_weights* w, const float* queries,
                             const int64_t* user_ids, int32_t batch, float* query_pack, float* eq_out, float* gq_out,
                             void* stream) {
  return query_prologue_checked(s, w, queries, user_ids, batch, query_pack, nullptr, eq_out, gq_out, stream);
}

int rails_mol_query_prologue_both(const rails_mol_shape* s, const rails_mol_weights* w, const float* queries,
                                  const int64_t* user_ids, int32_t batch, float* query_pack, float* query_pack_other,
                                  void* stream) {
  if (!query_pack_other) { g_err[0] = '\0'; set_error("query_prologue_both: NULL pointer"); return RAILS_EINVAL; }
  return query_prologue_checked(s, w, queries, user_ids, batch, query_pack, query_pack_other, nullptr, nullptr, stream);
}

static int query_prologue_checked(const rails_mol_shape* s, const rails_mol_weights* w, const float* queries, const int64_t* user_ids,
                                  int32_t batch, float* query_pack, float* query_pack_other, float* eq_out, float* gq_out, void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0) { set_error("query_prologue: batch < 0"); return RAILS_EINVAL; }
  if (batch == 0) return RAILS_OK;
  if (!w || !queries || !query_pack || !w->q_proj_w || !w->q_proj_b || (s->query_hidden_dim > 0 && (!w->q_glu_w || !w->q_glu_b)) ||
      (s->gating_has_query && (!w->gq_w1 || !w->gq_b1 || !w->gq_w2))) {
    set_error("query_prologue: NULL pointer");
    return RAILS_EINVAL;
  }
  if (s->num_uid_tables > 0) {
    if (!user_ids) { set_error("query_prologue: user_ids is required when num_uid_tables > 0"); return RAILS_EINVAL; }
    for (int t = 0; t < s->num_uid_tables; ++t)
      if (!w->uid_table[t] || w->uid_hash_size[t] <= 0) { set_error("query_prologue: uid table %d missing", t); return RAILS_EINVAL; }
  }
  return fail(query_prologue(*s, *w, queries, user_ids, batch, query_pack, eq_out, gq_out, (hipStream_t)stream, query_pack_other),
              "query_prologue");
}

// Launch arguments of a scoring pass over a shared corpus (per_row = 0) or per-row candidates (per_row = 1).
static int fill_score_args(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                           int64_t n_items, float* logits, int64_t ld, int per_row, ScoreArgs* out, const int32_t* run_if = nullptr) {
  ScoreArgs a{};
  const int QT = queries_per_group(*s);
  a.n_groups = (batch + QT - 1) / QT;
  a.wpack = gate_pack;
  a.eqfrag = query_pack;
  a.gqfrag = query_pack + (int64_t)a.n_groups * 32 * s->dot_product_dimension;
  a.ipack = index;
  a.logits = logits;
  a.ld = ld;
  a.n_items = n_items;
  a.n_tiles = num_tiles(n_items);
  a.B = batch;
  a.per_row = per_row;
  a.temperature = s->temperature;
  a.rcp_temperature = 1.0f / s->temperature;
  a.split = is_split(*s) ? 1 : 0;
  a.single = s->precision == RAILS_PRECISION_F16X1 ? 1 : 0;
  a.combine_none = s->gating_combination == RAILS_COMBINE_NONE ? 1 : 0;
  a.run_if = run_if;
  *out = a;
  return kOk;
}

static int score_common(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch,
                        const float* index, int64_t n_items, float* logits, int64_t ld, int per_row, void* stream,
                        const char* what, const int32_t* run_if = nullptr) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items < 0) { set_error("%s: negative size", what); return RAILS_EINVAL; }
  if (batch == 0 || n_items == 0) return RAILS_OK;
  if (!gate_pack || !query_pack || !index || !logits) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  if (ld < n_items) { set_error("%s: ld (%lld) < n_items (%lld)", what, (long long)ld, (long long)n_items); return RAILS_EINVAL; }
  if (per_row && n_items % 32 != 0) { set_error("%s: n_cand must be a multiple of 32", what); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("%s: no HIP device", what); return RAILS_ELAUNCH; }
  ScoreArgs a;
  fill_score_args(s, gate_pack, query_pack, batch, index, n_items, logits, ld, per_row, &a, run_if);
  const int r = score_launch(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, what);
}

int rails_mol_score_dense(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch,
                          const float* index, int64_t n_items, float* logits, int64_t ld, const int32_t* run_if, void* stream) {
  return score_common(s, gate_pack, query_pack, batch, index, n_items, logits, ld, 0, stream, "score_dense", run_if);
}

int rails_mol_score_dense_upper_supported(const rails_mol_shape* s) {
  if (!s || !shape_supported(s) || s->precision != RAILS_PRECISION_F16X3) return 0;
  const int cu = compute_units();
  if (cu <= 0) return 0;
  ScoreArgs a;
  fill_score_args(s, nullptr, nullptr, 32, nullptr, 32, nullptr, 32, 0, &a);
  a.upper = 1;
  a.dry_run = 1;
  const int r = score_launch(*s, a, cu, nullptr);
  g_err[0] = '\0';
  return r == kOk ? 1 : 0;
}

int rails_mol_score_dense_upper(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                int64_t n_items, float ub2, float ub1, float ub0, float* logits, int64_t ld, const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items < 0) { set_error("score_dense_upper: negative size"); return RAILS_EINVAL; }
  if (!(ub2 >= 0.0f && ub1 >= 0.0f && ub0 >= 0.0f) || !(ub2 + ub1 + ub0 < INFINITY)) {
    set_error("score_dense_upper: the bound polynomial needs three finite coefficients >= 0");
    return RAILS_EINVAL;
  }
  if (batch == 0 || n_items == 0) return RAILS_OK;
  if (!gate_pack || !query_pack || !index || !logits) { set_error("score_dense_upper: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_items) { set_error("score_dense_upper: ld (%lld) < n_items (%lld)", (long long)ld, (long long)n_items); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("score_dense_upper: no HIP device"); return RAILS_ELAUNCH; }
  ScoreArgs a;
  fill_score_args(s, gate_pack, query_pack, batch, index, n_items, logits, ld, 0, &a, run_if);
  a.upper = 1;
  a.ub2 = ub2;
  a.ub1 = ub1;
  a.ub0 = ub0;
  const int r = score_launch(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "score_dense_upper");
}

int rails_mol_score_indexed_supported(const rails_mol_shape* s, int32_t batch, int64_t n_cand) {
  if (!s || !shape_supported(s) || is_split(*s) || batch <= 0 || n_cand <= 0) return 0;
  const int cu = compute_units();
  if (cu <= 0) return 0;
  ScoreArgs a;
  fill_score_args(s, nullptr, nullptr, batch, nullptr, n_cand, nullptr, n_cand, 1, &a);
  a.cand_pos = reinterpret_cast<const int64_t*>(8);   // never dereferenced: dry run
  a.dry_run = 1;
  const int r = score_launch(*s, a, cu, nullptr);
  g_err[0] = '\0';
  return r == kOk ? 1 : 0;
}

int rails_mol_score_indexed(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                            int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld, void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items <= 0 || n_cand < 0) { set_error("score_indexed: bad size"); return RAILS_EINVAL; }
  if (batch == 0 || n_cand == 0) return RAILS_OK;
  if (!gate_pack || !query_pack || !index || !positions || !logits) { set_error("score_indexed: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("score_indexed: ld < n_cand"); return RAILS_EINVAL; }
  if (is_split(*s)) { set_error("score_indexed: exact-fp32 precision only"); return RAILS_ENOTSUP; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("score_indexed: no HIP device"); return RAILS_ELAUNCH; }
  ScoreArgs a;
  fill_score_args(s, gate_pack, query_pack, batch, index, n_cand, logits, ld, 1, &a);
  a.cand_pos = positions;
  a.index_items = n_items;
  const int r = score_launch(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "score_indexed");
}

size_t rails_mol_index_rows_floats(const rails_mol_shape* s, int64_t n_items) {
  if (!shape_ok(s) || n_items < 0 || is_split(*s)) return 0;
  return (size_t)n_items * (size_t)(tile_floats(*s) / 32);
}

int rails_mol_index_rows_build(const rails_mol_shape* s, const float* index, int64_t n_items, float* rows, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (is_split(*s)) { set_error("index_rows_build: exact-fp32 index only"); return RAILS_ENOTSUP; }
  if (n_items < 0) { set_error("index_rows_build: n_items < 0"); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!index || !rows) { set_error("index_rows_build: NULL pointer"); return RAILS_EINVAL; }
  return fail(index_rows_build(*s, index, n_items, rows, (hipStream_t)stream), "index_rows_build");
}

int rails_mol_score_indexed_rows(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index_rows,
                                 int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld, const int32_t* cand_counts,
                                 void* stream) {
  g_err[0] = '\0';
  if (!shape_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items <= 0 || n_cand < 0) { set_error("score_indexed_rows: bad size"); return RAILS_EINVAL; }
  if (batch == 0 || n_cand == 0) return RAILS_OK;
  if (!gate_pack || !query_pack || !index_rows || !positions || !logits) { set_error("score_indexed_rows: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("score_indexed_rows: ld < n_cand"); return RAILS_EINVAL; }
  if (is_split(*s)) { set_error("score_indexed_rows: exact-fp32 precision only"); return RAILS_ENOTSUP; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("score_indexed_rows: no HIP device"); return RAILS_ELAUNCH; }
  ScoreArgs a;
  fill_score_args(s, gate_pack, query_pack, batch, index_rows, n_cand, logits, ld, 1, &a);
  a.cand_pos = positions;
  a.index_items = n_items;
  a.irows = index_rows;
  a.cand_count = cand_counts;
  const int r = score_launch(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "score_indexed_rows");
}

int rails_mol_score_candidates(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch,
                               const float* cand_index, int64_t n_cand, float* logits, int64_t ld, void* stream) {
  return score_common(s, gate_pack, query_pack, batch, cand_index, n_cand, logits, ld, 1, stream, "score_candidates");
}

// ---- the shape-generic scoring route (mol_generic.hip) ----
int rails_mol_generic_supported(const rails_mol_shape* shape) { g_err[0] = '\0'; return generic_supported(shape) ? 1 : 0; }

size_t rails_mol_generic_gate_pack_floats(const rails_mol_shape* s) { return generic_supported(s) ? gen_gate_pack_floats(*s) : 0; }

size_t rails_mol_generic_index_floats(const rails_mol_shape* s, int64_t n_items) {
  if (!generic_supported(s) || n_items < 0) return 0;
  return (size_t)(num_tiles(n_items) * 32 * gen_item_floats(*s));
}

size_t rails_mol_generic_query_pack_floats(const rails_mol_shape* s, int32_t batch) {
  if (!generic_supported(s) || batch < 0) return 0;
  return (size_t)batch * (size_t)gen_query_floats(*s);
}

int rails_mol_generic_pack_gate_weights(const rails_mol_shape* s, const rails_mol_weights* w, float* gate_pack, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (!w || !gate_pack || !w->gqi_w1 || !w->gqi_b1 || !w->gqi_w2 || !w->gqi_b2) { set_error("generic_pack_gate_weights: NULL pointer"); return RAILS_EINVAL; }
  return fail(generic_pack_gate_weights(*s, *w, gate_pack, (hipStream_t)stream), "generic_pack_gate_weights");
}

int rails_mol_generic_index_build(const rails_mol_shape* s, const rails_mol_weights* w, const float* items, int64_t n_items, float* index,
                                  void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (n_items < 0) { set_error("generic_index_build: n_items < 0"); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!w || !items || !index || !w->i_proj_w || !w->i_proj_b || (s->gating_has_item && (!w->gi_w1 || !w->gi_b1 || !w->gi_w2)) ||
      (s->item_hidden_dim > 0 && (!w->i_glu_w || !w->i_glu_b))) {
    set_error("generic_index_build: NULL pointer");
    return RAILS_EINVAL;
  }
  const int r = index_build_plain(*s, *w, items, n_items, index, gen_item_floats(*s), gen_dp(*s), gen_lq(*s), (hipStream_t)stream);
  return r == kOk ? r : fail(r, "generic_index_build");
}

int rails_mol_generic_index_clear_tail(const rails_mol_shape* s, float* index, int64_t n_items, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (n_items < 0) { set_error("generic_index_clear_tail: n_items < 0"); return RAILS_EINVAL; }
  if (n_items % 32 == 0) return RAILS_OK;
  if (!index) { set_error("generic_index_clear_tail: NULL pointer"); return RAILS_EINVAL; }
  return fail(rows_clear_tail(index, n_items, gen_item_floats(*s), (hipStream_t)stream), "generic_index_clear_tail");
}

int rails_mol_generic_index_update(const rails_mol_shape* s, const rails_mol_weights* w, const float* items, int64_t n_new, const int64_t* positions,
                                   float* index, int64_t n_items, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (n_new < 0 || n_items < 0) { set_error("generic_index_update: negative size"); return RAILS_EINVAL; }
  if (n_new == 0) return RAILS_OK;
  if (!items || !positions || !index || !build_weights_ok(s, w)) { set_error("generic_index_update: NULL pointer"); return RAILS_EINVAL; }
  const int r = index_update_plain(*s, *w, items, n_new, positions, index, n_items, gen_item_floats(*s), gen_dp(*s), gen_lq(*s), (hipStream_t)stream);
  return r == kOk ? r : fail(r, "generic_index_update");
}

int rails_mol_generic_index_unpack(const rails_mol_shape* s, const float* index, int64_t n_items, float* ex_out, float* gi_out, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (n_items <= 0 || (!ex_out && !gi_out)) return RAILS_OK;
  if (!index) { set_error("generic_index_unpack: NULL index"); return RAILS_EINVAL; }
  return fail(generic_index_unpack(*s, index, n_items, ex_out, gi_out, (hipStream_t)stream), "generic_index_unpack");
}

int rails_mol_generic_query_prologue(const rails_mol_shape* s, const rails_mol_weights* w, const float* queries, const int64_t* user_ids,
                                     int32_t batch, float* query_pack, float* eq_out, float* gq_out, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0) { set_error("generic_query_prologue: batch < 0"); return RAILS_EINVAL; }
  if (batch == 0) return RAILS_OK;
  if (!w || !queries || !query_pack || !w->q_proj_w || !w->q_proj_b || (s->query_hidden_dim > 0 && (!w->q_glu_w || !w->q_glu_b)) ||
      (s->gating_has_query && (!w->gq_w1 || !w->gq_b1 || !w->gq_w2))) {
    set_error("generic_query_prologue: NULL pointer");
    return RAILS_EINVAL;
  }
  if (s->num_uid_tables > 0) {
    if (!user_ids) { set_error("generic_query_prologue: user_ids is required when num_uid_tables > 0"); return RAILS_EINVAL; }
    for (int t = 0; t < s->num_uid_tables; ++t)
      if (!w->uid_table[t] || w->uid_hash_size[t] <= 0) { set_error("generic_query_prologue: uid table %d missing", t); return RAILS_EINVAL; }
  }
  const int r = query_prologue_plain(*s, *w, queries, user_ids, batch, query_pack, gen_query_floats(*s), gen_dp(*s), eq_out, gq_out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "generic_query_prologue");
}

static int generic_score_common(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                int64_t n_items, float* logits, int64_t ld, int per_row, const int32_t* run_if, void* stream, const char* what) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items < 0) { set_error("%s: negative size", what); return RAILS_EINVAL; }
  if (batch == 0 || n_items == 0) return RAILS_OK;
  if (!gate_pack || !query_pack || !index || !logits) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  if (ld < n_items) { set_error("%s: ld (%lld) < n_items (%lld)", what, (long long)ld, (long long)n_items); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("%s: no HIP device", what); return RAILS_ELAUNCH; }
  GenericScoreArgs a{};
  a.wpack = gate_pack; a.qpack = query_pack; a.ipack = index; a.logits = logits; a.ld = ld; a.n_items = n_items; a.B = batch;
  a.per_row = per_row; a.run_if = run_if;
  const int r = generic_score(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, what);
}

int rails_mol_generic_score_dense(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                  int64_t n_items, float* logits, int64_t ld, const int32_t* run_if, void* stream) {
  return generic_score_common(s, gate_pack, query_pack, batch, index, n_items, logits, ld, 0, run_if, stream, "generic_score_dense");
}

int rails_mol_generic_score_candidates(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch,
                                       const float* cand_index, int64_t n_cand, float* logits, int64_t ld, const int32_t* run_if, void* stream) {
  return generic_score_common(s, gate_pack, query_pack, batch, cand_index, n_cand, logits, ld, 1, run_if, stream, "generic_score_candidates");
}

int rails_mol_generic_score_indexed(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                    int64_t n_items, const int64_t* positions, int64_t n_cand, const int32_t* counts, float* logits, int64_t ld,
                                    const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items < 0 || n_cand < 0) { set_error("generic_score_indexed: negative size"); return RAILS_EINVAL; }
  if (batch == 0 || n_cand == 0) return RAILS_OK;
  if (n_items == 0) { set_error("generic_score_indexed: candidates of an empty index"); return RAILS_EINVAL; }
  if (!gate_pack || !query_pack || !index || !positions || !logits) { set_error("generic_score_indexed: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("generic_score_indexed: ld (%lld) < n_cand (%lld)", (long long)ld, (long long)n_cand); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("generic_score_indexed: no HIP device"); return RAILS_ELAUNCH; }
  GenericScoreArgs a{};
  a.wpack = gate_pack; a.qpack = query_pack; a.ipack = index; a.logits = logits; a.ld = ld; a.n_items = n_cand; a.B = batch;
  a.per_row = 0; a.run_if = run_if; a.cand_pos = positions; a.cand_count = counts; a.index_items = n_items;
  const int r = generic_score(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "generic_score_indexed");
}

// The explaining launches: the per-row and the indexed launch with the two (batch, n_cand, L) outputs beside the logits.
static int generic_explain_common(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                  int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld, float* component_logits,
                                  float* weights, void* stream, const char* what) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_items < 0 || n_cand < 0) { set_error("%s: negative size", what); return RAILS_EINVAL; }
  if (batch == 0 || n_cand == 0) return RAILS_OK;
  if (positions && n_items == 0) { set_error("%s: candidates of an empty index", what); return RAILS_EINVAL; }
  if (!gate_pack || !query_pack || !index || !logits || !component_logits || !weights) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("%s: ld (%lld) < n_cand (%lld)", what, (long long)ld, (long long)n_cand); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("%s: no HIP device", what); return RAILS_ELAUNCH; }
  GenericScoreArgs a{};
  a.wpack = gate_pack; a.qpack = query_pack; a.ipack = index; a.logits = logits; a.ld = ld; a.n_items = n_cand; a.B = batch;
  a.per_row = positions ? 0 : 1; a.cand_pos = positions; a.index_items = n_items;
  a.cl_out = component_logits; a.pi_out = weights;
  const int r = generic_score(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, what);
}

int rails_mol_generic_explain(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* cand_index,
                              int64_t n_cand, float* logits, int64_t ld, float* component_logits, float* weights, void* stream) {
  return generic_explain_common(s, gate_pack, query_pack, batch, cand_index, 0, nullptr, n_cand, logits, ld, component_logits, weights, stream,
                                "generic_explain");
}

int rails_mol_generic_explain_indexed(const rails_mol_shape* s, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                      int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld, float* component_logits,
                                      float* weights, void* stream) {
  if (!positions) { g_err[0] = '\0'; set_error("generic_explain_indexed: NULL pointer"); return RAILS_EINVAL; }
  return generic_explain_common(s, gate_pack, query_pack, batch, index, n_items, positions, n_cand, logits, ld, component_logits, weights, stream,
                                "generic_explain_indexed");
}

// ---- the backward of the per-row-candidates launch (mol_generic_bwd.hip) ----
int rails_mol_generic_pair_backward_supported(const rails_mol_shape* s) {
  g_err[0] = '\0';
  return generic_supported(s) && generic_backward_supported(*s) ? 1 : 0;
}

size_t rails_mol_generic_gate_pack_t_floats(const rails_mol_shape* s) { return generic_supported(s) ? gen_gate_pack_t_floats(*s) : 0; }

int rails_mol_generic_pack_gate_weights_t(const rails_mol_shape* s, const rails_mol_weights* w, float* gate_pack_t, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (!w || !gate_pack_t || !w->gqi_w1 || !w->gqi_w2) { set_error("generic_pack_gate_weights_t: NULL pointer"); return RAILS_EINVAL; }
  return fail(generic_pack_gate_weights_t(*s, *w, gate_pack_t, (hipStream_t)stream), "generic_pack_gate_weights_t");
}

size_t rails_mol_generic_pair_backward_workspace_bytes(const rails_mol_shape* s, int64_t chunk_pairs) {
  if (!generic_supported(s) || chunk_pairs < 1) return 0;
  return sizeof(float) * generic_backward_workspace_floats(*s, chunk_pairs);
}

int rails_mol_generic_pair_backward(const rails_mol_shape* s, const float* gate_pack, const float* gate_pack_t, const float* query_pack, int32_t batch,
                                    const float* cand_index, int64_t n_cand, const float* dy, int64_t ld_dy, float* d_query_pack,
                                    float* d_cand_index, float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes,
                                    int64_t chunk_pairs, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (!generic_backward_supported(*s)) return RAILS_ENOTSUP;
  if (batch < 0 || n_cand < 0) { set_error("generic_pair_backward: negative size"); return RAILS_EINVAL; }
  if (batch == 0) return RAILS_OK;
  if (n_cand == 0) {      // sums over no pairs: the query side and the weight gradients are zeros (d_cand_index has no rows)
    hipStream_t st = (hipStream_t)stream;
    bool ok = !d_query_pack || hipMemsetAsync(d_query_pack, 0, sizeof(float) * (size_t)batch * gen_query_floats(*s), st) == hipSuccess;
    const size_t L = (size_t)num_logits(*s), H = (size_t)s->gating_qi_hidden_dim;
    ok = ok && (!dw1 || hipMemsetAsync(dw1, 0, sizeof(float) * H * L, st) == hipSuccess) && (!db1 || hipMemsetAsync(db1, 0, sizeof(float) * H, st) == hipSuccess);
    ok = ok && (!dw2 || hipMemsetAsync(dw2, 0, sizeof(float) * H * L, st) == hipSuccess) && (!db2 || hipMemsetAsync(db2, 0, sizeof(float) * L, st) == hipSuccess);
    return ok ? RAILS_OK : fail(kErrLaunch, "generic_pair_backward");
  }
  if (!gate_pack || !gate_pack_t || !query_pack || !cand_index || !dy) { set_error("generic_pair_backward: NULL pointer"); return RAILS_EINVAL; }
  if (ld_dy < n_cand) { set_error("generic_pair_backward: ld_dy (%lld) < n_cand (%lld)", (long long)ld_dy, (long long)n_cand); return RAILS_EINVAL; }
  const int n_w = (dw1 ? 1 : 0) + (db1 ? 1 : 0) + (dw2 ? 1 : 0) + (db2 ? 1 : 0);
  if (n_w != 0 && n_w != 4) { set_error("generic_pair_backward: dw1, db1, dw2, db2 are given together or not at all"); return RAILS_EINVAL; }
  if (n_w == 4) {
    if (chunk_pairs < 1) { set_error("generic_pair_backward: chunk_pairs < 1"); return RAILS_EINVAL; }
    if (!workspace || workspace_bytes < rails_mol_generic_pair_backward_workspace_bytes(s, chunk_pairs)) {
      set_error("generic_pair_backward: workspace shorter than rails_mol_generic_pair_backward_workspace_bytes");
      return RAILS_ENOMEM;
    }
  }
  const int cu = compute_units();
  if (cu <= 0) { set_error("generic_pair_backward: no HIP device"); return RAILS_ELAUNCH; }
  GenericBackwardArgs a{};
  a.wpack = gate_pack; a.wtpack = gate_pack_t; a.qpack = query_pack; a.ipack = cand_index; a.dy = dy; a.ld_dy = ld_dy; a.n_cand = n_cand; a.B = batch;
  a.d_qpack = d_query_pack; a.d_ipack = d_cand_index; a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2;
  a.workspace = static_cast<float*>(workspace); a.chunk_pairs = chunk_pairs;
  const int r = generic_pair_backward(*s, a, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "generic_pair_backward");
}

// ---- the bf16 candidate tables from the generic index (mol_coarse.hip) ----
int32_t rails_mol_generic_table_width(const rails_mol_shape* s) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return 0;
  const int w = gen_table_width(*s);
  if (w == 0) set_error("the generic route's candidate tables take dot_product_dimension <= 128 (the widest bf16 scan), got %d", s->dot_product_dimension);
  return w;
}

static int generic_table_check(const rails_mol_shape* s, const float* index, const int64_t* positions, bool update, int64_t m, void* table, int64_t n_items,
                               const char* what) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (rails_mol_generic_table_width(s) == 0) return RAILS_ENOTSUP;
  if (m < 0 || n_items < 0) { set_error("%s: negative size", what); return RAILS_EINVAL; }
  if (m > 0 && (!index || !table || (update && !positions))) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  return RAILS_OK;
}

int rails_mol_generic_coarse_build(const rails_mol_shape* s, const float* index, int64_t n_items, void* table, void* stream) {
  const int c = generic_table_check(s, index, nullptr, false, n_items, table, n_items, "generic_coarse_build");
  if (c != RAILS_OK || n_items == 0) return c;
  return fail(generic_coarse_table(*s, index, nullptr, n_items, table, n_items, (hipStream_t)stream), "generic_coarse_build");
}

int rails_mol_generic_coarse_update(const rails_mol_shape* s, const float* index, const int64_t* positions, int64_t n_new, void* table, int64_t n_items,
                                    void* stream) {
  const int c = generic_table_check(s, index, positions, true, n_new, table, n_items, "generic_coarse_update");
  if (c != RAILS_OK || n_new == 0) return c;
  return fail(generic_coarse_table(*s, index, positions, n_new, table, n_items, (hipStream_t)stream), "generic_coarse_update");
}

int rails_mol_generic_component_build(const rails_mol_shape* s, const float* index, int64_t n_items, void* table, void* stream) {
  const int c = generic_table_check(s, index, nullptr, false, n_items, table, n_items, "generic_component_build");
  if (c != RAILS_OK || n_items == 0) return c;
  return fail(generic_component_table(*s, index, nullptr, n_items, table, n_items, (hipStream_t)stream), "generic_component_build");
}

int rails_mol_generic_component_update(const rails_mol_shape* s, const float* index, const int64_t* positions, int64_t n_new, void* table, int64_t n_items,
                                       void* stream) {
  const int c = generic_table_check(s, index, positions, true, n_new, table, n_items, "generic_component_update");
  if (c != RAILS_OK || n_new == 0) return c;
  return fail(generic_component_table(*s, index, positions, n_new, table, n_items, (hipStream_t)stream), "generic_component_update");
}

int rails_mol_generic_eq_pad(const rails_mol_shape* s, const float* eq, int64_t rows, float* out, void* stream) {
  g_err[0] = '\0';
  if (!generic_supported(s)) return RAILS_ENOTSUP;
  if (rails_mol_generic_table_width(s) == 0) return RAILS_ENOTSUP;
  if (rows < 0) { set_error("generic_eq_pad: rows < 0"); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!eq || !out) { set_error("generic_eq_pad: NULL pointer"); return RAILS_EINVAL; }
  return fail(generic_eq_pad(*s, eq, rows, out, (hipStream_t)stream), "generic_eq_pad");
}

size_t rails_mips_index_floats(int32_t dim, int64_t n_items) {
  if (dim <= 0 || n_items < 0) return 0;
  return (size_t)num_tiles(n_items) * 32 * (size_t)((dim + 7) / 8 * 8);
}

int rails_mips_index_build(const float* items, int64_t n_items, int32_t dim, float* index, void* stream) {
  g_err[0] = '\0';
  if (dim <= 0 || n_items < 0) { set_error("mips_index_build: bad size"); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!items || !index) { set_error("mips_index_build: NULL pointer"); return RAILS_EINVAL; }
  return fail(mips_pack_items(items, n_items, dim, index, (hipStream_t)stream), "mips_index_build");
}

int rails_mips_index_update(const float* items, int64_t n_new, int32_t dim, const int64_t* positions, float* index, int64_t n_items, void* stream) {
  g_err[0] = '\0';
  if (dim <= 0 || n_new < 0 || n_items < 0) { set_error("mips_index_update: bad size"); return RAILS_EINVAL; }
  if (n_new == 0) return RAILS_OK;
  if (!items || !positions || !index) { set_error("mips_index_update: NULL pointer"); return RAILS_EINVAL; }
  return fail(mips_update_items(items, n_new, dim, positions, index, n_items, (hipStream_t)stream), "mips_index_update");
}

int rails_mips_index_gather_rows(const float* index, int64_t n_items, int32_t dim, const int64_t* positions, int64_t n_rows, float* rows, void* stream) {
  g_err[0] = '\0';
  if (dim <= 0 || n_rows < 0 || n_items < 0) { set_error("mips_index_gather_rows: bad size"); return RAILS_EINVAL; }
  if (n_rows == 0) return RAILS_OK;
  if (!index || !positions || !rows) { set_error("mips_index_gather_rows: NULL pointer"); return RAILS_EINVAL; }
  return fail(mips_gather_rows(index, n_items, dim, positions, n_rows, rows, (hipStream_t)stream), "mips_index_gather_rows");
}

int rails_mips_index_clear_tail(float* index, int64_t n_items, int32_t dim, void* stream) {
  g_err[0] = '\0';
  if (dim <= 0 || n_items < 0) { set_error("mips_index_clear_tail: bad size"); return RAILS_EINVAL; }
  if (n_items % 32 == 0) return RAILS_OK;
  if (!index) { set_error("mips_index_clear_tail: NULL pointer"); return RAILS_EINVAL; }
  return fail(tile_clear_tail(index, n_items, 32 * (int64_t)((dim + 7) / 8 * 8), (hipStream_t)stream), "mips_index_clear_tail");
}

size_t rails_mips_query_ws_floats(int32_t dim, int32_t batch) {
  if (dim <= 0 || batch < 0) return 0;
  return (size_t)((batch + 31) / 32) * 32 * (size_t)((dim + 7) / 8 * 8);
}

int rails_mips_score_indexed(const float* queries, int32_t batch, int32_t dim, const float* index, int64_t n_items, const int64_t* positions,
                             int64_t n_cand, float* query_ws, float* logits, int64_t ld, void* stream) {
  g_err[0] = '\0';
  if (dim <= 0 || batch < 0 || n_items <= 0 || n_cand < 0) { set_error("mips_score_indexed: bad size"); return RAILS_EINVAL; }
  if (batch == 0 || n_cand == 0) return RAILS_OK;
  if (!queries || !index || !positions || !query_ws || !logits) { set_error("mips_score_indexed: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("mips_score_indexed: ld < n_cand"); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("mips_score_indexed: no HIP device"); return RAILS_ELAUNCH; }
  return fail(mips_score_indexed(queries, batch, dim, index, n_items, positions, n_cand, query_ws, logits, ld, cu, (hipStream_t)stream),
              "mips_score_indexed");
}

int rails_mips_score(const float* queries, int32_t batch, int32_t dim, const float* index, int64_t n_items, float* query_ws,
                     float* logits, int64_t ld, void* stream) {
  g_err[0] = '\0';
  if (dim <= 0 || batch < 0 || n_items < 0) { set_error("mips_score: bad size"); return RAILS_EINVAL; }
  if (batch == 0 || n_items == 0) return RAILS_OK;
  if (!queries || !index || !query_ws || !logits) { set_error("mips_score: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_items) { set_error("mips_score: ld < n_items"); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("mips_score: no HIP device"); return RAILS_ELAUNCH; }
  return fail(mips_score(queries, batch, dim, index, n_items, query_ws, logits, ld, cu, (hipStream_t)stream), "mips_score");
}

int rails_dot_rowwise(const float* queries, const float* items, int64_t n_queries, int32_t n_cand, int32_t dim, int32_t r,
                      float* out, void* stream) {
  g_err[0] = '\0';
  if (n_queries < 0 || n_cand < 0 || dim <= 0 || r <= 0 || n_queries % r != 0) { set_error("dot_rowwise: bad size"); return RAILS_EINVAL; }
  if (n_queries == 0 || n_cand == 0) return RAILS_OK;
  if (!queries || !items || !out) { set_error("dot_rowwise: NULL pointer"); return RAILS_EINVAL; }
  return fail(dot_rowwise(queries, items, n_queries, n_cand, dim, r, out, (hipStream_t)stream), "dot_rowwise");
}

// ---- item id -> position map (id_map.hip) ----
static bool id_map_slots_ok(int64_t slots) { return slots >= 1 && slots <= (1LL << 33) && (slots & (slots - 1)) == 0; }

// the checks the four entry points share, before any launch: 1 = launch, 0 = nothing to do, < 0 = the error code
static int id_map_args(const char* what, bool pointers, int64_t slots, int64_t m, int64_t first = 0) {
  g_err[0] = '\0';
  if (!id_map_slots_ok(slots)) { set_error("%s: slots = %lld is not a power of two in [1, 2^33]", what, (long long)slots); return RAILS_EINVAL; }
  if (m < 0 || first < 0 || first > (1LL << 31) || m > (1LL << 31) - first) {
    set_error("%s: m = %lld ids from position %lld: sizes must be >= 0 and positions below 2^31", what, (long long)m, (long long)first);
    return RAILS_EINVAL;
  }
  if (m == 0) return 0;
  if (!pointers) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  return 1;
}

int64_t rails_id_map_slots(int64_t n_items) {
  g_err[0] = '\0';
  if (n_items < 0 || n_items >= (1LL << 31)) { set_error("id_map_slots: n_items = %lld outside [0, 2^31)", (long long)n_items); return RAILS_EINVAL; }
  int64_t slots = 4;
  while (slots < 4 * n_items) slots <<= 1;
  return slots;
}

size_t rails_id_map_bytes(int64_t slots) { return id_map_slots_ok(slots) ? (size_t)slots * 12 : 0; }

int rails_id_map_clear(void* map, int64_t slots, void* stream) {
  const int go = id_map_args("id_map_clear", map != nullptr, slots, 1);
  return go <= 0 ? go : fail(id_map_clear(map, slots, (hipStream_t)stream), "id_map_clear");
}

int rails_id_map_insert(void* map, int64_t slots, const int64_t* ids, const int64_t* positions, int64_t first, int64_t m, int32_t* flags, void* stream) {
  const int go = id_map_args("id_map_insert", map && ids && flags, slots, m, positions ? 0 : first);
  return go <= 0 ? go : fail(id_map_insert(map, slots, ids, positions, first, m, flags, (hipStream_t)stream), "id_map_insert");
}

int rails_id_map_erase(void* map, int64_t slots, const int64_t* ids, int64_t m, int32_t* missing, void* stream) {
  const int go = id_map_args("id_map_erase", map && ids && missing, slots, m);
  return go <= 0 ? go : fail(id_map_erase(map, slots, ids, m, missing, (hipStream_t)stream), "id_map_erase");
}

int rails_id_map_lookup(const void* map, int64_t slots, const int64_t* ids, int64_t m, int64_t* positions_out, void* stream) {
  const int go = id_map_args("id_map_lookup", map && ids && positions_out, slots, m);
  return go <= 0 ? go : fail(id_map_lookup(map, slots, ids, m, positions_out, (hipStream_t)stream), "id_map_lookup");
}

// ---- item masks (item_mask.hip) ----
// the checks the entry points share, before any launch: 1 = launch, < 0 = the error code
static int item_mask_args(const char* what, bool pointers, int64_t rows, int64_t n) {
  g_err[0] = '\0';
  if (rows < 1 || rows > (1 << 24) || n < 1 || n >= (1LL << 31)) {
    set_error("%s: rows = %lld, n = %lld: rows must lie in [1, 2^24] and n in [1, 2^31)", what, (long long)rows, (long long)n);
    return RAILS_EINVAL;
  }
  if (!pointers) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  return 1;
}

int64_t rails_item_mask_words(int64_t n) { return n < 0 ? 0 : item_mask_words(n); }

int64_t rails_item_mask_tile_items(void) { return item_mask_tile_bits(); }

int rails_item_mask_pack(const uint8_t* mask, int64_t ld, int32_t rows, int64_t n, uint32_t* words, int32_t* counts, void* stream) {
  const int go = item_mask_args("item_mask_pack", mask && words && counts, rows, n);
  if (go <= 0) return go;
  if (ld < n) { set_error("item_mask_pack: ld = %lld < n = %lld", (long long)ld, (long long)n); return RAILS_EINVAL; }
  return fail(item_mask_pack(mask, ld, rows, n, words, counts, (hipStream_t)stream), "item_mask_pack");
}

int rails_item_mask_set(const int64_t* positions, int64_t m, int64_t n, uint32_t* words, void* stream) {
  const int go = item_mask_args("item_mask_set", words && (positions || m == 0), 1, n);
  if (go <= 0) return go;
  if (m < 0) { set_error("item_mask_set: m < 0"); return RAILS_EINVAL; }
  if (m == 0) return RAILS_OK;
  return fail(item_mask_set(positions, m, n, words, (hipStream_t)stream), "item_mask_set");
}

int rails_item_mask_clear(const int64_t* positions, int64_t m, int64_t n, uint32_t* words, void* stream) {
  const int go = item_mask_args("item_mask_clear", words && (positions || m == 0), 1, n);
  if (go <= 0) return go;
  if (m < 0) { set_error("item_mask_clear: m < 0"); return RAILS_EINVAL; }
  if (m == 0) return RAILS_OK;
  return fail(item_mask_clear(positions, m, n, words, (hipStream_t)stream), "item_mask_clear");
}

int rails_item_mask_count(const uint32_t* words, int32_t rows, int64_t n, int32_t* counts, void* stream) {
  const int go = item_mask_args("item_mask_count", words && counts, rows, n);
  return go <= 0 ? go : fail(item_mask_count(words, rows, n, counts, (hipStream_t)stream), "item_mask_count");
}

size_t rails_item_mask_positions_workspace_bytes(int32_t rows, int64_t n) {
  return rows < 1 || n < 1 || n >= (1LL << 31) ? 0 : item_mask_positions_workspace_bytes(rows, n);
}

int rails_item_mask_positions(const uint32_t* words, int32_t rows, int64_t n, int64_t* out, int64_t out_ld, void* workspace, size_t workspace_bytes,
                              void* stream) {
  const int go = item_mask_args("item_mask_positions", words && workspace && (out || out_ld == 0), rows, n);
  if (go <= 0) return go;
  if (out_ld < 0) { set_error("item_mask_positions: out_ld < 0"); return RAILS_EINVAL; }
  if (workspace_bytes < item_mask_positions_workspace_bytes(rows, n)) { set_error("item_mask_positions: workspace too small"); return RAILS_ENOMEM; }
  return fail(item_mask_positions(words, rows, n, out, out_ld, workspace, (hipStream_t)stream), "item_mask_positions");
}

int rails_scores_mask(float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const uint32_t* words, int64_t words_row_stride, float fill,
                      const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0 || ld < n || first_item < 0 || words_row_stride < 0 || first_item + n >= (1LL << 31)) {
    set_error("scores_mask: bad size (rows = %d, n = %lld, ld = %lld, first_item = %lld)", rows, (long long)n, (long long)ld, (long long)first_item);
    return RAILS_EINVAL;
  }
  if (rows == 0 || n == 0) return RAILS_OK;
  if (!scores || !words) { set_error("scores_mask: NULL pointer"); return RAILS_EINVAL; }
  if (words_row_stride != 0 && words_row_stride < item_mask_words(first_item + n)) { set_error("scores_mask: the mask rows are shorter than first_item + n bits"); return RAILS_EINVAL; }
  return fail(scores_mask(scores, ld, rows, n, first_item, words, words_row_stride, fill, run_if, (hipStream_t)stream), "scores_mask");
}

int rails_item_tags_effective(const uint32_t* tags, const uint32_t* visible_words, int64_t n, uint32_t* eff_out, void* stream) {
  const int go = item_mask_args("item_tags_effective", tags && visible_words && eff_out, 1, n);
  return go <= 0 ? go : fail(item_tags_effective(tags, visible_words, n, eff_out, (hipStream_t)stream), "item_tags_effective");
}

int rails_item_tags_count(const uint32_t* eff_tags, int64_t n, const uint32_t* words, int32_t n_words, int32_t* counts_out, void* stream) {
  g_err[0] = '\0';
  if (n_words == 0) return RAILS_OK;
  if (n_words < 0 || n_words > (1 << 16)) { set_error("item_tags_count: n_words = %d outside [0, 65536]", n_words); return RAILS_EINVAL; }
  const int go = item_mask_args("item_tags_count", eff_tags && words && counts_out, 1, n);
  return go <= 0 ? go : fail(item_tags_count(eff_tags, n, words, n_words, counts_out, (hipStream_t)stream), "item_tags_count");
}

int rails_item_mask_from_tags(const uint32_t* eff_tags, int64_t n, const uint32_t* allowed, int32_t rows, uint32_t* words_out, int32_t* counts_out,
                              void* stream) {
  const int go = item_mask_args("item_mask_from_tags", eff_tags && allowed && words_out && counts_out, rows, n);
  return go <= 0 ? go : fail(item_mask_from_tags(eff_tags, n, allowed, rows, words_out, counts_out, (hipStream_t)stream), "item_mask_from_tags");
}

int rails_scores_at_eligible(float* scores, int64_t ld, int32_t rows, int64_t t, const int64_t* positions, int64_t n, const uint32_t* words,
                             int64_t words_row_stride, const uint32_t* eff_tags, const uint32_t* allowed, const int64_t* invalid_ids, int32_t width,
                             const int64_t* item_ids, float* extra_a, float* extra_b, int32_t extra_len, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || t < 0 || n < 1 || ld < t || width < 0 || extra_len < 0 || words_row_stride < 0) {
    set_error("scores_at_eligible: bad size (rows = %d, t = %lld, n = %lld, ld = %lld)", rows, (long long)t, (long long)n, (long long)ld);
    return RAILS_EINVAL;
  }
  if (rows == 0 || t == 0) return RAILS_OK;
  if (!scores || !positions) { set_error("scores_at_eligible: NULL pointer"); return RAILS_EINVAL; }
  if ((eff_tags == nullptr) != (allowed == nullptr)) { set_error("scores_at_eligible: eff_tags and allowed go together"); return RAILS_EINVAL; }
  if (words && words_row_stride != 0 && words_row_stride < item_mask_words(n)) { set_error("scores_at_eligible: the mask rows are shorter than n bits"); return RAILS_EINVAL; }
  if (width == 0) invalid_ids = nullptr;
  if (invalid_ids && !item_ids) { set_error("scores_at_eligible: invalid_ids without item_ids"); return RAILS_EINVAL; }
  if ((extra_a == nullptr) != (extra_b == nullptr)) { set_error("scores_at_eligible: the two extra arrays go together"); return RAILS_EINVAL; }
  return fail(scores_at_eligible(scores, ld, rows, t, positions, n, words, words_row_stride, eff_tags, allowed, invalid_ids, width, item_ids, extra_a, extra_b,
                                 extra_len, (hipStream_t)stream), "scores_at_eligible");
}

int rails_scores_mask_tags(float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const uint32_t* eff_tags, const uint32_t* allowed,
                           int32_t rows_per_allowed, float fill, const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0 || ld < n || first_item < 0 || first_item + n >= (1LL << 31)) {
    set_error("scores_mask_tags: bad size (rows = %d, n = %lld, ld = %lld, first_item = %lld)", rows, (long long)n, (long long)ld, (long long)first_item);
    return RAILS_EINVAL;
  }
  if (rows == 0 || n == 0) return RAILS_OK;
  if (!scores || !eff_tags || !allowed) { set_error("scores_mask_tags: NULL pointer"); return RAILS_EINVAL; }
  if (rows_per_allowed < 1) { set_error("scores_mask_tags: rows_per_allowed = %d < 1", rows_per_allowed); return RAILS_EINVAL; }
  return fail(scores_mask_tags(scores, ld, rows, n, first_item, eff_tags, allowed, rows_per_allowed, fill, run_if, (hipStream_t)stream), "scores_mask_tags");
}

// ---- exact ranks of given items (rank.hip) ----
static int rank_args(const char* what, bool pointers, int64_t rows, int64_t n, int64_t ld, int64_t t) {
  const int go = item_mask_args(what, pointers, rows, n);
  if (go <= 0) return go;
  if (ld < n) { set_error("%s: ld = %lld < n = %lld", what, (long long)ld, (long long)n); return RAILS_EINVAL; }
  if (t < 1 || t > 64) { set_error("%s: t = %lld targets per row outside [1, 64]", what, (long long)t); return RAILS_EINVAL; }
  return 1;
}

int rails_scores_rank_keys(const float* scores, int64_t ld, int32_t rows, int64_t n, const int64_t* positions, int32_t t, uint64_t* keys_out, void* stream) {
  g_err[0] = '\0';
  if (rows == 0) return RAILS_OK;
  const int go = rank_args("scores_rank_keys", scores && positions && keys_out, rows, n, ld, t);
  return go <= 0 ? go : fail(scores_rank_keys(scores, ld, rows, n, positions, t, keys_out, (hipStream_t)stream), "scores_rank_keys");
}

int rails_scores_rank(const float* scores, int64_t ld, int32_t rows, int64_t n, const uint64_t* keys, int32_t t, const uint32_t* mask_words,
                      int64_t words_row_stride, int32_t* ranks_out, void* stream) {
  g_err[0] = '\0';
  if (rows == 0) return RAILS_OK;
  const int go = rank_args("scores_rank", scores && keys && ranks_out, rows, n, ld, t);
  if (go <= 0) return go;
  if (words_row_stride != 0 && words_row_stride < item_mask_words(n)) { set_error("scores_rank: the mask rows are shorter than n bits"); return RAILS_EINVAL; }
  return fail(scores_rank(scores, ld, rows, n, keys, t, mask_words, words_row_stride, ranks_out, (hipStream_t)stream), "scores_rank");
}

int rails_item_mask_clear_rows(const int64_t* positions, int32_t rows, int64_t m, int64_t n, uint32_t* words, int64_t words_row_stride, void* stream) {
  g_err[0] = '\0';
  if (m < 0) { set_error("item_mask_clear_rows: m < 0"); return RAILS_EINVAL; }
  if (rows == 0 || m == 0) return RAILS_OK;
  const int go = item_mask_args("item_mask_clear_rows", positions && words, rows, n);
  if (go <= 0) return go;
  if (words_row_stride < item_mask_words(n)) { set_error("item_mask_clear_rows: the mask rows are shorter than n bits"); return RAILS_EINVAL; }
  return fail(item_mask_clear_rows(positions, rows, m, n, words, words_row_stride, (hipStream_t)stream), "item_mask_clear_rows");
}

// ---- softmax over the corpus (softmax.hip) ----
static int softmax_args(const char* what, bool pointers, int64_t rows, int64_t n, int64_t ld, float inv_temperature, int64_t words_row_stride) {
  const int go = item_mask_args(what, pointers, rows, n);
  if (go <= 0) return go;
  if (ld < n) { set_error("%s: ld = %lld < n = %lld", what, (long long)ld, (long long)n); return RAILS_EINVAL; }
  if (!(inv_temperature > 0.0f && inv_temperature <= 3.402823466e+38f)) { set_error("%s: inv_temperature = %g is not a finite number > 0", what, (double)inv_temperature); return RAILS_EINVAL; }
  if (words_row_stride != 0 && words_row_stride < item_mask_words(n)) { set_error("%s: the mask rows are shorter than n bits", what); return RAILS_EINVAL; }
  return 1;
}

size_t rails_scores_lse_workspace_bytes(int32_t rows, int64_t n) {
  return rows > 0 && rows <= (1 << 24) && n > 0 && n < (1LL << 31) ? scores_lse_workspace_bytes(rows, n) : 0;
}

int rails_scores_lse(const float* scores, int64_t ld, int32_t rows, int64_t n, float inv_temperature, const uint32_t* mask_words, int64_t words_row_stride,
                     void* workspace, size_t workspace_bytes, float* lse_out, void* stream) {
  g_err[0] = '\0';
  if (rows == 0) return RAILS_OK;
  const int go = softmax_args("scores_lse", scores && workspace && lse_out, rows, n, ld, inv_temperature, words_row_stride);
  if (go <= 0) return go;
  if (workspace_bytes < scores_lse_workspace_bytes(rows, n)) { set_error("scores_lse: workspace too small"); return RAILS_ENOMEM; }
  return fail(scores_lse(scores, ld, rows, n, inv_temperature, mask_words, words_row_stride, workspace, lse_out, (hipStream_t)stream), "scores_lse");
}

int rails_scores_log_prob(const float* scores, int64_t ld, int32_t rows, int64_t n, const int64_t* positions, int64_t t, float inv_temperature, const float* lse,
                          const uint32_t* mask_words, int64_t words_row_stride, float* out, void* stream) {
  g_err[0] = '\0';
  if (rows == 0) return RAILS_OK;
  const int go = softmax_args("scores_log_prob", scores && positions && lse && out, rows, n, ld, inv_temperature, words_row_stride);
  if (go <= 0) return go;
  if (t < 1) { set_error("scores_log_prob: t = %lld targets per row < 1", (long long)t); return RAILS_EINVAL; }
  return fail(scores_log_prob(scores, ld, rows, n, positions, t, inv_temperature, lse, mask_words, words_row_stride, out, (hipStream_t)stream), "scores_log_prob");
}

int rails_scores_gumbel(const float* scores, int64_t ld, int32_t rows, int64_t n, float inv_temperature, uint64_t seed, int64_t first_row,
                        const uint32_t* mask_words, int64_t words_row_stride, float* out, int64_t out_ld, void* stream) {
  g_err[0] = '\0';
  if (rows == 0) return RAILS_OK;
  const int go = softmax_args("scores_gumbel", scores && out, rows, n, ld, inv_temperature, words_row_stride);
  if (go <= 0) return go;
  if (out_ld < n) { set_error("scores_gumbel: out_ld = %lld < n = %lld", (long long)out_ld, (long long)n); return RAILS_EINVAL; }
  if (first_row < 0) { set_error("scores_gumbel: first_row < 0"); return RAILS_EINVAL; }
  return fail(scores_gumbel(scores, ld, rows, n, inv_temperature, seed, first_row, mask_words, words_row_stride, out, out_ld, (hipStream_t)stream), "scores_gumbel");
}

// ---- range search over a score matrix (range.hip) ----
size_t rails_scores_range_workspace_bytes(int32_t rows, int64_t n) {
  return rows > 0 && rows <= (1 << 24) && n > 0 && n < (1LL << 31) ? scores_range_workspace_bytes(rows, n) : 0;
}

int rails_scores_range_count(const float* scores, int64_t ld, int32_t rows, int64_t n, const float* thresholds, float inv_temperature, const float* lse,
                             const uint32_t* mask_words, int64_t words_row_stride, void* workspace, size_t workspace_bytes, int64_t* counts_out,
                             int64_t* lims_out, void* stream) {
  g_err[0] = '\0';
  if (rows == 0) return RAILS_OK;
  const int go = softmax_args("scores_range_count", scores && thresholds && workspace && counts_out && lims_out, rows, n, ld, inv_temperature, words_row_stride);
  if (go <= 0) return go;
  if (workspace_bytes < scores_range_workspace_bytes(rows, n)) { set_error("scores_range_count: workspace too small"); return RAILS_ENOMEM; }
  return fail(scores_range_count(scores, ld, rows, n, thresholds, inv_temperature, lse, mask_words, words_row_stride, workspace, counts_out, lims_out,
                                 (hipStream_t)stream), "scores_range_count");
}

int rails_scores_range_write(const float* scores, int64_t ld, int32_t rows, int64_t n, const float* thresholds, float inv_temperature, const float* lse,
                             const uint32_t* mask_words, int64_t words_row_stride, void* workspace, size_t workspace_bytes, uint64_t* keys_out,
                             int64_t capacity, void* stream) {
  g_err[0] = '\0';
  if (capacity < 0) { set_error("scores_range_write: capacity < 0"); return RAILS_EINVAL; }
  if (rows == 0 || capacity == 0) return RAILS_OK;
  const int go = softmax_args("scores_range_write", scores && thresholds && workspace && keys_out, rows, n, ld, inv_temperature, words_row_stride);
  if (go <= 0) return go;
  if (workspace_bytes < scores_range_workspace_bytes(rows, n)) { set_error("scores_range_write: workspace too small"); return RAILS_ENOMEM; }
  return fail(scores_range_write(scores, ld, rows, n, thresholds, inv_temperature, lse, mask_words, words_row_stride, workspace, keys_out, capacity,
                                 (hipStream_t)stream), "scores_range_write");
}

int rails_scores_range_sort(uint64_t* keys, const int64_t* lims, int32_t rows, int32_t max_count, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || rows > (1 << 24) || max_count < 0) { set_error("scores_range_sort: rows = %d, max_count = %d", rows, max_count); return RAILS_EINVAL; }
  if (max_count > kRangeSortMax) { set_error("scores_range_sort: max_count = %d beyond the %d keys one workgroup sorts", max_count, kRangeSortMax); return RAILS_ENOTSUP; }
  if (rows == 0 || max_count < 2) return RAILS_OK;
  if (!keys || !lims) { set_error("scores_range_sort: NULL pointer"); return RAILS_EINVAL; }
  return fail(scores_range_sort(keys, lims, rows, max_count, (hipStream_t)stream), "scores_range_sort");
}

int rails_scores_range_decode(const uint64_t* keys, int64_t total, const int64_t* ids, int64_t n, float* scores_out, int64_t* ids_out, void* stream) {
  g_err[0] = '\0';
  if (total < 0 || n < 1 || n >= (1LL << 31)) { set_error("scores_range_decode: total = %lld, n = %lld", (long long)total, (long long)n); return RAILS_EINVAL; }
  if (total == 0) return RAILS_OK;
  if (!keys || !scores_out || !ids_out) { set_error("scores_range_decode: NULL pointer"); return RAILS_EINVAL; }
  return fail(scores_range_decode(keys, total, ids, n, scores_out, ids_out, (hipStream_t)stream), "scores_range_decode");
}

// ---- query fusion (fuse.hip) ----
int rails_scores_fuse_rows(const float* scores, int64_t ld, int32_t rows_in, int64_t n, const int64_t* lims, int32_t n_out, int32_t mode, const float* weights,
                           float* out, int64_t ld_out, const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (rows_in < 0 || rows_in > (1 << 24) || n_out < 0 || n_out > (1 << 24) || n < 1 || n >= (1LL << 31) || ld < n || ld_out < n) {
    set_error("scores_fuse_rows: bad size (rows_in = %d, n_out = %d, n = %lld, ld = %lld, ld_out = %lld)", rows_in, n_out, (long long)n, (long long)ld,
              (long long)ld_out);
    return RAILS_EINVAL;
  }
  if (mode != RAILS_FUSE_MAX && mode != RAILS_FUSE_SUM) { set_error("scores_fuse_rows: mode = %d is neither RAILS_FUSE_MAX nor RAILS_FUSE_SUM", mode); return RAILS_EINVAL; }
  if (weights && mode == RAILS_FUSE_MAX) { set_error("scores_fuse_rows: weights go with RAILS_FUSE_SUM"); return RAILS_EINVAL; }
  if (n_out == 0) return RAILS_OK;
  if (!lims || !out || (rows_in > 0 && !scores)) { set_error("scores_fuse_rows: NULL pointer"); return RAILS_EINVAL; }
  if (rows_in > 0) {      // the elements either matrix spans, first to last
    const float* s_end = scores + ((int64_t)(rows_in - 1) * ld + n);
    const float* o_end = out + ((int64_t)(n_out - 1) * ld_out + n);
    if (scores < o_end && out < s_end) { set_error("scores_fuse_rows: out overlaps scores"); return RAILS_EINVAL; }
  }
  return fail(scores_fuse_rows(scores, ld, rows_in, n, lims, n_out, mode, weights, out, ld_out, run_if, (hipStream_t)stream), "scores_fuse_rows");
}

int rails_topk_fuse_lists(const float* scores, int64_t ld, const int64_t* positions, int32_t rows_in, int32_t depth, const int64_t* lims, int32_t n_out,
                          int32_t max_segment, int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids,
                          float* out_scores, void* stream) {
  g_err[0] = '\0';
  if (rows_in < 0 || depth < 1 || n_out < 0 || max_segment < 1 || n_items < 0 || width < 0 || k < 0 || ld < depth) {
    set_error("topk_fuse_lists: bad size (rows_in = %d, depth = %d, n_out = %d, max_segment = %d, n_items = %lld, width = %d, k = %d, ld = %lld)", rows_in, depth,
              n_out, max_segment, (long long)n_items, width, k, (long long)ld);
    return RAILS_EINVAL;
  }
  if (n_out == 0 || k == 0) return RAILS_OK;
  if (!lims || !out_ids || !out_scores || (rows_in > 0 && (!scores || !positions)) || (width > 0 && !invalid_ids)) {
    set_error("topk_fuse_lists: NULL pointer");
    return RAILS_EINVAL;
  }
  const int r = topk_fuse_lists(scores, ld, positions, rows_in, depth, lims, n_out, max_segment, n_items, ids, invalid_ids, width, k, out_ids, out_scores,
                                (hipStream_t)stream);
  return r == kOk ? r : fail(r, "topk_fuse_lists");
}

int rails_lists_union(const int64_t* positions, int64_t ld, int32_t rows_in, int32_t width, const int64_t* lims, int32_t n_out, int32_t max_segment,
                      int64_t n_items, int64_t* out, int32_t w_out, int32_t* counts, void* stream) {
  g_err[0] = '\0';
  if (rows_in < 0 || width < 1 || n_out < 0 || max_segment < 1 || n_items < 0 || ld < width || w_out < 1) {
    set_error("lists_union: bad size (rows_in = %d, width = %d, n_out = %d, max_segment = %d, n_items = %lld, ld = %lld, w_out = %d)", rows_in, width, n_out,
              max_segment, (long long)n_items, (long long)ld, w_out);
    return RAILS_EINVAL;
  }
  if (n_out == 0) return RAILS_OK;
  if (!lims || !out || (rows_in > 0 && !positions)) { set_error("lists_union: NULL pointer"); return RAILS_EINVAL; }
  return fail(lists_union(positions, ld, width, rows_in, lims, n_out, max_segment, n_items, out, w_out, counts, (hipStream_t)stream), "lists_union");
}

size_t rails_mol_coarse_table_bytes(const rails_mol_shape* s, int64_t n_items) {
  if (!shape_ok(s) || n_items < 0) return 0;
  return (size_t)n_items * (size_t)s->dot_product_dimension * 2;
}

int rails_mol_coarse_build(const rails_mol_shape* s, const float* index, int64_t n_items, void* table, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (s->dot_product_dimension % 8 != 0) { set_error("coarse_build: d must be a multiple of 8"); return RAILS_ENOTSUP; }
  if (n_items < 0) { set_error("coarse_build: n_items < 0"); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!index || !table) { set_error("coarse_build: NULL pointer"); return RAILS_EINVAL; }
  if (is_split(*s)) { set_error("coarse_build: needs an fp32-format item index (build one with precision = RAILS_PRECISION_FP32)"); return RAILS_ENOTSUP; }
  return fail(coarse_build(*s, index, n_items, table, (hipStream_t)stream), "coarse_build");
}

size_t rails_mol_coarse_prefilter_bytes(const rails_mol_shape* s, int64_t n_items) {
  if (!shape_ok(s)) return 0;
  return coarse_prefilter_bytes(*s, n_items);
}

static int table_update_check(const rails_mol_shape* s, const float* src, const int64_t* positions, int64_t n_new, void* table, int64_t n_items,
                              const char* what) {
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (s->dot_product_dimension % 8 != 0) { set_error("%s: d must be a multiple of 8", what); return RAILS_ENOTSUP; }
  if (n_new < 0 || n_items < 0) { set_error("%s: negative size", what); return RAILS_EINVAL; }
  if (n_new > 0 && (!src || !positions || !table)) { set_error("%s: NULL pointer", what); return RAILS_EINVAL; }
  if (is_split(*s)) { set_error("%s: needs an fp32-format item index (build one with precision = RAILS_PRECISION_FP32)", what); return RAILS_ENOTSUP; }
  return RAILS_OK;
}

int rails_mol_coarse_update(const rails_mol_shape* s, const float* src_index, int32_t src_in_place, const int64_t* positions, int64_t n_new, void* table,
                            int64_t n_items, void* stream) {
  g_err[0] = '\0';
  const int c = table_update_check(s, src_index, positions, n_new, table, n_items, "coarse_update");
  if (c != RAILS_OK || n_new == 0) return c;
  return fail(coarse_update(*s, src_index, src_in_place ? 1 : 0, positions, n_new, table, n_items, (hipStream_t)stream), "coarse_update");
}

int rails_mol_component_update(const rails_mol_shape* s, const float* src_index, int32_t src_in_place, const int64_t* positions, int64_t n_new, void* table,
                               int64_t n_total, void* stream) {
  g_err[0] = '\0';
  const int c = table_update_check(s, src_index, positions, n_new, table, n_total, "component_update");
  if (c != RAILS_OK || n_new == 0) return c;
  return fail(component_update(*s, src_index, src_in_place ? 1 : 0, positions, n_new, table, n_total, (hipStream_t)stream), "component_update");
}

int rails_mol_coarse_prefilter_build(const rails_mol_shape* s, const void* table, int64_t n_items, void* prefilter, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (n_items <= 0) { set_error("coarse_prefilter_build: n_items must be positive"); return RAILS_EINVAL; }
  if (!table || !prefilter) { set_error("coarse_prefilter_build: NULL pointer"); return RAILS_EINVAL; }
  return fail(coarse_prefilter_build(*s, table, n_items, prefilter, (hipStream_t)stream), "coarse_prefilter_build");
}

size_t rails_mol_coarse_topk_workspace_bytes(const rails_mol_shape* s, int32_t batch, int64_t n_items, int32_t k_prime) {
  if (!shape_ok(s) || batch <= 0) return 0;
  return coarse_topk_workspace_bytes(*s, batch, n_items, k_prime);
}

int32_t rails_mol_coarse_topk_capacity(int32_t batch, int64_t n_items, int32_t k_prime) {
  return batch > 0 ? coarse_topk_capacity(batch, n_items, k_prime) : 0;
}

static int coarse_topk_entry(const rails_mol_shape* s, const float* eq, int32_t batch, int32_t average_queries, const void* table,
                             int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes, float* out_scores,
                             int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* prefilter,
                             const uint32_t* visible_words, const uint32_t* eff_tags, const uint32_t* allowed, void* stream);

int rails_mol_coarse_topk(const rails_mol_shape* s, const float* eq, int32_t batch, int32_t average_queries, const void* table,
                          int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes, float* out_scores,
                          int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* prefilter, void* stream) {
  return rails_mol_coarse_topk_visible(s, eq, batch, average_queries, table, n_items, k_prime, workspace, workspace_bytes, out_scores, out_positions,
                                       out_counts, out_of_range, prefilter, nullptr, stream);
}

int rails_mol_coarse_topk_visible(const rails_mol_shape* s, const float* eq, int32_t batch, int32_t average_queries, const void* table,
                                  int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes, float* out_scores,
                                  int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* prefilter,
                                  const uint32_t* visible_words, void* stream) {
  return coarse_topk_entry(s, eq, batch, average_queries, table, n_items, k_prime, workspace, workspace_bytes, out_scores, out_positions, out_counts,
                           out_of_range, prefilter, visible_words, nullptr, nullptr, stream);
}

int rails_mol_coarse_topk_tagged(const rails_mol_shape* s, const float* eq, int32_t batch, int32_t average_queries, const void* table,
                                 int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes, float* out_scores,
                                 int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* prefilter,
                                 const uint32_t* eff_tags, const uint32_t* allowed, void* stream) {
  if (eff_tags && !allowed) { g_err[0] = '\0'; set_error("coarse_topk_tagged: eff_tags without allowed"); return RAILS_EINVAL; }
  return coarse_topk_entry(s, eq, batch, average_queries, table, n_items, k_prime, workspace, workspace_bytes, out_scores, out_positions, out_counts,
                           out_of_range, prefilter, nullptr, eff_tags, eff_tags ? allowed : nullptr, stream);
}

static int coarse_topk_entry(const rails_mol_shape* s, const float* eq, int32_t batch, int32_t average_queries, const void* table,
                             int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes, float* out_scores,
                             int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* prefilter,
                             const uint32_t* visible_words, const uint32_t* eff_tags, const uint32_t* allowed, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (batch < 0 || n_items < 0 || k_prime < 0) { set_error("coarse_topk: negative size"); return RAILS_EINVAL; }
  if (k_prime > n_items) { set_error("coarse_topk: selected index k out of range (k = %d > n = %lld)", k_prime, (long long)n_items); return RAILS_EINVAL; }
  if (batch == 0 || k_prime == 0) return RAILS_OK;
  if (!eq || !table || !workspace || !out_scores || !out_positions || !out_counts) { set_error("coarse_topk: NULL pointer"); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("coarse_topk: no HIP device"); return RAILS_ELAUNCH; }
  const int r = coarse_topk(*s, eq, batch, average_queries ? 1 : 0, table, n_items, k_prime, workspace, workspace_bytes,
                            out_scores, out_positions, out_counts, out_of_range, prefilter, cu, (hipStream_t)stream, visible_words, eff_tags, allowed);
  return r == kOk ? r : fail(r, "coarse_topk");
}

int rails_mol_coarse_score(const rails_mol_shape* s, const float* eq, int32_t batch, int32_t average_queries,
                           const void* table, int64_t n_items, float* scores, int64_t ld, const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (batch < 0 || n_items < 0) { set_error("coarse_score: negative size"); return RAILS_EINVAL; }
  if (batch == 0 || n_items == 0) return RAILS_OK;
  if (!eq || !table || !scores) { set_error("coarse_score: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_items) { set_error("coarse_score: ld < n_items"); return RAILS_EINVAL; }
  const int r = coarse_score(*s, eq, batch, average_queries ? 1 : 0, table, n_items, scores, ld, (hipStream_t)stream, run_if);
  return r == kOk ? r : fail(r, "coarse_score");
}

size_t rails_mol_component_table_bytes(const rails_mol_shape* s, int64_t n_items) {
  if (!shape_ok(s) || n_items < 0) return 0;
  return (size_t)n_items * (size_t)s->item_dot_product_groups * (size_t)s->dot_product_dimension * 2;
}

int rails_mol_component_build(const rails_mol_shape* s, const float* index, int64_t n_items, void* table, int64_t n_total, int64_t first_item,
                              void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (s->dot_product_dimension % 8 != 0) { set_error("component_build: d must be a multiple of 8"); return RAILS_ENOTSUP; }
  if (n_items < 0 || first_item < 0 || first_item + n_items > n_total) { set_error("component_build: items [%lld, %lld) outside a table of %lld", (long long)first_item, (long long)(first_item + n_items), (long long)n_total); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!index || !table) { set_error("component_build: NULL pointer"); return RAILS_EINVAL; }
  if (is_split(*s)) { set_error("component_build: needs an fp32-format item index (build one with precision = RAILS_PRECISION_FP32)"); return RAILS_ENOTSUP; }
  return fail(component_build(*s, index, n_items, table, n_total, first_item, (hipStream_t)stream), "component_build");
}

size_t rails_mol_component_topk_workspace_bytes(const rails_mol_shape* s, int32_t batch, int64_t n_items, int32_t k_group) {
  if (!shape_ok(s) || batch <= 0) return 0;
  return component_topk_workspace_bytes(*s, batch, n_items, k_group);
}

int32_t rails_mol_component_topk_capacity(const rails_mol_shape* s, int32_t batch, int64_t n_items, int32_t k_group) {
  if (!shape_ok(s) || batch <= 0) return 0;
  return component_topk_capacity(*s, batch, n_items, k_group);
}

static int component_topk_entry(const rails_mol_shape* s, const float* eq, int32_t batch, const void* table, int64_t n_items,
                                int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                                int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, const uint32_t* visible_words,
                                const uint32_t* eff_tags, const uint32_t* allowed, void* stream);

int rails_mol_component_topk(const rails_mol_shape* s, const float* eq, int32_t batch, const void* table, int64_t n_items,
                             int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                             int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* stream) {
  return rails_mol_component_topk_visible(s, eq, batch, table, n_items, k_group, workspace, workspace_bytes, out_scores, out_positions, out_counts,
                                          out_of_range, nullptr, stream);
}

int rails_mol_component_topk_visible(const rails_mol_shape* s, const float* eq, int32_t batch, const void* table, int64_t n_items,
                                     int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                                     int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, const uint32_t* visible_words,
                                     void* stream) {
  return component_topk_entry(s, eq, batch, table, n_items, k_group, workspace, workspace_bytes, out_scores, out_positions, out_counts, out_of_range,
                              visible_words, nullptr, nullptr, stream);
}

int rails_mol_component_topk_tagged(const rails_mol_shape* s, const float* eq, int32_t batch, const void* table, int64_t n_items,
                                    int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                                    int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, const uint32_t* eff_tags,
                                    const uint32_t* allowed, void* stream) {
  if (eff_tags && !allowed) { g_err[0] = '\0'; set_error("component_topk_tagged: eff_tags without allowed"); return RAILS_EINVAL; }
  return component_topk_entry(s, eq, batch, table, n_items, k_group, workspace, workspace_bytes, out_scores, out_positions, out_counts, out_of_range,
                              nullptr, eff_tags, eff_tags ? allowed : nullptr, stream);
}

int32_t rails_mol_scan_plan(int32_t rows, int64_t n_items, int32_t k, int32_t comp_rows, int32_t* out4) {
  if (!out4 || rows < 1 || n_items < 1 || k < 1 || comp_rows < 0) return 0;
  return scan_plan_numbers(rows, n_items, k, comp_rows, out4);
}

static int component_topk_entry(const rails_mol_shape* s, const float* eq, int32_t batch, const void* table, int64_t n_items,
                                int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                                int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, const uint32_t* visible_words,
                                const uint32_t* eff_tags, const uint32_t* allowed, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (batch < 0 || n_items < 0 || k_group < 0) { set_error("component_topk: negative size"); return RAILS_EINVAL; }
  if (k_group > n_items) { set_error("component_topk: selected index k out of range (k = %d > n = %lld)", k_group, (long long)n_items); return RAILS_EINVAL; }
  if (batch == 0 || k_group == 0) return RAILS_OK;
  if (!eq || !table || !workspace || !out_scores || !out_positions || !out_counts) { set_error("component_topk: NULL pointer"); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("component_topk: no HIP device"); return RAILS_ELAUNCH; }
  const int r = component_topk(*s, eq, batch, table, n_items, k_group, workspace, workspace_bytes, out_scores, out_positions,
                               out_counts, out_of_range, cu, (hipStream_t)stream, visible_words, eff_tags, allowed);
  return r == kOk ? r : fail(r, "component_topk");
}

int rails_mol_component_score(const rails_mol_shape* s, const float* eq, int32_t batch, const void* table, int64_t n_items,
                              float* scores, int64_t ld, const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (batch < 0 || n_items < 0) { set_error("component_score: negative size"); return RAILS_EINVAL; }
  if (batch == 0 || n_items == 0) return RAILS_OK;
  if (!eq || !table || !scores) { set_error("component_score: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_items) { set_error("component_score: ld < n_items"); return RAILS_EINVAL; }
  const int r = component_score(*s, eq, batch, table, n_items, scores, ld, (hipStream_t)stream, run_if);
  return r == kOk ? r : fail(r, "component_score");
}

int rails_sort_rows_i64(const int64_t* in, int32_t rows, int32_t n, int64_t* out, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0) { set_error("sort_rows_i64: negative size"); return RAILS_EINVAL; }
  if (rows == 0 || n == 0) return RAILS_OK;
  if (!in || !out) { set_error("sort_rows_i64: NULL pointer"); return RAILS_EINVAL; }
  const int r = sort_rows_i64(in, rows, n, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "sort_rows_i64");
}

int rails_mask_sorted_duplicates(const int64_t* sorted_idx, float* scores, int64_t ld, int32_t rows, int32_t n, float fill,
                                 void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0) { set_error("mask_sorted_duplicates: negative size"); return RAILS_EINVAL; }
  if (rows == 0 || n == 0) return RAILS_OK;
  if (!sorted_idx || !scores) { set_error("mask_sorted_duplicates: NULL pointer"); return RAILS_EINVAL; }
  return fail(mask_sorted_duplicates(sorted_idx, scores, ld, rows, n, fill, (hipStream_t)stream), "mask_sorted_duplicates");
}

size_t rails_topk_workspace_bytes(int32_t rows, int64_t n, int32_t k) {
  if (rows <= 0 || n <= 0 || k <= 0) return 256;
  return topk_workspace_bytes(rows, n, k);
}

int rails_topk(const float* scores, int64_t ld, int32_t rows, int64_t n, int32_t k, int32_t sorted, const int64_t* ids,
               int64_t ids_row_stride, float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
               const int32_t* run_if, void* stream) {
  (void)sorted;  // the descending order returned is also a valid unsorted answer
  g_err[0] = '\0';
  if (rows < 0 || n < 0 || k < 0) { set_error("topk: negative size"); return RAILS_EINVAL; }
  if (k > n) { set_error("topk: selected index k out of range (k = %d > n = %lld)", k, (long long)n); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !out_scores || !out_ids) { set_error("topk: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n) { set_error("topk: ld < n"); return RAILS_EINVAL; }
  if (n > 16384 && !workspace) { set_error("topk: workspace is required for n > 16384"); return RAILS_ENOMEM; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("topk: no HIP device"); return RAILS_ELAUNCH; }
  const int r = topk(scores, ld, rows, n, k, ids, ids_row_stride, out_scores, out_ids, workspace, workspace_bytes, cu,
                     (hipStream_t)stream, nullptr, 0, 0, nullptr, run_if);
  return r == kOk ? r : fail(r, "topk");
}

int rails_topk_candidates(const float* scores, int64_t ld, int32_t rows, int32_t n_cand, int32_t k, const int64_t* positions,
                          const int64_t* ids, float* out_scores, int64_t* out_ids, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n_cand < 0 || k < 0) { set_error("topk_candidates: negative size"); return RAILS_EINVAL; }
  if (k > n_cand) { set_error("topk_candidates: selected index k out of range (k = %d > n = %d)", k, n_cand); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !positions || !out_scores || !out_ids) { set_error("topk_candidates: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("topk_candidates: ld < n_cand"); return RAILS_EINVAL; }
  if (n_cand > 16384) { set_error("topk_candidates: n_cand = %d exceeds 16384", n_cand); return RAILS_ENOTSUP; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("topk_candidates: no HIP device"); return RAILS_ELAUNCH; }
  const int r = topk(scores, ld, rows, n_cand, k, ids, 0, out_scores, out_ids, nullptr, 0, cu, (hipStream_t)stream, nullptr, 0, 0, nullptr,
                     nullptr, positions, n_cand);
  return r == kOk ? r : fail(r, "topk_candidates");
}

int rails_topk_candidates_filtered(const float* scores, int64_t ld, int32_t rows, int32_t n_cand, int32_t k_prime, const int64_t* positions,
                                   const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids,
                                   float* out_scores, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n_cand < 0 || k_prime < 0 || k < 0 || width < 0) { set_error("topk_candidates_filtered: negative size"); return RAILS_EINVAL; }
  if (k_prime > n_cand || k > k_prime) { set_error("topk_candidates_filtered: need k <= k' <= n_cand (k = %d, k' = %d, n = %d)", k, k_prime, n_cand); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !positions || !out_scores || !out_ids || (width > 0 && !invalid_ids)) { set_error("topk_candidates_filtered: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("topk_candidates_filtered: ld < n_cand"); return RAILS_EINVAL; }
  if (n_cand <= 1024 || n_cand > 8192 || !topk_can_fuse_filter(n_cand, k_prime, width, k)) {
    set_error("topk_candidates_filtered: unsupported size (n_cand = %d, k' = %d, width = %d, k = %d)", n_cand, k_prime, width, k);
    return RAILS_ENOTSUP;
  }
  const int cu = compute_units();
  if (cu <= 0) { set_error("topk_candidates_filtered: no HIP device"); return RAILS_ELAUNCH; }
  static const int64_t no_seen = 0;     // width 0: the filter still runs (it copies the first k), its list is never read
  const int r = topk(scores, ld, rows, n_cand, k_prime, ids, 0, out_scores, out_ids, nullptr, 0, cu, (hipStream_t)stream,
                     width > 0 ? invalid_ids : &no_seen, width, k, nullptr, nullptr, positions, n_cand);
  return r == kOk ? r : fail(r, "topk_candidates_filtered");
}

size_t rails_rerank_workspace_bytes(int32_t rows, int32_t n_cand) { return rows > 0 && n_cand > 0 ? rerank_workspace_bytes(rows, n_cand) : 0; }

int rails_rerank_topk_filtered(const float* scores, int64_t ld, int32_t rows, int32_t n_cand, int32_t k_prime, const int64_t* positions,
                               const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, void* workspace, size_t workspace_bytes,
                               int64_t* out_ids, float* out_scores, int32_t* out_of_range, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n_cand < 0 || k_prime < 0 || k < 0 || width < 0) { set_error("rerank_topk_filtered: negative size"); return RAILS_EINVAL; }
  if (k_prime > n_cand || k > k_prime) { set_error("rerank_topk_filtered: need k <= k' <= n_cand (k = %d, k' = %d, n = %d)", k, k_prime, n_cand); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !positions || !out_scores || !out_ids || !out_of_range || !workspace || (width > 0 && !invalid_ids)) { set_error("rerank_topk_filtered: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n_cand) { set_error("rerank_topk_filtered: ld < n_cand"); return RAILS_EINVAL; }
  static const int64_t no_seen = 0;
  const int r = rerank_topk_filtered(scores, ld, rows, n_cand, k_prime, positions, ids, width > 0 ? invalid_ids : &no_seen, width, k, workspace,
                                     workspace_bytes, out_ids, out_scores, out_of_range, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "rerank_topk_filtered");
}

// rails_topk_collapse and its quota form: one check list under the called entry's name; the plain walk hands max_per_group = 0 on.
static int collapse_checked(const char* name, bool quota, const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth,
                            const int32_t* group_ranks, int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k,
                            int32_t max_per_group, float* out_scores, int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || depth < 0 || k < 0 || width < 0 || n_items < 0) { set_error("%s: negative size", name); return RAILS_EINVAL; }
  if (quota && max_per_group < 1) { set_error("%s: max_per_group = %d below 1", name, max_per_group); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !positions || !group_ranks || !out_scores || !out_positions || !out_ids || !out_counts || !out_of_range || (width > 0 && !invalid_ids)) { set_error("%s: NULL pointer", name); return RAILS_EINVAL; }
  if (ld < depth) { set_error("%s: ld < depth", name); return RAILS_EINVAL; }
  return fail(topk_collapse(scores, ld, positions, rows, depth, group_ranks, n_items, ids, invalid_ids, width, k, max_per_group, out_scores, out_positions,
                            out_ids, out_counts, out_of_range, (hipStream_t)stream), name);
}

int rails_topk_collapse(const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth, const int32_t* group_ranks,
                        int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, float* out_scores,
                        int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, void* stream) {
  return collapse_checked("topk_collapse", false, scores, ld, positions, rows, depth, group_ranks, n_items, ids, invalid_ids, width, k, 0, out_scores,
                          out_positions, out_ids, out_counts, out_of_range, stream);
}

int rails_topk_collapse_quota(const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth, const int32_t* group_ranks,
                              int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, int32_t max_per_group,
                              float* out_scores, int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, void* stream) {
  return collapse_checked("topk_collapse_quota", true, scores, ld, positions, rows, depth, group_ranks, n_items, ids, invalid_ids, width, k,
                          max_per_group, out_scores, out_positions, out_ids, out_counts, out_of_range, stream);
}

// rails_topk_mmr: the arguments and every limit before anything else, so a refused call never launches (and needs no device).
size_t rails_topk_mmr_workspace_bytes(int32_t rows, int32_t pool, int32_t dim) {
  return rows > 0 && pool > 0 && dim > 0 ? mmr_workspace_bytes(rows, pool, dim) : 0;
}

int rails_topk_mmr(const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth, const float* vectors, int64_t n_items,
                   int32_t dim, float lam, int32_t k, int32_t pool, const int64_t* ids, const int64_t* invalid_ids, int32_t width, void* workspace,
                   size_t workspace_bytes, float* out_scores, int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range,
                   void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || depth < 0 || k < 0 || pool < 0 || width < 0 || n_items < 0) { set_error("topk_mmr: negative size"); return RAILS_EINVAL; }
  if (!(lam > 0.0f && lam <= 1.0f)) { set_error("topk_mmr: lam = %g outside (0, 1]", (double)lam); return RAILS_EINVAL; }
  if (k > pool) { set_error("topk_mmr: k = %d beyond pool = %d", k, pool); return RAILS_EINVAL; }
  if (dim < 1) { set_error("topk_mmr: dim = %d below 1", dim); return RAILS_EINVAL; }
  if (pool > 1024) { set_error("topk_mmr: pool = %d beyond 1024", pool); return RAILS_ENOTSUP; }
  if (dim > 256) { set_error("topk_mmr: dim = %d beyond 256", dim); return RAILS_ENOTSUP; }
  if (width > 4096) { set_error("topk_mmr: width = %d beyond 4096 seen ids per row", width); return RAILS_ENOTSUP; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !positions || !vectors || !out_scores || !out_positions || !out_ids || !out_counts || !out_of_range || (width > 0 && !invalid_ids)) {
    set_error("topk_mmr: NULL pointer");
    return RAILS_EINVAL;
  }
  if (ld < depth) { set_error("topk_mmr: ld < depth"); return RAILS_EINVAL; }
  return fail(topk_mmr(scores, ld, positions, rows, depth, vectors, n_items, dim, lam, k, pool, ids, invalid_ids, width, workspace, workspace_bytes,
                       out_scores, out_positions, out_ids, out_counts, out_of_range, (hipStream_t)stream), "topk_mmr");
}

// rails_scores_group_max and rails_scores_group_next: one check list under the called entry's name.  rounds: the next entry, whose empty pass
// (n == 0) is nothing to do; the max entry's may still clear its table, and its strides and bound (n_groups, none) pass the round's checks.
static int group_table_checked(const char* name, bool rounds, const float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item,
                               const int32_t* group_ranks, int64_t n_groups, uint64_t* table, int64_t table_stride, const uint64_t* below,
                               int64_t below_stride, int32_t clear_table, const int64_t* ids, const int64_t* invalid_ids, int32_t width, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0 || first_item < 0 || n_groups < 0 || width < 0) { set_error("%s: negative size", name); return RAILS_EINVAL; }
  if (rows == 0 || n_groups == 0 || (rounds && n == 0)) return RAILS_OK;
  if (!table || (n > 0 && (!scores || !group_ranks)) || (width > 0 && !invalid_ids)) { set_error("%s: NULL pointer", name); return RAILS_EINVAL; }
  if (ld < n) { set_error("%s: ld < n", name); return RAILS_EINVAL; }
  if (table_stride < n_groups || (below && below_stride < n_groups)) { set_error("%s: a row stride below n_groups", name); return RAILS_EINVAL; }
  if (below == table) { set_error("%s: a round cannot bound itself", name); return RAILS_EINVAL; }
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(table);
  return fail(rounds ? scores_group_next(scores, ld, rows, n, first_item, group_ranks, n_groups, keys, table_stride, reinterpret_cast<const unsigned long long*>(below),
                                         below_stride, ids, invalid_ids, width, (hipStream_t)stream)
                     : scores_group_max(scores, ld, rows, n, first_item, group_ranks, n_groups, keys, clear_table, ids, invalid_ids, width, (hipStream_t)stream), name);
}

int rails_scores_group_next(const float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const int32_t* group_ranks, int64_t n_groups,
                            uint64_t* table, int64_t table_stride, const uint64_t* below, int64_t below_stride, const int64_t* ids,
                            const int64_t* invalid_ids, int32_t width, void* stream) {
  return group_table_checked("scores_group_next", true, scores, ld, rows, n, first_item, group_ranks, n_groups, table, table_stride, below, below_stride, 0,
                             ids, invalid_ids, width, stream);
}

int rails_scores_group_max(const float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const int32_t* group_ranks, int64_t n_groups,
                           uint64_t* table, int32_t clear_table, const int64_t* ids, const int64_t* invalid_ids, int32_t width, void* stream) {
  return group_table_checked("scores_group_max", false, scores, ld, rows, n, first_item, group_ranks, n_groups, table, n_groups, nullptr, 0, clear_table,
                             ids, invalid_ids, width, stream);
}

int rails_topk_keys(const uint64_t* table, int32_t rows, int64_t n_groups, int32_t k, const int64_t* ids, float* out_scores, int64_t* out_positions,
                    int64_t* out_ids, int32_t* out_counts, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n_groups < 0 || k < 0) { set_error("topk_keys: negative size"); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!table || !out_scores || !out_positions || !out_ids || !out_counts) { set_error("topk_keys: NULL pointer"); return RAILS_EINVAL; }
  const int r = topk_keys(reinterpret_cast<const unsigned long long*>(table), rows, n_groups, k, ids, out_scores, out_positions, out_ids, out_counts,
                          (hipStream_t)stream);
  return r == kOk ? r : fail(r, "topk_keys");
}

int rails_topk_filter_fusable(int64_t n, int32_t k_prime, int32_t width, int32_t k) { return topk_can_fuse_filter(n, k_prime, width, k) ? 1 : 0; }

int rails_topk_filtered(const float* scores, int64_t ld, int32_t rows, int64_t n, int32_t k_prime, const int64_t* ids, int64_t ids_row_stride,
                        const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids, float* out_scores, void* workspace,
                        size_t workspace_bytes, const int32_t* run_if, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0 || k_prime < 0 || k < 0 || width < 0) { set_error("topk_filtered: negative size"); return RAILS_EINVAL; }
  if (k_prime > n) { set_error("topk_filtered: selected index k out of range (k' = %d > n = %lld)", k_prime, (long long)n); return RAILS_EINVAL; }
  if (k > k_prime) { set_error("topk_filtered: k = %d > k' = %d", k, k_prime); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!scores || !out_scores || !out_ids || !invalid_ids) { set_error("topk_filtered: NULL pointer"); return RAILS_EINVAL; }
  if (ld < n) { set_error("topk_filtered: ld < n"); return RAILS_EINVAL; }
  if (!topk_can_fuse_filter(n, k_prime, width, k)) { set_error("topk_filtered: sizes outside the fused path (rails_topk_filter_fusable)"); return RAILS_ENOTSUP; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("topk_filtered: no HIP device"); return RAILS_ELAUNCH; }
  const int r = topk(scores, ld, rows, n, k_prime, ids, ids_row_stride, out_scores, out_ids, workspace, workspace_bytes, cu, (hipStream_t)stream,
                     invalid_ids, width, k, nullptr, run_if);
  return r == kOk ? r : fail(r, "topk_filtered");
}

int rails_pack_candidates(const float* scores, const int64_t* ids, int32_t rows, int32_t k_local, int32_t k, int64_t* msg,
                          void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || k_local < 0 || k < 0 || k_local > k) { set_error("pack_candidates: bad size"); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!msg || (k_local > 0 && (!scores || !ids))) { set_error("pack_candidates: NULL pointer"); return RAILS_EINVAL; }
  return fail(pack_candidates(scores, ids, rows, k_local, k, msg, (hipStream_t)stream), "pack_candidates");
}

int rails_merge_candidates(const int64_t* gathered, int32_t n_ranks, int32_t rows, int32_t k, int32_t k_out, float* out_scores,
                           int64_t* out_ids, void* stream) {
  g_err[0] = '\0';
  if (n_ranks <= 0 || rows < 0 || k <= 0 || k_out < 0 || (int64_t)k_out > (int64_t)n_ranks * k) { set_error("merge_candidates: bad size"); return RAILS_EINVAL; }
  if (rows == 0 || k_out == 0) return RAILS_OK;
  if (!gathered || !out_scores || !out_ids) { set_error("merge_candidates: NULL pointer"); return RAILS_EINVAL; }
  const int r = merge_candidates(gathered, n_ranks, rows, k, k_out, out_scores, out_ids, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "merge_candidates");
}

int rails_merge_candidates_filtered(const int64_t* gathered, int32_t n_ranks, int32_t rows, int32_t k, int32_t k_prime, const int64_t* invalid_ids,
                                    int32_t width, int32_t k_out, int64_t* out_ids, float* out_scores, void* stream) {
  g_err[0] = '\0';
  if (n_ranks <= 0 || rows < 0 || k <= 0 || k_prime <= 0 || (int64_t)k_prime > (int64_t)n_ranks * k || width < 0 || k_out <= 0 || k_out > k_prime) { set_error("merge_candidates_filtered: bad size"); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!gathered || !out_scores || !out_ids || !invalid_ids) { set_error("merge_candidates_filtered: NULL pointer"); return RAILS_EINVAL; }
  const int r = merge_candidates(gathered, n_ranks, rows, k, k_prime, out_scores, out_ids, (hipStream_t)stream, invalid_ids, width, k_out);
  return r == kOk ? r : fail(r, "merge_candidates_filtered");
}

int rails_merge_candidates_verdict(const int64_t* gathered, int32_t n_ranks, int32_t rows, int32_t k, int32_t k_out, float default_eps, float safety,
                                   const float* guard_values, int32_t guard_per_row, float guard_limit, float* state, float* state_host,
                                   void* call_ws, const int64_t* invalid_ids, int32_t width, int32_t f_k, int64_t* out_ids, float* out_scores,
                                   void* stream) {
  g_err[0] = '\0';
  if (n_ranks <= 0 || rows < 0 || k <= 0 || k_out <= 0 || (int64_t)k_out > (int64_t)n_ranks * k || width < 0 || !(default_eps >= 0.0f) || !(safety >= 0.0f)) {
    set_error("merge_candidates_verdict: bad size");
    return RAILS_EINVAL;
  }
  if (rows == 0) return RAILS_OK;
  if (!gathered || !out_scores || !out_ids || !state || !call_ws || (guard_values && (guard_per_row <= 0 || !(guard_limit >= 0.0f))) ||
      (invalid_ids && (f_k <= 0 || f_k > k_out))) {
    set_error("merge_candidates_verdict: bad argument");
    return RAILS_EINVAL;
  }
  MergeVerdict v{default_eps, safety, guard_values, guard_per_row, guard_limit, state, state_host, static_cast<unsigned int*>(call_ws)};
  const int r = merge_candidates(gathered, n_ranks, rows, k, k_out, out_scores, out_ids, (hipStream_t)stream, invalid_ids, width, f_k, &v);
  return r == kOk ? r : fail(r, "merge_candidates_verdict");
}

int rails_abi_version(void) { return RAILS_ABI_VERSION; }

int rails_hash_item_table(uint64_t seed, int64_t first_item, int64_t n_items, int32_t dim, float scale, float* out, void* stream) {
  g_err[0] = '\0';
  if (first_item < 0 || n_items < 0 || dim <= 0) { set_error("hash_item_table: bad size"); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!out) { set_error("hash_item_table: NULL pointer"); return RAILS_EINVAL; }
  return fail(hash_item_table(seed, first_item, n_items, dim, scale, out, (hipStream_t)stream), "hash_item_table");
}

int rails_range_flag_i32(const int32_t* values, int32_t n, int32_t lo, int32_t hi, int32_t* flag, void* stream) {
  g_err[0] = '\0';
  if (n < 0 || (n > 0 && (!values || !flag))) { set_error("range_flag: bad argument"); return RAILS_EINVAL; }
  return fail(range_flag(values, n, lo, hi, flag, (hipStream_t)stream), "range_flag");
}

int rails_rescore_verdict(const float* row_stats, int32_t rows, float default_eps, float safety, const float* guard_values, int64_t guard_count,
                          float guard_limit, float* state, void* stream) {
  g_err[0] = '\0';
  if (rows <= 0 || !row_stats || !state || !(default_eps >= 0.0f) || !(safety >= 0.0f) || guard_count < 0 || (guard_values && !(guard_limit >= 0.0f))) {
    set_error("rescore_verdict: bad argument");
    return RAILS_EINVAL;
  }
  const int r = rescore_verdict(row_stats, rows, default_eps, safety, guard_values, guard_count, guard_limit, state, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "rescore_verdict");
}

int rails_margin_stats(const float* kth_scores, int64_t ld, int32_t col, const float* m_max, const float* err_max, int32_t rows, float* row_stats, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || col < 0 || ld <= col || (rows > 0 && (!kth_scores || !m_max || !err_max || !row_stats))) { set_error("margin_stats: bad argument"); return RAILS_EINVAL; }
  return fail(margin_stats(kth_scores, ld, col, m_max, err_max, rows, row_stats, (hipStream_t)stream), "margin_stats");
}

int rails_mfma_probe_f16(const uint16_t* a, const uint16_t* b, const float* c, float* d, int64_t n, void* stream) {
  g_err[0] = '\0';
  if (n < 0 || (n > 0 && (!a || !b || !c || !d))) { set_error("mfma_probe_f16: bad argument"); return RAILS_EINVAL; }
  return fail(mfma_probe_f16(a, b, c, d, n, (hipStream_t)stream), "mfma_probe_f16");
}

int rails_mfma_probe_f32(const float* a, const float* b, const float* c, float* d, int64_t n, void* stream) {
  g_err[0] = '\0';
  if (n < 0 || (n > 0 && (!a || !b || !c || !d))) { set_error("mfma_probe_f32: bad argument"); return RAILS_EINVAL; }
  return fail(mfma_probe_f32(a, b, c, d, n, (hipStream_t)stream), "mfma_probe_f32");
}

int rails_scalar_probe_f32(const float* x, int64_t n, float* out, void* stream) {
  g_err[0] = '\0';
  if (n < 0 || (n > 0 && (!x || !out))) { set_error("scalar_probe_f32: bad argument"); return RAILS_EINVAL; }
  return fail(scalar_probe(x, n, out, (hipStream_t)stream), "scalar_probe_f32");
}

int rails_rescore_select(const float* exact_scores, int64_t ld, const float* approx_scores, const float* approx_dense, int64_t ld_dense,
                         const int64_t* positions, const int64_t* ids, int64_t n_items, int32_t rows, int32_t n_ranked, int32_t n_cand,
                         int32_t k, float margin_eps, float check_eps, int32_t one_sided, float* out_scores, int64_t* out_ids, int32_t* row_ok,
                         float* row_stats, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n_ranked <= 0 || n_cand < n_ranked || k <= 0 || k > n_ranked || ld < n_cand) { set_error("rescore_select: bad size"); return RAILS_EINVAL; }
  if (n_items <= 0 || n_items > 0xFFFFFFFFll) { set_error("rescore_select: positions must fit 32 bits (n_items = %lld)", (long long)n_items); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!exact_scores || !approx_scores || !positions || !out_scores || !out_ids || (!row_ok && !row_stats) || (n_cand > n_ranked && (!approx_dense || ld_dense < n_items))) {
    set_error("rescore_select: NULL pointer or short stride");
    return RAILS_EINVAL;
  }
  const int r = rescore_select(exact_scores, ld, approx_scores, approx_dense, ld_dense, positions, ids, rows, n_ranked, n_cand, k, margin_eps,
                               check_eps, one_sided != 0, out_scores, out_ids, row_ok, row_stats, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "rescore_select");
}

size_t rails_candidates_workspace_bytes(int32_t rows) { return candidates_workspace_bytes(rows); }

int rails_candidates_select(const float* scores, int64_t ld, int32_t rows, int64_t n, int32_t cap, float lo, float hi, void* workspace,
                            int64_t* out_positions, float* out_approx, int64_t cand_ld, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || n < 0 || cap <= 0 || ld < n) { set_error("candidates_select: bad size"); return RAILS_EINVAL; }
  if (rows == 0 || n == 0) return RAILS_OK;
  if (!scores || !workspace || !out_positions || !out_approx) { set_error("candidates_select: NULL pointer"); return RAILS_EINVAL; }
  const int cu = compute_units();
  if (cu <= 0) { set_error("candidates_select: no HIP device"); return RAILS_ELAUNCH; }
  const int r = candidates_select(scores, ld, rows, n, cap, lo, hi, workspace, out_positions, out_approx, cand_ld, cu, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "candidates_select");
}

int rails_candidates_finish(const float* exact_scores, int64_t ld, const float* approx, const int64_t* positions, int64_t cand_ld, int32_t cap,
                            void* workspace, const int64_t* ids, int64_t n_items, int32_t rows, int32_t k, float default_eps, float safety,
                            int32_t one_sided, const float* guard_values, int32_t guard_per_row, float guard_limit, float* out_scores,
                            int64_t* out_ids, const int64_t* invalid_ids, int32_t width, int32_t f_k, int64_t* f_out_ids, float* f_out_scores,
                            float* state, float* state_host, int64_t* msg, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || cap <= 0 || k <= 0 || ld < cap || cand_ld < cap || n_items <= 0 || n_items > 0xFFFFFFFFll) { set_error("candidates_finish: bad size"); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!exact_scores || !approx || !positions || !workspace || (!msg && (!out_scores || !out_ids || !state)) || !(default_eps >= 0.0f) || !(safety >= 0.0f) ||
      (guard_values && (guard_per_row <= 0 || !(guard_limit >= 0.0f))) || (invalid_ids && (msg || !f_out_ids || !f_out_scores))) {
    set_error("candidates_finish: bad argument");
    return RAILS_EINVAL;
  }
  const int r = candidates_finish(exact_scores, ld, approx, positions, cand_ld, cap, workspace, ids, n_items, rows, k, default_eps, safety, one_sided != 0,
                                  guard_values, guard_per_row, guard_limit, out_scores, out_ids, invalid_ids, width, f_k, f_out_ids, f_out_scores, state,
                                  state_host, msg, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "candidates_finish");
}

int rails_filter_seen_ids(const int64_t* top_ids, const float* top_scores, int32_t rows, int32_t k_prime,
                          const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids, float* out_scores,
                          void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || k_prime < 0 || width < 0 || k < 0) { set_error("filter_seen_ids: negative size"); return RAILS_EINVAL; }
  if (rows == 0 || k == 0) return RAILS_OK;
  if (!top_ids || !top_scores || !out_ids || !out_scores || (width > 0 && !invalid_ids)) {
    set_error("filter_seen_ids: NULL pointer");
    return RAILS_EINVAL;
  }
  const int r = filter_seen(top_ids, top_scores, rows, k_prime, invalid_ids, width, k, out_ids, out_scores,
                            (hipStream_t)stream);
  return r == kOk ? r : fail(r, "filter_seen_ids");
}

// ---- HSTU query encoder, eval path ----
int rails_hstu_preprocess(const float* embeddings, const int64_t* ids, const int64_t* lengths, const float* pos_emb, int32_t batch,
                          int32_t seq_len, int32_t dim, float scale, float* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || seq_len < 0 || dim < 0) { set_error("hstu_preprocess: negative size"); return RAILS_EINVAL; }
  if (batch == 0 || seq_len == 0 || dim == 0) return RAILS_OK;
  if (!embeddings || !ids || !lengths || !pos_emb || !out) { set_error("hstu_preprocess: NULL pointer"); return RAILS_EINVAL; }
  return fail(hstu_preprocess(embeddings, ids, lengths, pos_emb, batch, seq_len, dim, scale, out, (hipStream_t)stream), "hstu_preprocess");
}

int rails_rows_layer_norm(const float* x, int64_t ldx, int64_t rows, int32_t dim, float eps, const float* mul, int64_t ldm, float* out,
                          int64_t ldo, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || dim <= 0) { set_error("rows_layer_norm: bad size"); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!x || !out || ldx < dim || ldo < dim || (mul && ldm < dim)) { set_error("rows_layer_norm: NULL pointer or short stride"); return RAILS_EINVAL; }
  return fail(rows_layer_norm(x, ldx, rows, dim, eps, mul, ldm, out, ldo, (hipStream_t)stream), "rows_layer_norm");
}

int rails_gemm_f32(const float* a, int64_t lda, const float* w, int32_t w_is_nk, const float* bias, const float* residual, int64_t ldr,
                   int64_t m, int32_t n, int32_t k, int32_t act, const int64_t* lengths, int32_t seq_len, float* c, int64_t ldc,
                   void* stream) {
  g_err[0] = '\0';
  if (m < 0 || n < 0 || k <= 0) { set_error("gemm_f32: bad size"); return RAILS_EINVAL; }
  if (m == 0 || n == 0) return RAILS_OK;
  if (!a || !w || !c || lda < k || ldc < n || (residual && ldr < n)) { set_error("gemm_f32: NULL pointer or short stride"); return RAILS_EINVAL; }
  if (act < RAILS_ACT_NONE || act > RAILS_ACT_GELU) { set_error("gemm_f32: unknown activation %d", act); return RAILS_EINVAL; }
  if (lengths && (seq_len <= 0 || m % seq_len != 0)) { set_error("gemm_f32: rows are not batch * seq_len"); return RAILS_EINVAL; }
  return fail(gemm_f32(a, lda, w, w_is_nk ? 1 : 0, bias, residual, ldr, m, n, k, act, lengths, seq_len, c, ldc, (hipStream_t)stream), "gemm_f32");
}

int rails_gemm_f32_id_masked(const float* a, int64_t lda, const float* w, int32_t w_is_nk, const float* bias, const float* residual,
                             int64_t ldr, int64_t m, int32_t n, int32_t k, int32_t act, const int64_t* row_ids, float* c, int64_t ldc,
                             void* stream) {
  g_err[0] = '\0';
  if (m < 0 || n < 0 || k <= 0) { set_error("gemm_f32_id_masked: bad size"); return RAILS_EINVAL; }
  if (m == 0 || n == 0) return RAILS_OK;
  if (!a || !w || !c || !row_ids || lda < k || ldc < n || (residual && ldr < n)) {
    set_error("gemm_f32_id_masked: NULL pointer or short stride");
    return RAILS_EINVAL;
  }
  if (act < RAILS_ACT_NONE || act > RAILS_ACT_GELU) { set_error("gemm_f32_id_masked: unknown activation %d", act); return RAILS_EINVAL; }
  return fail(gemm_f32(a, lda, w, w_is_nk ? 1 : 0, bias, residual, ldr, m, n, k, act, nullptr, 0, c, ldc, (hipStream_t)stream, row_ids),
              "gemm_f32_id_masked");
}

int rails_mol_gate_combine(const float* logits, int64_t ld_logits, const float* pair_part, int64_t ld_pair, const float* query_part,
                           const float* item_part, int64_t rows, int32_t items_per_query, int32_t num_logits, int32_t item_part_per_row,
                           int32_t combination, int32_t renormalise, float eps, float* out, float* probs_out, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || items_per_query <= 0 || num_logits <= 0) { set_error("gate_combine: bad size"); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!logits || !out || ld_logits < num_logits || (pair_part && ld_pair < num_logits) || rows % items_per_query != 0) {
    set_error("gate_combine: NULL pointer, short stride or rows not a multiple of items_per_query");
    return RAILS_EINVAL;
  }
  if (combination != RAILS_COMBINE_GLU_SILU && combination != RAILS_COMBINE_NONE) { set_error("gate_combine: unknown combination %d", combination); return RAILS_EINVAL; }
  if (combination == RAILS_COMBINE_GLU_SILU && (!pair_part || !query_part || !item_part)) { set_error("gate_combine: glu_silu needs all three gate parts"); return RAILS_EINVAL; }
  if (!pair_part && !query_part && !item_part) { set_error("gate_combine: no gate part"); return RAILS_EINVAL; }
  return fail(gate_combine(logits, ld_logits, pair_part, ld_pair, query_part, item_part, rows, items_per_query, num_logits, item_part_per_row ? 1 : 0,
                           combination == RAILS_COMBINE_GLU_SILU ? 1 : 0, renormalise ? 1 : 0, eps, out, probs_out, (hipStream_t)stream), "gate_combine");
}

int rails_glu_f32(const float* x, int64_t ldx, const float* w, const float* b, int64_t rows, int32_t in_features, int32_t out_features,
                  int32_t kind, float* scratch, float* out, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || in_features <= 0 || out_features <= 0) { set_error("glu_f32: bad size"); return RAILS_EINVAL; }
  if (kind != RAILS_GEGLU && kind != RAILS_SWIGLU) { set_error("glu_f32: unknown kind %d", kind); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!x || !w || !scratch || !out || ldx < in_features) { set_error("glu_f32: NULL pointer or short stride"); return RAILS_EINVAL; }
  const int n2 = 2 * out_features;
  const int rc = gemm_f32(x, ldx, w, 0, b, nullptr, 0, rows, n2, in_features, 0, nullptr, 0, scratch, n2, (hipStream_t)stream);
  if (rc != kOk) return fail(rc, "glu_f32 (gemm)");
  return fail(glu_gate(scratch, n2, rows, out_features, kind, out, (hipStream_t)stream), "glu_f32 (gate)");
}

int rails_hstu_time_buckets(const int64_t* timestamps, int32_t batch, int32_t seq_len, const int64_t* thresholds, int32_t num_buckets,
                            uint8_t* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || seq_len < 0 || num_buckets <= 0) { set_error("hstu_time_buckets: bad size"); return RAILS_EINVAL; }
  if (batch == 0 || seq_len == 0) return RAILS_OK;
  if (!timestamps || !thresholds || !out) { set_error("hstu_time_buckets: NULL pointer"); return RAILS_EINVAL; }
  const int r = hstu_time_buckets(timestamps, batch, seq_len, thresholds, num_buckets, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "hstu_time_buckets");
}

int rails_hstu_attention(const float* uvqk, int64_t ld, int32_t batch, int32_t seq_len, int32_t heads, int32_t dqk, int32_t dv,
                         const int64_t* lengths, const uint8_t* buckets, const float* ts_w, const float* pos_w, int32_t num_buckets,
                         float* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || seq_len < 0 || heads <= 0 || dqk <= 0 || dv <= 0) { set_error("hstu_attention: bad size"); return RAILS_EINVAL; }
  if (batch == 0 || seq_len == 0) return RAILS_OK;
  if (!uvqk || !lengths || !out || ld < (int64_t)2 * heads * (dqk + dv)) { set_error("hstu_attention: NULL pointer or short stride"); return RAILS_EINVAL; }
  if (buckets && (!ts_w || !pos_w || num_buckets <= 0)) { set_error("hstu_attention: buckets without bias tables"); return RAILS_EINVAL; }
  const int r = hstu_attention(uvqk, ld, batch, seq_len, heads, dqk, dv, lengths, buckets, ts_w, pos_w, num_buckets, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "hstu_attention");
}

int rails_hstu_fused_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets) {
  return hstu_fused_supported(seq_len, dim, heads, dqk, dv, num_buckets) ? 1 : 0;
}

int rails_hstu_encode_fused(const float* embeddings, const int64_t* ids, const int64_t* lengths, const uint8_t* buckets,
                            const float* pos_emb, const rails_hstu_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len,
                            int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets, int32_t postproc_mode, float eps,
                            float* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || n_blocks < 0 || (postproc_mode != 0 && postproc_mode != 1)) { set_error("hstu_encode_fused: bad argument"); return RAILS_EINVAL; }
  if (batch == 0) return RAILS_OK;
  if (!embeddings || !ids || !lengths || !pos_emb || !out || (n_blocks > 0 && !layers)) { set_error("hstu_encode_fused: NULL pointer"); return RAILS_EINVAL; }
  const int r = hstu_encode_fused(embeddings, ids, lengths, buckets, pos_emb, layers, n_blocks, batch, seq_len, dim, heads, dqk, dv,
                                  num_buckets, postproc_mode, eps, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "hstu_encode_fused");
}

int rails_hstu_decode_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets) {
  return hstu_decode_supported(seq_len, dim, heads, dqk, dv, num_buckets) ? 1 : 0;
}

int rails_hstu_decode(const float* embeddings, const int64_t* ids, const int64_t* positions, const int64_t* lengths,
                      const int64_t* timestamps, const int64_t* thresholds, const float* pos_emb, const rails_hstu_decode_layer* layers,
                      int32_t n_blocks, int32_t batch, int32_t seq_len, int64_t cache_rows, int32_t dim, int32_t heads, int32_t dqk,
                      int32_t dv, int32_t num_buckets, int32_t linear_act, int32_t postproc_mode, float eps, float* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || n_blocks < 1 || seq_len < 1 || dim < 1 || heads < 1 || dqk < 1 || dv < 1 || cache_rows < batch) {
    set_error("hstu_decode: bad size (batch %d, n_blocks %d, seq_len %d, dim %d, heads %d, dqk %d, dv %d, cache_rows %lld)", batch, n_blocks,
              seq_len, dim, heads, dqk, dv, (long long)cache_rows);
    return RAILS_EINVAL;
  }
  if ((linear_act != RAILS_ACT_NONE && linear_act != RAILS_ACT_SILU) || (postproc_mode != 0 && postproc_mode != 1)) {
    set_error("hstu_decode: bad linear_act %d or postproc_mode %d", linear_act, postproc_mode);
    return RAILS_EINVAL;
  }
  if (timestamps && (!thresholds || num_buckets < 1)) { set_error("hstu_decode: timestamps without a threshold table"); return RAILS_EINVAL; }
  if (!hstu_decode_supported(seq_len, dim, heads, dqk, dv, num_buckets)) {
    set_error("hstu_decode: dim %d, heads %d, dqk %d, dv %d, %d buckets not supported (dim <= 1024, dqk <= 32, dv <= 32, <= 255 buckets, "
              "row buffers within the LDS bound)", dim, heads, dqk, dv, num_buckets);
    return RAILS_ENOTSUP;
  }
  if (batch == 0) return RAILS_OK;
  if (!embeddings || !ids || !positions || !lengths || !pos_emb || !layers || !out) { set_error("hstu_decode: NULL pointer"); return RAILS_EINVAL; }
  const int r = hstu_decode(embeddings, ids, positions, lengths, timestamps, thresholds, pos_emb, layers, n_blocks, batch, seq_len, cache_rows,
                            dim, heads, dqk, dv, num_buckets, linear_act, postproc_mode, eps, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "hstu_decode");
}

int rails_hstu_decode_rows_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets) {
  return hstu_decode_rows_supported(seq_len, dim, heads, dqk, dv, num_buckets) ? 1 : 0;
}

int64_t rails_hstu_decode_rows_workspace_floats(int64_t work_rows, int32_t batch, int32_t dim, int32_t heads, int32_t dqk, int32_t dv) {
  if (work_rows < 0 || batch < 0 || dim < 0 || heads < 0 || dqk < 0 || dv < 0) return 0;
  return hstu_decode_rows_workspace_floats(work_rows, batch, dim, heads, dv);
}

int rails_hstu_decode_rows(const float* embeddings, const int64_t* ids, const int64_t* positions, const int64_t* counts, int32_t max_rows,
                           const int64_t* lengths, const int64_t* timestamps, const int64_t* thresholds, const float* pos_emb,
                           const rails_hstu_decode_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len, int64_t cache_rows,
                           int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets, int32_t linear_act,
                           int32_t postproc_mode, float eps, float* work, float* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || n_blocks < 1 || seq_len < 1 || dim < 1 || heads < 1 || dqk < 1 || dv < 1 || cache_rows < batch) {
    set_error("hstu_decode_rows: bad size (batch %d, n_blocks %d, seq_len %d, dim %d, heads %d, dqk %d, dv %d, cache_rows %lld)", batch,
              n_blocks, seq_len, dim, heads, dqk, dv, (long long)cache_rows);
    return RAILS_EINVAL;
  }
  if (max_rows < 1) { set_error("hstu_decode_rows: max_rows %d < 1", max_rows); return RAILS_EINVAL; }
  if ((int64_t)batch * max_rows > RAILS_HSTU_DECODE_MAX_ROWS) {
    set_error("hstu_decode_rows: batch %d x max_rows %d = %lld work rows, more than the %d of one step", batch, max_rows,
              (long long)batch * max_rows, RAILS_HSTU_DECODE_MAX_ROWS);
    return RAILS_EINVAL;
  }
  if (max_rows > seq_len) {
    set_error("hstu_decode_rows: max_rows %d outside [1, seq_len %d]", max_rows, seq_len);
    return RAILS_EINVAL;
  }
  if ((linear_act != RAILS_ACT_NONE && linear_act != RAILS_ACT_SILU) || (postproc_mode != 0 && postproc_mode != 1)) {
    set_error("hstu_decode_rows: bad linear_act %d or postproc_mode %d", linear_act, postproc_mode);
    return RAILS_EINVAL;
  }
  if (timestamps && (!thresholds || num_buckets < 1)) { set_error("hstu_decode_rows: timestamps without a threshold table"); return RAILS_EINVAL; }
  if (!hstu_decode_rows_supported(seq_len, dim, heads, dqk, dv, num_buckets)) {
    set_error("hstu_decode_rows: dim %d, heads %d, dqk %d, dv %d, %d buckets not supported (dim <= 1024, dqk <= 32, dv <= 32, <= 255 buckets, "
              "heads * dv <= 1024)", dim, heads, dqk, dv, num_buckets);
    return RAILS_ENOTSUP;
  }
  if (batch == 0) return RAILS_OK;
  if (!embeddings || !ids || !positions || !lengths || !pos_emb || !layers || !work || !out) {
    set_error("hstu_decode_rows: NULL pointer");
    return RAILS_EINVAL;
  }
  const int r = hstu_decode_rows(embeddings, ids, positions, counts, max_rows, lengths, timestamps, thresholds, pos_emb, layers, n_blocks, batch,
                                 seq_len, cache_rows, dim, heads, dqk, dv, num_buckets, linear_act, postproc_mode, eps, work, out,
                                 (hipStream_t)stream);
  return r == kOk ? r : fail(r, "hstu_decode_rows");
}

// ---- SASRec query encoder, eval path ----
int rails_sasrec_attention(const float* qkv, int64_t ld, int32_t batch, int32_t seq_len, int32_t dim, int32_t heads, float* out,
                           void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || seq_len < 0 || dim <= 0 || heads <= 0) { set_error("sasrec_attention: bad size"); return RAILS_EINVAL; }
  if (dim % heads != 0) { set_error("sasrec_attention: dim %d is not a multiple of heads %d", dim, heads); return RAILS_EINVAL; }
  if (dim / heads > 64) { set_error("sasrec_attention: head_dim = %d (supported: <= 64)", dim / heads); return RAILS_ENOTSUP; }
  if (batch == 0 || seq_len == 0) return RAILS_OK;
  if (!qkv || !out || ld < (int64_t)3 * dim) { set_error("sasrec_attention: NULL pointer or short stride"); return RAILS_EINVAL; }
  const int r = sasrec_attention(qkv, ld, batch, seq_len, heads, dim / heads, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "sasrec_attention");
}

int rails_sasrec_fused_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t ffn_dim) {
  return sasrec_fused_supported(seq_len, dim, heads, ffn_dim) ? 1 : 0;
}

int rails_sasrec_encode_fused(const float* embeddings, const int64_t* ids, const int64_t* lengths, const float* pos_emb,
                              const rails_sasrec_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len, int32_t dim,
                              int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps, float* out,
                              void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || n_blocks < 0 || seq_len <= 0 || dim <= 0 || heads <= 0 || ffn_dim <= 0) { set_error("sasrec_encode_fused: bad size"); return RAILS_EINVAL; }
  if (dim % heads != 0) { set_error("sasrec_encode_fused: dim %d is not a multiple of heads %d", dim, heads); return RAILS_EINVAL; }
  if ((ffn_act != RAILS_ACT_RELU && ffn_act != RAILS_ACT_GELU) || (postproc_mode != 0 && postproc_mode != 1)) {
    set_error("sasrec_encode_fused: bad ffn_act %d or postproc_mode %d", ffn_act, postproc_mode);
    return RAILS_EINVAL;
  }
  if (batch == 0) return RAILS_OK;
  if (!embeddings || !ids || !lengths || !pos_emb || !out || (n_blocks > 0 && !layers)) { set_error("sasrec_encode_fused: NULL pointer"); return RAILS_EINVAL; }
  if (!sasrec_fused_supported(seq_len, dim, heads, ffn_dim)) {
    set_error("sasrec_encode_fused: seq_len %d, dim %d, heads %d, ffn_dim %d not supported (seq_len <= 64, dim <= 128, ffn_dim <= 128, "
              "head_dim <= 64)", seq_len, dim, heads, ffn_dim);
    return RAILS_ENOTSUP;
  }
  const int r = sasrec_encode_fused(embeddings, ids, lengths, pos_emb, layers, n_blocks, batch, seq_len, dim, heads, ffn_dim, ffn_act,
                                    postproc_mode, eps, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, "sasrec_encode_fused");
}

int rails_sasrec_decode_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t ffn_dim) {
  return sasrec_decode_supported(seq_len, dim, heads, ffn_dim) ? 1 : 0;
}

int64_t rails_sasrec_decode_workspace_floats(int32_t batch, int32_t dim, int32_t ffn_dim) {
  return batch < 0 || dim < 0 || ffn_dim < 0 ? 0 : sasrec_decode_workspace_floats(batch, dim, ffn_dim);
}

static int sasrec_decode_entry(const char* name, const float* embeddings, const int64_t* ids, const int64_t* lengths, const int64_t* new_counts,
                               int32_t max_new, const float* pos_emb, const rails_sasrec_decode_layer* layers, int32_t n_blocks, int32_t batch,
                               int32_t seq_len, int32_t dim, int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps,
                               float* work, float* out, void* stream) {
  g_err[0] = '\0';
  if (batch < 0 || n_blocks < 1 || seq_len <= 0 || dim <= 0 || heads <= 0 || ffn_dim <= 0) {
    set_error("%s: bad size (batch %d, n_blocks %d, seq_len %d, dim %d, heads %d, ffn_dim %d)", name, batch, n_blocks, seq_len, dim, heads,
              ffn_dim);
    return RAILS_EINVAL;
  }
  if (dim % heads != 0) { set_error("%s: dim %d is not a multiple of heads %d", name, dim, heads); return RAILS_EINVAL; }
  if ((ffn_act != RAILS_ACT_RELU && ffn_act != RAILS_ACT_GELU) || (postproc_mode != 0 && postproc_mode != 1)) {
    set_error("%s: bad ffn_act %d or postproc_mode %d", name, ffn_act, postproc_mode);
    return RAILS_EINVAL;
  }
  if (!sasrec_decode_supported(seq_len, dim, heads, ffn_dim)) {
    set_error("%s: seq_len %d, dim %d, heads %d, ffn_dim %d not supported (seq_len <= 2048, dim <= 1024, ffn_dim <= 1024, "
              "head_dim <= 64)", name, seq_len, dim, heads, ffn_dim);
    return RAILS_ENOTSUP;
  }
  if (max_new < 1 || max_new > seq_len) {
    set_error("%s: max_new %d not supported (1 <= max_new <= seq_len %d)", name, max_new, seq_len);
    return RAILS_ENOTSUP;
  }
  if ((int64_t)batch * max_new > RAILS_SASREC_DECODE_MAX_ROWS) {
    set_error("%s: batch %d x max_new %d = %lld work rows not supported (at most %d per step)", name, batch, max_new,
              (long long)batch * max_new, RAILS_SASREC_DECODE_MAX_ROWS);
    return RAILS_ENOTSUP;
  }
  if (batch == 0) return RAILS_OK;
  if (!embeddings || !ids || !lengths || !pos_emb || !layers || !work || !out) { set_error("%s: NULL pointer", name); return RAILS_EINVAL; }
  for (int i = 0; i < n_blocks; ++i) {
    const rails_sasrec_decode_layer& L = layers[i];
    if (!L.in_proj_weight || !L.in_proj_bias || !L.out_proj_weight || !L.out_proj_bias || !L.conv1_weight || !L.conv1_bias ||
        !L.conv2_weight || !L.conv2_bias || !L.k || !L.v) {
      set_error("%s: NULL pointer in layers[%d]", name, i);
      return RAILS_EINVAL;
    }
  }
  const int r = sasrec_decode(embeddings, ids, lengths, new_counts, max_new, pos_emb, layers, n_blocks, batch, seq_len, dim, heads, ffn_dim,
                              ffn_act, postproc_mode, eps, work, out, (hipStream_t)stream);
  return r == kOk ? r : fail(r, name);
}

int rails_sasrec_decode(const float* embeddings, const int64_t* ids, const int64_t* lengths, const float* pos_emb,
                        const rails_sasrec_decode_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len, int32_t dim,
                        int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps, float* work, float* out,
                        void* stream) {
  return sasrec_decode_entry("sasrec_decode", embeddings, ids, lengths, nullptr, 1, pos_emb, layers, n_blocks, batch, seq_len, dim, heads,
                             ffn_dim, ffn_act, postproc_mode, eps, work, out, stream);
}

int rails_sasrec_decode_rows(const float* embeddings, const int64_t* ids, const int64_t* lengths, const int64_t* new_counts, int32_t max_new,
                             const float* pos_emb, const rails_sasrec_decode_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len,
                             int32_t dim, int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps, float* work,
                             float* out, void* stream) {
  return sasrec_decode_entry("sasrec_decode_rows", embeddings, ids, lengths, new_counts, max_new, pos_emb, layers, n_blocks, batch, seq_len,
                             dim, heads, ffn_dim, ffn_act, postproc_mode, eps, work, out, stream);
}

int rails_rows_normalize(const float* x, int64_t ldx, const int64_t* row_index, int64_t rows, int32_t dim, int32_t mode, float eps,
                         float* out, void* stream) {
  g_err[0] = '\0';
  if (rows < 0 || dim <= 0 || (mode != 0 && mode != 1)) { set_error("rows_normalize: bad argument"); return RAILS_EINVAL; }
  if (rows == 0) return RAILS_OK;
  if (!x || !out || ldx < dim) { set_error("rows_normalize: NULL pointer or short stride"); return RAILS_EINVAL; }
  return fail(rows_normalize(x, ldx, row_index, rows, dim, mode, eps, out, (hipStream_t)stream), "rows_normalize");
}

size_t rails_ivf_build_workspace_bytes(const rails_mol_shape* s, int64_t n_items, int32_t nlist, int32_t n_sample) {
  if (!shape_ok(s) || n_items < 0 || nlist <= 0 || n_sample < 0) return 0;
  return ivf_build_workspace_bytes(*s, n_items, nlist, n_sample);
}

static int ivf_source(const rails_mol_shape* s, const float* index, const void* components16, int64_t n_items, int32_t nlist, const char* what) {
  if (!shape_ok(s)) return RAILS_EINVAL;
  if ((index != nullptr) == (components16 != nullptr)) { set_error("%s: pass exactly one of index and components16", what); return RAILS_EINVAL; }
  return ivf_check(*s, n_items, nlist, index != nullptr);
}

int rails_ivf_components16_build(const rails_mol_shape* s, const float* index, int64_t n_items, void* components16, int64_t n_total,
                                 int64_t first_item, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (s->dot_product_dimension % 8 != 0) { set_error("ivf_components16_build: d must be a multiple of 8"); return RAILS_ENOTSUP; }
  if (n_items < 0 || first_item < 0 || first_item + n_items > n_total) { set_error("ivf_components16_build: items [%lld, %lld) outside a table of %lld", (long long)first_item, (long long)(first_item + n_items), (long long)n_total); return RAILS_EINVAL; }
  if (n_items == 0) return RAILS_OK;
  if (!index || !components16) { set_error("ivf_components16_build: NULL pointer"); return RAILS_EINVAL; }
  if (is_split(*s)) { set_error("ivf_components16_build: needs an fp32-format item index (build one with precision = RAILS_PRECISION_FP32)"); return RAILS_ENOTSUP; }
  return fail(ivf_components16(*s, index, n_items, components16, n_total, first_item, (hipStream_t)stream), "ivf_components16_build");
}

int rails_ivf_train(const rails_mol_shape* s, const float* index, const void* components16, int64_t n_items, const int32_t* sample_positions,
                    int32_t n_sample, int32_t nlist, int32_t iters, int32_t init, float* centroids, void* workspace, size_t workspace_bytes, void* stream) {
  g_err[0] = '\0';
  const int c = ivf_source(s, index, components16, n_items, nlist, "ivf_train");
  if (c != kOk) return c;
  if (n_sample < nlist || n_sample > n_items || iters < 0) {
    set_error("ivf_train: n_sample = %d outside [nlist = %d, n_items = %lld] or iters = %d < 0", n_sample, nlist, (long long)n_items, iters);
    return RAILS_EINVAL;
  }
  if (!sample_positions || !centroids || !workspace) { set_error("ivf_train: NULL pointer"); return RAILS_EINVAL; }
  return fail(ivf_train(*s, index, components16, n_items, sample_positions, n_sample, nlist, iters, init, centroids, workspace, workspace_bytes,
                        (hipStream_t)stream), "ivf_train");
}

int rails_ivf_assign(const rails_mol_shape* s, const float* index, const void* components16, int64_t n_items, int32_t nlist, const float* centroids,
                     int32_t* assign, void* stream) {
  g_err[0] = '\0';
  const int c = ivf_source(s, index, components16, n_items, nlist, "ivf_assign");
  if (c != kOk) return c;
  if (!centroids || !assign) { set_error("ivf_assign: NULL pointer"); return RAILS_EINVAL; }
  return fail(ivf_assign(*s, index, components16, n_items, nlist, centroids, assign, (hipStream_t)stream), "ivf_assign");
}

int rails_ivf_build_lists(const rails_mol_shape* s, const float* index, const void* components16, int64_t n_items, int32_t nlist, const float* centroids,
                          void* vectors, int32_t* positions, int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
  g_err[0] = '\0';
  const int c = ivf_source(s, index, components16, n_items, nlist, "ivf_build_lists");
  if (c != kOk) return c;
  if (!centroids || !vectors || !positions || !offsets || !workspace) { set_error("ivf_build_lists: NULL pointer"); return RAILS_EINVAL; }
  return fail(ivf_build_lists(*s, index, components16, n_items, nlist, centroids, vectors, positions, offsets, workspace, workspace_bytes,
                              (hipStream_t)stream), "ivf_build_lists");
}

size_t rails_ivf_lists_edit_workspace_bytes(const rails_mol_shape* s, int64_t n_old, int32_t nlist, int64_t m) {
  g_err[0] = '\0';
  if (!shape_ok(s) || ivf_lists_edit_check(*s, n_old, nlist, m) != kOk) return 0;
  return ivf_lists_edit_workspace_bytes(*s, n_old, (int)m);
}

int rails_ivf_lists_edit(const rails_mol_shape* s, const float* source_index, int32_t src_in_place, const int64_t* positions, int64_t m, int64_t n_keep,
                         int32_t nlist, const float* centroids, const void* old_vectors, const int32_t* old_positions, const int32_t* old_offsets,
                         int64_t n_old, void* new_vectors, int32_t* new_positions, int32_t* new_offsets, int64_t n_new, void* workspace,
                         size_t workspace_bytes, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  const int c = ivf_lists_edit_check(*s, n_old, nlist, m);
  if (c != kOk) return c;
  if (is_split(*s)) { set_error("ivf_lists_edit: needs an fp32-format item index (build one with precision = RAILS_PRECISION_FP32)"); return RAILS_ENOTSUP; }
  if (n_keep < 0 || n_new < 1 || n_new > std::min(n_old, n_keep) + m || n_new > 0x7fffffffLL) {
    set_error("ivf_lists_edit: n_new = %lld outside [1, min(n_old = %lld, n_keep = %lld) + m = %lld]", (long long)n_new, (long long)n_old, (long long)n_keep,
              (long long)m);
    return RAILS_EINVAL;
  }
  if (!old_vectors || !old_positions || !old_offsets || !new_vectors || !new_positions || !new_offsets || !workspace ||
      (m > 0 && (!source_index || !positions || !centroids))) {
    set_error("ivf_lists_edit: NULL pointer");
    return RAILS_EINVAL;
  }
  return fail(ivf_lists_edit(*s, source_index, src_in_place ? 1 : 0, positions, (int)m, n_keep, nlist, centroids, old_vectors, old_positions, old_offsets,
                             n_old, new_vectors, new_positions, new_offsets, n_new, workspace, workspace_bytes, (hipStream_t)stream), "ivf_lists_edit");
}

int rails_ivf_plan(const rails_mol_shape* s, const int32_t* offsets, int32_t nlist, int32_t nprobe, int32_t k_per_group, int32_t* max_probes,
                   int32_t* max_list) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (!offsets || !max_probes || !max_list || nlist <= 0 || nprobe <= 0 || k_per_group <= 0) { set_error("ivf_plan: bad argument"); return RAILS_EINVAL; }
  int mp = 0, ml = 0;
  ivf_plan(offsets, s->item_dot_product_groups, nlist, std::min(nprobe, nlist), k_per_group, &mp, &ml);
  *max_probes = mp;
  *max_list = ml;
  return RAILS_OK;
}

size_t rails_ivf_search_workspace_bytes(const rails_mol_shape* s, int32_t batch, int32_t nlist, int32_t nprobe, int32_t max_probes, int32_t max_list,
                                        int32_t k_per_group) {
  if (!shape_ok(s) || batch <= 0 || ivf_search_check(*s, nlist, nprobe, max_probes, max_list, k_per_group, INT64_MAX) != kOk) return 0;
  return ivf_search_workspace_bytes(*s, batch, nlist, nprobe, max_probes, max_list, k_per_group);
}

int rails_ivf_search(const rails_mol_shape* s, const float* eq, int32_t batch, const float* centroids, const void* vectors, const int32_t* positions,
                     const int32_t* offsets, int64_t n_items, int32_t nlist, int32_t nprobe, int32_t max_probes, int32_t max_list, int32_t k_per_group,
                     void* workspace, size_t workspace_bytes, int64_t* out_positions, int32_t* unfilled, void* stream) {
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (batch < 0) { set_error("ivf_search: negative batch"); return RAILS_EINVAL; }
  const int c = ivf_search_check(*s, nlist, nprobe, max_probes, max_list, k_per_group, n_items);
  if (c != kOk) return c;
  if (batch == 0) return RAILS_OK;
  if (!eq || !centroids || !vectors || !positions || !offsets || !workspace || !out_positions) { set_error("ivf_search: NULL pointer"); return RAILS_EINVAL; }
  return fail(ivf_search(*s, eq, batch, centroids, vectors, positions, offsets, n_items, nlist, nprobe, max_probes, max_list, k_per_group, workspace,
                         workspace_bytes, out_positions, unfilled, (hipStream_t)stream), "ivf_search");
}


int rails_ivf_list_words(const int32_t* positions, int32_t groups, int64_t n_items, const uint32_t* eff_tags, const uint32_t* visible_words,
                         uint32_t* list_words, void* stream) {
  g_err[0] = '\0';
  if (groups < 1 || n_items < 1 || n_items > 0x7fffffffLL) { set_error("ivf_list_words: groups = %d or n_items = %lld outside [1, 2^31)", groups, (long long)n_items); return RAILS_EINVAL; }
  if (!positions || !list_words || (eff_tags == nullptr) == (visible_words == nullptr)) {
    set_error("ivf_list_words: NULL pointer, or not exactly one of eff_tags and visible_words");
    return RAILS_EINVAL;
  }
  return fail(ivf_list_words(positions, groups, n_items, eff_tags, visible_words, list_words, (hipStream_t)stream), "ivf_list_words");
}

int rails_ivf_list_counts(const uint32_t* list_words, const int32_t* offsets, int32_t groups, int64_t n_items, int32_t nlist, const uint32_t* allowed,
                          int32_t count_rows, int32_t* counts, void* stream) {
  g_err[0] = '\0';
  if (groups < 1 || n_items < 1 || n_items > 0x7fffffffLL || nlist < 1 || nlist > 4096 || count_rows < 1) {
    set_error("ivf_list_counts: groups = %d, n_items = %lld, nlist = %d or count_rows = %d outside the limits", groups, (long long)n_items, nlist, count_rows);
    return RAILS_EINVAL;
  }
  if (!list_words || !offsets || !allowed || !counts) { set_error("ivf_list_counts: NULL pointer"); return RAILS_EINVAL; }
  return fail(ivf_list_counts(list_words, offsets, groups, n_items, nlist, allowed, count_rows, counts, (hipStream_t)stream), "ivf_list_counts");
}

int rails_ivf_plan_filtered(const int32_t* counts, int32_t count_rows, int32_t groups, int32_t nlist, int32_t nprobe, int32_t k_per_group,
                            int32_t* max_probes) {
  g_err[0] = '\0';
  if (!counts || !max_probes || count_rows < 1 || groups < 1 || nlist <= 0 || nprobe <= 0 || k_per_group <= 0) { set_error("ivf_plan_filtered: bad argument"); return RAILS_EINVAL; }
  *max_probes = ivf_plan_filtered(counts, count_rows, groups, nlist, std::min(nprobe, nlist), k_per_group);
  return RAILS_OK;
}

int rails_ivf_search_filtered(const rails_mol_shape* s, const float* eq, int32_t batch, const float* centroids, const void* vectors, const int32_t* positions,
                              const int32_t* offsets, int64_t n_items, int32_t nlist, int32_t nprobe, int32_t max_probes, int32_t max_list,
                              int32_t k_per_group, void* workspace, size_t workspace_bytes, int64_t* out_positions, int32_t* unfilled,
                              const uint32_t* list_words, const uint32_t* allowed, const int32_t* counts, int32_t count_rows, void* stream) {
  if (!list_words)
    return rails_ivf_search(s, eq, batch, centroids, vectors, positions, offsets, n_items, nlist, nprobe, max_probes, max_list, k_per_group, workspace,
                            workspace_bytes, out_positions, unfilled, stream);
  g_err[0] = '\0';
  if (!shape_ok(s)) return RAILS_EINVAL;
  if (batch < 0) { set_error("ivf_search_filtered: negative batch"); return RAILS_EINVAL; }
  const int c = ivf_search_check(*s, nlist, nprobe, max_probes, max_list, k_per_group, n_items);
  if (c != kOk) return c;
  if (batch == 0) return RAILS_OK;
  if (!eq || !centroids || !vectors || !positions || !offsets || !workspace || !out_positions || !allowed || !counts) {
    set_error("ivf_search_filtered: NULL pointer");
    return RAILS_EINVAL;
  }
  if (count_rows != 1 && count_rows != batch) { set_error("ivf_search_filtered: count_rows = %d is neither 1 nor batch = %d", count_rows, batch); return RAILS_EINVAL; }
  return fail(ivf_search_filtered(*s, eq, batch, centroids, vectors, positions, offsets, n_items, nlist, nprobe, max_probes, max_list, k_per_group, workspace,
                                  workspace_bytes, out_positions, unfilled, list_words, allowed, counts, count_rows, (hipStream_t)stream),
              "ivf_search_filtered");
}

}  // extern "C"
