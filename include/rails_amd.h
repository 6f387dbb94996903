/* rails_amd — C ABI of the MI355X-native Mixture-of-Logits (MoL) retrieval path.
 *
 * The reference (bailuding/rails) is pure Python/PyTorch and has no FFI of its own; the "interface
 * each entry point replaces" is therefore a Python call site of the reference, cited per function as
 * `path:line` inside the reference repository.  INTEGRATION.md shows the ctypes binding a maintainer
 * adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM of the current HIP device) unless stated otherwise;
 *     matrices are dense row-major exactly as the reference's state_dict() / tensors hold them;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on it: no allocation, no synchronisation, no host copies;
 *   - return value 0 on success, a negative RAILS_E* code otherwise; rails_last_error() returns
 *     a thread-local human-readable message for the last failure;
 *   - `run_if` (where an entry point has it) is the LAUNCH PREDICATE: NULL, or an int32 in device memory that every kernel of the
 *     call reads when it starts, in stream order -- the call is a no-op unless it is non-zero.  It is how a caller enqueues a
 *     fallback behind a device-side verdict without reading the verdict on the host (rails_rescore_verdict and rails_range_flag_i32
 *     write such flags).  No counterpart in the reference;
 *   - packed buffers (`gate pack`, `item index`, `query pack`) are opaque fp32 blobs whose sizes
 *     come from the *_floats() helpers; they are only valid for the shape they were built for.
 */
#ifndef RAILS_AMD_H_
#define RAILS_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this interface: bumped whenever a struct gains a field or an entry point changes meaning (round 2 -> 3: 3, the
 * structs of round 2 carried no version; 5: the launch predicate became the explicit `run_if` argument of the entry points that
 * honour it and the per-thread rails_set_run_predicate is gone -- the library keeps no state between calls but the last error;
 * 6: rails_mol_coarse_topk gained its out_of_range output and its optional int8 pre-filter (rails_mol_coarse_prefilter_*),
 * rails_topk_candidates is new, rails_mol_score_indexed takes any n_cand; 7: rails_rescore_verdict gained its guard arguments and state[7], the rails_*_probe_* entry points are new, and rails_mol_score_topk / _survivors / rails_select_survivors -- the selection fused into the scoring kernels, 0.9 % slower than the dense kernels + rails_topk wherever it was measured -- are gone;
 * 8: rails_mol_score_dense_upper[_supported] and rails_mol_index_rows_* / rails_mol_score_indexed_rows are new, rails_rescore_select gained one_sided;
 * 9: rails_candidates_* -- the threshold selection and the fused finish of the proved exact top-k -- and rails_merge_candidates_verdict
 * are new, rails_mol_score_indexed_rows gained cand_counts, the component table became item-group-major (rails_mol_component_build
 * gained n_total / first_item, rails_mol_component_topk its out_of_range flag, rails_mol_component_topk_capacity is new);
 * 10: rails_topk_candidates_filtered, rails_rerank_topk_filtered / rails_rerank_workspace_bytes and rails_mol_coarse_topk_capacity are new;
 * 11: the SASRec encoder entries rails_sasrec_* and rails_gemm_f32_id_masked are new, rails_gemm_f32 gained act 2 (relu) / 3 (gelu);
 * 12: the HSTU cached-decoding entries rails_hstu_decode[_supported] and struct rails_hstu_decode_layer are new;
 * 13: the SASRec cached-decoding entries rails_sasrec_decode[_supported] / rails_sasrec_decode_workspace_floats and struct
 * rails_sasrec_decode_layer are new;
 * 14: the IVF-Flat component index rails_ivf_* (MoLNaiveTopK use_faiss=True) is new;
 * 15: the shape-generic fp32 scoring route rails_mol_generic_* is new; the candidate-key entry points rails_group_keys_* of the item-sharded
 * MoLNaiveTopK / MoLCombTopK, the list edit rails_ivf_lists_edit[_workspace_bytes] of the IVF index, the item masks rails_item_mask_* /
 * rails_scores_mask, the hidden-item entries rails_item_mask_clear / rails_mol_coarse_topk_visible / rails_mol_component_topk_visible and the
 * item-tag entries rails_item_tags_effective / rails_item_tags_count / rails_item_mask_from_tags / rails_scores_mask_tags / rails_mol_coarse_topk_tagged /
 * rails_mol_component_topk_tagged / rails_mol_scan_plan and the filtered-list entries rails_ivf_list_words / rails_ivf_list_counts /
 * rails_ivf_plan_filtered / rails_ivf_search_filtered and the group-collapse entries rails_topk_collapse / rails_scores_group_max / rails_topk_keys
 * (and their quota forms rails_topk_collapse_quota / rails_scores_group_next)
 * and the generic route's candidate entries rails_mol_generic_score_indexed / rails_mol_generic_table_width / rails_mol_generic_coarse_build /
 * rails_mol_generic_coarse_update / rails_mol_generic_component_build / rails_mol_generic_component_update / rails_mol_generic_eq_pad
 * and the rank entries rails_scores_rank_keys / rails_scores_rank / rails_item_mask_clear_rows
 * and the softmax entries rails_scores_lse[_workspace_bytes] / rails_scores_log_prob / rails_scores_gumbel
 * and the range-search entries rails_scores_range_workspace_bytes / rails_scores_range_count / _write / _sort / _decode
 * and the query-fusion entries rails_scores_fuse_rows / rails_topk_fuse_lists / rails_lists_union
 * and the multi-row SASRec decode step rails_sasrec_decode_rows / RAILS_SASREC_DECODE_MAX_ROWS (rails_sasrec_decode is its max_new = 1 call,
 * bit for bit what it was)
 * and the diversity entries rails_topk_mmr / rails_topk_mmr_workspace_bytes
 * and the multi-row HSTU decode step rails_hstu_decode_rows[_supported] / rails_hstu_decode_rows_workspace_floats /
 * RAILS_HSTU_DECODE_MAX_ROWS (rails_hstu_decode is what it was)
 * and the pair-level entries rails_mol_generic_explain / rails_mol_generic_explain_indexed / rails_scores_at_eligible / rails_mips_score_indexed
 * and the backward entries rails_mol_generic_pair_backward[_supported / _workspace_bytes] / rails_mol_generic_pack_gate_weights_t /
 * rails_mol_generic_gate_pack_t_floats
 * were added under 15 as well: no struct
 * and no existing entry point changed, so callers built against the earlier header of 15 stay valid).  A binding checks rails_abi_version() == RAILS_ABI_VERSION at load time: callers built
 * against an older header pass shorter structs, and the library would read the new fields from whatever follows them. */
#define RAILS_ABI_VERSION 15
int rails_abi_version(void);

#define RAILS_OK 0
#define RAILS_EINVAL (-22)       /* bad argument (null pointer, non-positive size, k > n ...) */
#define RAILS_ENOTSUP (-95)      /* shape / option outside what the HIP kernels implement */
#define RAILS_ENOMEM (-12)       /* caller-provided workspace too small */
#define RAILS_ELAUNCH (-5)       /* HIP launch failure (message carries hipGetErrorString) */

#define RAILS_GEGLU 0
#define RAILS_SWIGLU 1

/* rails_mol_shape.precision -- the arithmetic of the fused scoring pass and, with it, the FORMAT of the three packed
 * buffers (gate pack, query pack, item index); every buffer must be built and used with the same value.
 *   RAILS_PRECISION_FP32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 fragments.  The parity path and the default.
 *   RAILS_PRECISION_F16X3  every operand of the three contractions is stored as f16 hi + f16 lo (same bytes as the fp32
 *                          fragment it replaces) and every product block costs three f16 MFMAs (lo*hi, hi*lo, hi*hi),
 *                          fp32 accumulate: ~22 significant bits per product, same 1e-4 logit bar, ~3-4x the speed.
 *                          The item index then holds Ex to 22 bits (rails_mol_index_unpack returns hi + lo);
 *                          rails_mol_coarse_build / rails_mol_component_build take an fp32-format index only.
 *   RAILS_PRECISION_F16X1  the F16X3 buffers (same format, interchangeable) scored with the hi * hi product only: plain f16
 *                          operands, fp32 accumulate, 1.6x the speed of F16X3, logits ~1e-2 off (NOT within the 1e-4 bar).
 *                          It exists as the first pass of a speculate-then-verify top-k whose candidates are re-scored in
 *                          fp32 (rails_rescore_select; rails_amd precision "f16-exact"), not as a result-producing mode. */
#define RAILS_PRECISION_FP32 0
#define RAILS_PRECISION_F16X3 1
#define RAILS_PRECISION_F16X1 2

/* rails_mol_shape.gating_combination: how the three gate parts become mixture weights (MoLGatingFn.forward).
 *   GLU_SILU  g = gq * gi + gqi;  w = g * sigmoid(g)      (every shipped config; needs all three parts)
 *   NONE      w = [gq] + [gi] + gqi                        (absent parts contribute nothing); exact-fp32 precision only */
#define RAILS_COMBINE_GLU_SILU 0
#define RAILS_COMBINE_NONE 1
#define RAILS_MAX_UID_TABLES 4

/* Hyper-parameters of one MoL module; field names follow create_mol_interaction_module
 * (modeling/similarity_utils.py:42-70). */
typedef struct rails_mol_shape {
  int32_t query_embedding_dim;
  int32_t item_embedding_dim;
  int32_t dot_product_dimension;      /* d */
  int32_t query_dot_product_groups;   /* P_Q */
  int32_t item_dot_product_groups;    /* P_X */
  int32_t query_hidden_dim;           /* GLU width of the query projection (512); <= 0: plain Linear (similarity_utils.py:108-116) */
  int32_t gating_query_hidden_dim;    /* 128 */
  int32_t gating_item_hidden_dim;     /* 128 */
  int32_t gating_qi_hidden_dim;       /* 128 */
  int32_t query_nonlinearity;         /* RAILS_GEGLU | RAILS_SWIGLU */
  int32_t num_uid_tables;             /* len(uid_embedding_hash_sizes) */
  int32_t dot_product_l2_norm;        /* 0 | 1 */
  float temperature;                  /* 0.05 */
  float eps;                          /* 1e-6 */
  int32_t precision;                  /* RAILS_PRECISION_FP32 | RAILS_PRECISION_F16X3 | RAILS_PRECISION_F16X1 */
  int32_t item_hidden_dim;            /* > 0: the item projection has a GLU hidden layer of this width (similarity_utils.py:127-143) */
  int32_t item_nonlinearity;          /* RAILS_GEGLU | RAILS_SWIGLU, used when item_hidden_dim > 0 */
  int32_t gating_combination;         /* RAILS_COMBINE_GLU_SILU | RAILS_COMBINE_NONE (similarity_fn.py:175-197) */
  int32_t gating_has_query;           /* 0: no query-only gate part (gating_query_fn = False); only with RAILS_COMBINE_NONE */
  int32_t gating_has_item;            /* 0: no item-only gate part  (gating_item_fn = False);  only with RAILS_COMBINE_NONE */
} rails_mol_shape;

/* Raw module weights, one pointer per state_dict() tensor (SURVEY.md section 8b lists the keys). */
typedef struct rails_mol_weights {
  const float* q_glu_w;   /* _query_embeddings_fn._query_emb_proj_module.1._w   (D_q, 2*query_hidden); NULL if query_hidden_dim <= 0 */
  const float* q_glu_b;   /* ...1._b                                            (2*query_hidden)      */
  const float* q_proj_w;  /* ...2.weight  (d*(P_Q-u), query_hidden);  query_hidden_dim <= 0: ...1.weight (d*(P_Q-u), D_q) */
  const float* q_proj_b;  /* ...2.bias / ...1.bias                                                    */
  const float* uid_table[RAILS_MAX_UID_TABLES];  /* _uid_embeddings_{i}.weight   (hash_i + 1, d)       */
  int64_t uid_hash_size[RAILS_MAX_UID_TABLES];
  const float* i_proj_w;  /* _item_embeddings_fn._item_emb_proj_module.1.weight  (P_X*d, D_i)         */
  const float* i_proj_b;
  const float* gq_w1;     /* _gating_fn._query_only_partial_module.0.weight      (H_q, D_q)           */
  const float* gq_b1;
  const float* gq_w2;     /* ...2.weight                                          (L, H_q)            */
  const float* gi_w1;     /* _gating_fn._item_only_partial_module.1.weight       (H_i, D_i)           */
  const float* gi_b1;
  const float* gi_w2;     /* ...3.weight                                          (L, H_i)            */
  const float* gqi_w1;    /* _gating_fn._qi_partial_module.1.weight              (H, L); gating_qi_hidden_dim <= 0 (pair gate without hidden
                           * layer, similarity_utils.py:199-206): the single Linear's (L, L) weight, gqi_b1 its (L) bias, gqi_w2 / gqi_b2 NULL */
  const float* gqi_b1;
  const float* gqi_w2;    /* ...3.weight                                          (L, H)              */
  const float* gqi_b2;
  const float* i_glu_w;   /* item_hidden_dim > 0: _item_embeddings_fn._item_emb_proj_module.1._w (D_i, 2*item_hidden); then      */
  const float* i_glu_b;   /* ...1._b, and i_proj_w / i_proj_b are ...2.weight (P_X*d, item_hidden) / ...2.bias; else NULL  */
} rails_mol_weights;

/* Thread-local message of the last failed call ("" if none). */
const char* rails_last_error(void);

/* Library / device probe: number of compute units of the current device (256 on MI355X), or < 0. */
int rails_device_compute_units(void);

/* 1 if the fused scoring kernel is compiled for this shape, else 0 (rails_last_error() says why). */
int rails_mol_shape_supported(const rails_mol_shape* shape);

/* ---- index build -----------------------------------------------------------------------------
 * Replaces what MoLTopKModule.__init__ (rails/indexing/mol_top_k.py:29-81) keeps per corpus, plus the
 * item-side work the reference redoes on every forward: RecoMoLItemEmbeddingsFn.forward
 * (rails/similarities/mol/item_embeddings_fns.py:149-183) and the item-only gate
 * (rails/similarities/mol/similarity_fn.py:170-171). */

/* fp32 count of the packed pair-gate weights. */
size_t rails_mol_gate_pack_floats(const rails_mol_shape* shape);
/* Permute the pair-gate MLP (gqi_*) into MFMA fragment order. */
int rails_mol_pack_gate_weights(const rails_mol_shape* shape, const rails_mol_weights* w, float* gate_pack,
                                void* stream);

/* fp32 count of the item index for n_items items (tiles of 32 items, last tile zero padded). */
size_t rails_mol_index_floats(const rails_mol_shape* shape, int64_t n_items);
/* items: (n_items, D_i) row-major.  Writes component embeddings Ex (l2-normalised) and the item gate gi
 * of every item into `index` in tile/fragment order. */
int rails_mol_index_build(const rails_mol_shape* shape, const rails_mol_weights* w, const float* items,
                          int64_t n_items, float* index, void* stream);
/* In-place update of an existing index of n_items items (added under ABI 15: no struct and no existing entry point changed): item j of
 * `items` (n_new, D_i) is built and stored at slot positions[j] (int64, device memory) -- rails_mol_index_build's kernel with scatter stores,
 * one launch, no temporary index; fp32 fragments or, under a split precision, the f16 hi / lo halves.  An item's values do not depend on its
 * slot or its neighbours: the index equals the one rails_mol_index_build makes of the updated table, bit for bit.  positions must be unique
 * and inside [0, n_items) (the caller checks; a position outside is skipped, duplicates leave either item).  Touches n_new items' bytes only.
 * To append, grow the buffer to rails_mol_index_floats(n_items + n_new) (old bytes copied, the rest zero) and update the new positions. */
int rails_mol_index_update(const rails_mol_shape* shape, const rails_mol_weights* w, const float* items, int64_t n_new, const int64_t* positions,
                           float* index, int64_t n_items, void* stream);
/* Inverse view for accessors/tests: plain Ex (n_items, P_X, d) and/or gi (n_items, L); either may be NULL.
 * Mirrors MoLSimilarity.get_item_component_embeddings (similarity_fn.py:294-339). */
int rails_mol_index_unpack(const rails_mol_shape* shape, const float* index, int64_t n_items, float* ex_out,
                           float* gi_out, void* stream);
/* Gather rows of an index into a new tile-packed index: out tile layout over `n_rows * n_cand` items
 * taken at cand_idx[r * n_cand + j] (positions in `index`, int64).  n_cand must be a multiple of 32.
 * Replaces self._item_embeddings[idx] (mol_top_k.py:361-363) for the rerank pass. */
int rails_mol_index_gather(const rails_mol_shape* shape, const float* index, int64_t n_items,
                           const int64_t* cand_idx, int64_t n_rows, int64_t n_cand, float* out_index,
                           void* stream);

/* ---- query side ------------------------------------------------------------------------------
 * Replaces RecoMoLQueryEmbeddingsFn.forward (rails/similarities/mol/query_embeddings_fns.py:175-254,
 * GLU at rails/similarities/layers.py:19-74) and the query-only gate (similarity_fn.py:166-169). */
/* Floats of the query pack: Eq fragments of ceil(batch / (32/P_Q)) query groups, gq fragments of `batch` rows, and the
 * prologue's own scratch (GLU output, first gate layer, raw projection and raw gate of ceil(batch/32)*32 rows). */
size_t rails_mol_query_pack_floats(const rails_mol_shape* shape, int32_t batch);
/* queries: (batch, D_q); user_ids: (batch) int64 or NULL when num_uid_tables == 0.
 * eq_out (batch, P_Q, d) and gq_out (batch, L) are optional plain copies (NULL to skip). */
int rails_mol_query_prologue(const rails_mol_shape* shape, const rails_mol_weights* w, const float* queries,
                             const int64_t* user_ids, int32_t batch, float* query_pack, float* eq_out,
                             float* gq_out, void* stream);
/* The same launch(es), writing the pack TWICE: query_pack in shape->precision's format and query_pack_other in the other
 * one (fp32 fragments <-> f16 hi/lo fragments; same values, rails_mol_query_pack_floats floats each).  For callers that score
 * one batch in two precisions (the verified fast modes: f16 first pass, fp32 re-scoring of the candidates). */
int rails_mol_query_prologue_both(const rails_mol_shape* shape, const rails_mol_weights* w, const float* queries,
                                  const int64_t* user_ids, int32_t batch, float* query_pack, float* query_pack_other,
                                  void* stream);

/* ---- scoring ---------------------------------------------------------------------------------
 * Replaces MoLSimilarity.forward for the shared-corpus case (similarity_fn.py:341-413, B' == 1):
 * logits[b * ld + x] for b < batch, x < n_items. */
int rails_mol_score_dense(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack,
                          int32_t batch, const float* index, int64_t n_items, float* logits, int64_t ld,
                          const int32_t* run_if, void* stream);
/* The first pass of the proved exact top-k with a PER-PAIR error bound (no counterpart in the reference, which scores every item in one
 * precision: rails/indexing/mol_top_k.py:99-130): precision F16X3 only; logits[b * ld + x] = s + (ub2 c + ub1) c + ub0 with s the f16x3 logit
 * rails_mol_score_dense writes and c = max_l |cl_l| over the pair's P_Q * P_X cross logits as the kernel computed them.  With the
 * coefficients of rails_amd/f16x3_bound.py upper_bound_poly (>= 0, finite) the value is an UPPER BOUND of the pair's fp32-kernel logit: the
 * bound on |f16x3 - fp32| is quadratic in the magnitude of the cross logits, and the a-priori |cl| <= 1/tau it is otherwise evaluated at is
 * 2-3 x what the pairs of a corpus reach (config 4: one eps = 3.0 for every pair needs > 60 000 candidates per query at 12.5 M items, the
 * per-pair bound 730-900).  Built for the f16x3 kernels of the BASELINE shapes (the 256-logit team kernel and the 8-wave register-resident units);
 * rails_mol_score_dense_upper_supported says whether a shape has it. */
int rails_mol_score_dense_upper_supported(const rails_mol_shape* shape);
int rails_mol_score_dense_upper(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                int64_t n_items, float ub2, float ub1, float ub0, float* logits, int64_t ld, const int32_t* run_if, void* stream);
/* Per-row candidates (B' == B branch, similarity_fn.py:397-402): `cand_index` was produced by
 * rails_mol_index_gather with n_rows == batch; logits[b * ld + j] for j < n_cand. */
int rails_mol_score_candidates(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack,
                               int32_t batch, const float* cand_index, int64_t n_cand, float* logits,
                               int64_t ld, void* stream);
/* ---- The shape-generic scoring route: runtime-shape exact-fp32 kernels for the MoL shapes rails_mol_shape_supported refuses.
 * Envelope: precision RAILS_PRECISION_FP32, a pair gate with a hidden layer (1 <= gating_qi_hidden_dim <= 512),
 * P_Q * P_X <= 256, dot_product_dimension <= 256, and whatever the query prologue (64 KiB of LDS) and the index build (160 KiB)
 * take; every variant axis of the fused route (GLU / Linear projections, uid tables, both gating combinations, l2 norm on / off).
 * The route has its own packs (row-major, see rails_amd/csrc/mol_generic.h): a generic index, query pack or gate pack is not
 * interchangeable with the fused route's.  Eq, Ex, gq and gi are computed by the fused route's own prologue / index-build
 * arithmetic.  A pair's logit has the same bits whatever the batch, the row, the item position, n_items, and whether
 * rails_mol_generic_score_dense or rails_mol_generic_score_candidates scored it.  A shape the fused route supports is accepted too
 * (the caller decides the route; the two routes agree to rounding, not bit for bit).
 * rails_mol_generic_supported and the three size helpers answer without a device. */
int rails_mol_generic_supported(const rails_mol_shape* shape);
size_t rails_mol_generic_gate_pack_floats(const rails_mol_shape* shape);
size_t rails_mol_generic_index_floats(const rails_mol_shape* shape, int64_t n_items);   /* whole tiles of 32 items, stored back to back */
size_t rails_mol_generic_query_pack_floats(const rails_mol_shape* shape, int32_t batch);
int rails_mol_generic_pack_gate_weights(const rails_mol_shape* shape, const rails_mol_weights* w, float* gate_pack, void* stream);
int rails_mol_generic_index_build(const rails_mol_shape* shape, const rails_mol_weights* w, const float* items, int64_t n_items, float* index,
                                  void* stream);
/* rails_mol_index_clear_tail for the generic route's row-major index (rows n_items .. end of the last tile) */
int rails_mol_generic_index_clear_tail(const rails_mol_shape* shape, float* index, int64_t n_items, void* stream);
/* rails_mol_index_update for the generic route's row-major index */
int rails_mol_generic_index_update(const rails_mol_shape* shape, const rails_mol_weights* w, const float* items, int64_t n_new, const int64_t* positions,
                                   float* index, int64_t n_items, void* stream);
int rails_mol_generic_index_unpack(const rails_mol_shape* shape, const float* index, int64_t n_items, float* ex_out, float* gi_out, void* stream);
int rails_mol_generic_query_prologue(const rails_mol_shape* shape, const rails_mol_weights* w, const float* queries, const int64_t* user_ids,
                                     int32_t batch, float* query_pack, float* eq_out, float* gq_out, void* stream);
/* logits[b * ld + x] for x < n_items; run_if as in rails_mol_score_dense */
int rails_mol_generic_score_dense(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                  int64_t n_items, float* logits, int64_t ld, const int32_t* run_if, void* stream);
/* per-row candidates: candidate j of row b is item b * n_cand + j of `cand_index` (a generic index of batch * n_cand items; any n_cand) */
int rails_mol_generic_score_candidates(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch,
                                       const float* cand_index, int64_t n_cand, float* logits, int64_t ld, const int32_t* run_if, void* stream);
/* per-row candidates scored IN PLACE on the shared generic index (rails_mol_score_indexed / rails_mol_score_indexed_rows for this route; the
 * index is row-major already): candidate j of row b is item positions[b * n_cand + j] of `index`, clamped into [0, n_items); any n_cand >= 1.
 * counts: NULL, or per-row live counts (int32 on the device): only logits[b * ld + j] for j < counts[b] are written, tiles of 32 candidates
 * past the count are skipped.  A pair's logit has the bits rails_mol_generic_score_dense gives it. */
int rails_mol_generic_score_indexed(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                                    int64_t n_items, const int64_t* positions, int64_t n_cand, const int32_t* counts, float* logits, int64_t ld,
                                    const int32_t* run_if, void* stream);
/* The explaining launches (score_of / explain_of): rails_mol_generic_score_candidates / rails_mol_generic_score_indexed
 * that also store, per pair, the L = P_Q * P_X cross logits after the division by tau (component_logits[(b * n_cand + j) * L + l], l = p * P_X +
 * m) and the L mixture weights the reference's combiner returns in eval mode (weights, the same layout; they sum to 1 up to rounding).  The
 * logit of a pair has the bits of every other rails_mol_generic_score_* launch.  Both outputs hold batch * n_cand * L floats.  The indexed form
 * takes no per-row counts: every one of the n_cand slots of a row is scored and written. */
int rails_mol_generic_explain(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch, const float* cand_index,
                              int64_t n_cand, float* logits, int64_t ld, float* component_logits, float* weights, void* stream);
int rails_mol_generic_explain_indexed(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch,
                                      const float* index, int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld,
                                      float* component_logits, float* weights, void* stream);
/* The backward of rails_mol_generic_score_candidates (the differentiable MoLSimilarity.forward): gradients of
 * sum(dy * logits) in eval-mode arithmetic; dy is (batch, n_cand) with leading dimension ld_dy.  The kernels read what the forward reads
 * (gate_pack, query_pack, cand_index) plus gate_pack_t: the two pair-gate matrices transposed, rails_mol_generic_gate_pack_t_floats floats
 * written by rails_mol_generic_pack_gate_weights_t.  Outputs, each optional (NULL: its work is skipped):
 *   d_query_pack  rails_mol_generic_query_pack_floats(batch) floats, the query pack's layout: the gradient of the l2-normalised Eq BEFORE its
 *                 division by tau, and of gq; pads zero
 *   d_cand_index  batch * n_cand rows of the item layout (P_X * dp + Lq floats each, no tile padding): the gradient of Ex and gi; pads zero
 *   dw1 (H, L), db1 (H), dw2 (L, H), db2 (L), row-major, together or not at all: the pair gate's weight gradients.  They are summed through
 *                 `workspace` (rails_mol_generic_pair_backward_workspace_bytes(shape, chunk_pairs) bytes, uninitialised; RAILS_ENOMEM if
 *                 shorter): the rows run in chunks of whole rows of at most chunk_pairs pairs (rounded up to 256; a row of more candidates
 *                 is RAILS_EINVAL), so no buffer grows with batch * n_cand.
 * n_cand == 0: d_query_pack and the weight gradients are set to zero.
 * No floating-point atomics: every sum over pairs runs over a fixed partition in a fixed order, so the bits depend on neither the device nor
 * the run.  rails_mol_generic_pair_backward_supported: 1 iff the shape is inside the generic route's envelope and
 * ceil(P_Q / 32) * ceil(d / 32) <= 4 (the dEq accumulators of a row live in registers); answered without a device. */
int rails_mol_generic_pair_backward_supported(const rails_mol_shape* shape);
size_t rails_mol_generic_gate_pack_t_floats(const rails_mol_shape* shape);
int rails_mol_generic_pack_gate_weights_t(const rails_mol_shape* shape, const rails_mol_weights* weights, float* gate_pack_t, void* stream);
size_t rails_mol_generic_pair_backward_workspace_bytes(const rails_mol_shape* shape, int64_t chunk_pairs);
int rails_mol_generic_pair_backward(const rails_mol_shape* shape, const float* gate_pack, const float* gate_pack_t, const float* query_pack,
                                    int32_t batch, const float* cand_index, int64_t n_cand, const float* dy, int64_t ld_dy, float* d_query_pack,
                                    float* d_cand_index, float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes,
                                    int64_t chunk_pairs, void* stream);
/* The bf16 candidate tables of the two-pass algorithms from the generic index.  rails_mol_generic_table_width: the smallest of 32 / 64 / 128
 * that is >= dot_product_dimension, 0 for d > 128 (no table; answered without a device).  Rows have that many columns, the columns d .. width
 * exact zeros; the real columns carry rails_mol_coarse_build's / rails_mol_component_build's arithmetic, operation for operation.  The coarse
 * table is (n_items, width), the component table item-group-major (P_X, n_items, width); the scans rails_mol_coarse_* / rails_mol_component_*
 * run on them under a copy of the shape with dot_product_dimension = width, Eq padded alike (rails_mol_generic_eq_pad: (rows, d) fp32 ->
 * (rows, width), zeros behind; rows = batch * P_Q).  The update forms rewrite rows positions[0 .. n_new) (those outside [0, n_items) are
 * skipped) of a table of n_items rows from the index, which holds the new items already. */
int32_t rails_mol_generic_table_width(const rails_mol_shape* shape);
int rails_mol_generic_coarse_build(const rails_mol_shape* shape, const float* index, int64_t n_items, void* table, void* stream);
int rails_mol_generic_coarse_update(const rails_mol_shape* shape, const float* index, const int64_t* positions, int64_t n_new, void* table,
                                    int64_t n_items, void* stream);
int rails_mol_generic_component_build(const rails_mol_shape* shape, const float* index, int64_t n_items, void* table, void* stream);
int rails_mol_generic_component_update(const rails_mol_shape* shape, const float* index, const int64_t* positions, int64_t n_new, void* table,
                                       int64_t n_items, void* stream);
int rails_mol_generic_eq_pad(const rails_mol_shape* shape, const float* eq, int64_t rows, float* out, void* stream);
/* Per-row candidates scored IN PLACE: logits[b][j] = MoL(query b, item positions[b][j]) with the item operands read straight from the
 * shared index -- rails_mol_index_gather + rails_mol_score_candidates without the gathered copy and its launch (same arithmetic per
 * pair, same bits).  Exact-fp32 shapes on the independent-wave shell (rails_mol_score_indexed_supported != 0); the 256-logit shape
 * and the f16 precisions gather.  positions must lie in [0, n_items) (they are clamped, not masked); any n_cand >= 1. */
int rails_mol_score_indexed_supported(const rails_mol_shape* shape, int32_t batch, int64_t n_cand);
/* The same re-scoring from a ROW-MAJOR copy of the fp32 index: rails_mol_index_rows_build writes item i's operands as rails_mol_index_rows_floats /
 * n_items consecutive floats (fragment slot s, lane half h as float4 number 2 s + h of the row), so that a candidate's bytes are fetched in
 * whole cache lines -- in the tile-packed index each 16-byte piece of a candidate lies in a line of its own (8 x the bytes; amzn-books, 32 x 1 024
 * candidates: 47 -> 24 us; 32 x 10 272: the whole step 3.67 -> 3.34 ms).  Same values in the same order: the logits are bit-identical to rails_mol_score_indexed's.  Shapes and sizes where
 * rails_mol_score_indexed_supported holds; exact-fp32 precision.  One more copy of the index in memory (optional: callers that cannot afford it
 * use rails_mol_score_indexed). */
size_t rails_mol_index_rows_floats(const rails_mol_shape* shape, int64_t n_items);
int rails_mol_index_rows_build(const rails_mol_shape* shape, const float* index, int64_t n_items, float* index_rows, void* stream);
/* An index that was CUT to n_items items (its first rails_mol_index_floats(shape, n_items) floats kept): the slots n_items .. end of the last tile
 * are set to zero, what rails_mol_index_build leaves there -- the cut index is then the bytes of a fresh build of its first n_items items.  Either
 * index format (fp32, split-f16); touches one tile; nothing to do when n_items is a multiple of 32.  The row-major copy has no padding. */
int rails_mol_index_clear_tail(const rails_mol_shape* shape, float* index, int64_t n_items, void* stream);
/* The rows of n_new positions copied again from the (already updated) index; nothing else is read or written. */
int rails_mol_index_rows_update(const rails_mol_shape* shape, const float* index, int64_t n_items, const int64_t* positions, int64_t n_new,
                                float* index_rows, void* stream);
/* cand_counts (optional, may be NULL): row b has cand_counts[b] <= n_cand candidates (rails_candidates_select's counts): only logits[b][0 .. cand_counts[b])
 * are written, the tiles past them are skipped. */
int rails_mol_score_indexed_rows(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch, const float* index_rows,
                                 int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld, const int32_t* cand_counts,
                                 void* stream);
int rails_mol_score_indexed(const rails_mol_shape* shape, const float* gate_pack, const float* query_pack, int32_t batch, const float* index,
                            int64_t n_items, const int64_t* positions, int64_t n_cand, float* logits, int64_t ld, void* stream);

/* ---- dot-product (MIPS) scoring ---------------------------------------------------------------
 * Replaces torch.mm(query_embeddings, item_embeddings_t) of MIPSBruteForceTopK.forward
 * (rails/indexing/mips_top_k.py:56-81) and of DotProductSimilarity.forward
 * (rails/similarities/dot_product_similarity_fn.py:48-54).  fp32. */
size_t rails_mips_index_floats(int32_t dim, int64_t n_items);          /* tile-packed copy of the (n, dim) table */
int rails_mips_index_build(const float* items, int64_t n_items, int32_t dim, float* index, void* stream);
/* In-place changes of a built index (additions under ABI 15).  rails_mips_index_update: rails_mips_index_build's stores with scatter addressing --
 * item j of `items` (n_new, dim) goes to slot positions[j] (int64, device memory, unique) of an index of n_items items; a position outside
 * [0, n_items) is skipped.  No arithmetic: the slot holds the bytes a fresh build of the changed table holds.  rails_mips_index_gather_rows: the
 * inverse read, rows (n_rows, dim) = the items at `positions` as the index holds them (a position outside the index reads zeros).
 * rails_mips_index_clear_tail: as rails_mol_index_clear_tail, for an index cut to n_items items. */
int rails_mips_index_update(const float* items, int64_t n_new, int32_t dim, const int64_t* positions, float* index, int64_t n_items, void* stream);
int rails_mips_index_gather_rows(const float* index, int64_t n_items, int32_t dim, const int64_t* positions, int64_t n_rows, float* rows, void* stream);
int rails_mips_index_clear_tail(float* index, int64_t n_items, int32_t dim, void* stream);
size_t rails_mips_query_ws_floats(int32_t dim, int32_t batch);         /* scratch for the packed queries */
/* rails_mips_score for per-row candidates read in place: logits[b * ld + j] = <queries[b], item positions[b * n_cand + j]> with the bits
 * rails_mips_score gives that pair (the same MFMA chain; the item operand is fetched by position).  Positions outside [0, n_items) are clamped
 * into it (the caller overwrites their entries).  query_ws as rails_mips_score. */
int rails_mips_score_indexed(const float* queries, int32_t batch, int32_t dim, const float* index, int64_t n_items, const int64_t* positions,
                             int64_t n_cand, float* query_ws, float* logits, int64_t ld, void* stream);
int rails_mips_score(const float* queries, int32_t batch, int32_t dim, const float* index, int64_t n_items,
                     float* query_ws, float* logits, int64_t ld, void* stream);

/* ---- item id -> position map (additions under ABI 15) ------------------------------------------
 * What lets a caller address the corpus of a top-k module by item id (positions_of, update_items_by_id, remove_items_by_id, upsert_items).
 * An open-addressing table with linear probing in device memory: int64 keys[slots], then int32 values[slots]; slots a power of two.
 * INT64_MIN marks an EMPTY slot and INT64_MIN + 1 an ERASED one (a tombstone; an insert never reuses it): both are reserved, an id equal to
 * either is counted and not stored.  The home slot of an id is mix(id) & (slots - 1), mix the splitmix64 step of the hashed item tables
 * below, on the id as an unsigned 64-bit word (arithmetic mod 2^64):
 *   z = id + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  mix = z ^ (z >> 31)
 * -- a bijection (odd multipliers, xor-shifts).  One thread per id; every probe loop ends within `slots` steps.  Which key lands in which
 * slot depends on the order the atomic claims win in: the contract is on lookups, not on the table's bytes.
 * slots: the smallest power of two >= 4 * max(n_items, 1), so a fresh table has load <= 1/4; RAILS_EINVAL for n_items < 0 or >= 2^31 (values
 *   are int32 positions).  bytes: 12 * slots; 0 when slots is not a power of two in [1, 2^33].
 * clear: every slot EMPTY.
 * insert: ids[u] (int64, device) -> positions[u] (int64, device), or first + u when positions is NULL.  flags (3 x int32, device, ADDED to):
 *   [0] ids already in the table or given twice in the call (the table keeps one entry), [1] reserved ids or positions outside [0, 2^31),
 *   [2] inserts that found no slot in a full table.
 * erase: the key becomes ERASED; *missing (int32, device, ADDED to) counts the ids that were absent (or given a second time).
 * lookup: positions_out[u] (int64, device) = the position of ids[u], -1 where absent.
 * All four return RAILS_EINVAL before any launch for a NULL pointer, slots not a power of two, m < 0 or first + m > 2^31; m = 0 is a no-op. */
int64_t rails_id_map_slots(int64_t n_items);
size_t rails_id_map_bytes(int64_t slots);
int rails_id_map_clear(void* map, int64_t slots, void* stream);
int rails_id_map_insert(void* map, int64_t slots, const int64_t* ids, const int64_t* positions, int64_t first, int64_t m, int32_t* flags, void* stream);
int rails_id_map_erase(void* map, int64_t slots, const int64_t* ids, int64_t m, int32_t* missing, void* stream);
int rails_id_map_lookup(const void* map, int64_t slots, const int64_t* ids, int64_t m, int64_t* positions_out, void* stream);

/* ---- item masks: a top-k call restricted to a subset of the corpus (added under ABI 15: new entries only) -----------------------
 * No counterpart in the reference: CandidateIndex.apply_object_filter ("general per batch filters", indexing/candidate_index.py) raises
 * NotImplementedError there.  A mask is `rows` rows of rails_item_mask_words of n 32-bit words; bit i % 32 of word i / 32 of a row is
 * item i (1 = the item may be returned) and the unused high bits of a row's last word are zero.  1 <= n < 2^31, 1 <= rows <= 2^24. */
int64_t rails_item_mask_words(int64_t n);                 /* ceil(n / 32) */
int64_t rails_item_mask_tile_items(void);                 /* items per tile of the compaction below (8 192) */
/* mask_u8 (rows, n) bool bytes with row stride ld (non-zero = set) -> words (rows, words-of-n), every word written, and counts[r] = set
 * bits of row r.  One wave ballot per 64 items; two launches. */
int rails_item_mask_pack(const uint8_t* mask_u8, int64_t ld, int32_t rows, int64_t n, uint32_t* words, int32_t* counts, void* stream);
/* ONE row, zeroed by the caller: the bits at positions[0 .. m) are set (a 32-bit atomic OR each; repeats are harmless).  The caller
 * checks the positions against [0, n) beforehand; the kernel skips one outside it. */
int rails_item_mask_set(const int64_t* positions, int64_t m, int64_t n, uint32_t* words, void* stream);
/* The counterpart (added under ABI 15): the bits at positions[0 .. m) of ONE row are cleared (a 32-bit atomic AND-NOT each; repeats are
 * harmless), every other bit stays.  What hide_items does to a module's visibility row. */
int rails_item_mask_clear(const int64_t* positions, int64_t m, int64_t n, uint32_t* words, void* stream);
/* counts[r] = set bits of row r among its first n */
int rails_item_mask_count(const uint32_t* words, int32_t rows, int64_t n, int32_t* counts, void* stream);
/* Stable compaction: out[r * out_ld + j] = the j-th set position of row r, ascending, for j < counts[r]; the slots from counts[r] to
 * out_ld hold 0; set positions beyond out_ld are dropped (the caller passes out_ld >= the largest count).  Per-tile popcounts, an
 * exclusive 64-bit scan of every row's tile counts, the write, the padding: four launches, rows of any length.  `workspace`:
 * rails_item_mask_positions_workspace_bytes bytes, uninitialised. */
size_t rails_item_mask_positions_workspace_bytes(int32_t rows, int64_t n);
int rails_item_mask_positions(const uint32_t* words, int32_t rows, int64_t n, int64_t* out, int64_t out_ld, void* workspace, size_t workspace_bytes,
                              void* stream);
/* In place: scores[b * ld + x] = fill for x < n wherever bit first_item + x of row b's mask is clear (row b of the mask starts at
 * words + b * words_row_stride; words_row_stride = 0: one row shared by every b).  The mask rows hold at least first_item + n bits.
 * Entries whose bit is set are neither read nor written: their bits stay, NaN payloads included.  run_if: the launch predicate. */
int rails_scores_mask(float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const uint32_t* words, int64_t words_row_stride,
                      float fill, const int32_t* run_if, void* stream);

/* ---- item tags (added under ABI 15; no counterpart in the reference) ------------------------------
 * One 32-bit word of attributes per item, bit j = the item carries attribute j; a call carries one ALLOW word per query row (or one for the
 * whole batch) and row b may return item x iff tags[x] & allowed[b] != 0.  Every kernel reads the EFFECTIVE tags: the word of a hidden
 * item is 0, so a hidden item matches no word.  All arrays live in device memory. */
/* eff_out[i] = tags[i] where bit i of the visibility row (rails_item_mask_words(n) words, bit set = visible) is set, else 0. */
int rails_item_tags_effective(const uint32_t* tags, const uint32_t* visible_words, int64_t n, uint32_t* eff_out, void* stream);
/* counts_out[j] = the number of items i < n with eff_tags[i] & words[j] != 0, for j < n_words (at most 65 536): how many items each allow
 * word keeps.  One workgroup per word; the caller reads a count back once and keeps it. */
int rails_item_tags_count(const uint32_t* eff_tags, int64_t n, const uint32_t* words, int32_t n_words, int32_t* counts_out, void* stream);
/* The item mask of a tag filter: bit i of row r of words_out (`rows` rows of rails_item_mask_words(n) words, the unused high bits zero) is
 * set iff eff_tags[i] & allowed[r] != 0 -- packed with one wave ballot per 64 items, as rails_item_mask_pack packs bool bytes --, and
 * counts_out[r] = the row's set bits.  What the exact modules hand to their masked strategies. */
int rails_item_mask_from_tags(const uint32_t* eff_tags, int64_t n, const uint32_t* allowed, int32_t rows, uint32_t* words_out, int32_t* counts_out,
                              void* stream);
/* The eligibility pass of the pair-level calls.  scores (rows, t) holds the score of item positions[r * t + j] for row
 * r; in place, scores[r * ld + j] = -inf wherever the position lies outside [0, n) or row r may not return its item:
 *   words      NULL, or mask words as rails_scores_mask takes them (words_row_stride = 0: one row for every r) -- the bit must be set
 *   eff_tags / allowed   both NULL, or the effective tags (n) and one allow word per row (rows) -- eff_tags[p] & allowed[r] must be non-zero
 *   invalid_ids / item_ids   both NULL, or the rows' seen ids (rows, width) and the ids of the n items -- item_ids[p] must not be among row r's
 * extra_a / extra_b: NULL, or two (rows, t, extra_len) fp32 arrays whose extra_len entries of a pair are set to 0 where its score is set to -inf.
 * One thread per pair, no atomics; kept entries are neither read nor written. */
int rails_scores_at_eligible(float* scores, int64_t ld, int32_t rows, int64_t t, const int64_t* positions, int64_t n, const uint32_t* words,
                             int64_t words_row_stride, const uint32_t* eff_tags, const uint32_t* allowed, const int64_t* invalid_ids, int32_t width,
                             const int64_t* item_ids, float* extra_a, float* extra_b, int32_t extra_len, void* stream);
/* rails_scores_mask with the tag test in place of a mask bit.  In place: scores[r * ld + x] = fill for x < n wherever
 * eff_tags[first_item + x] & allowed[r / rows_per_allowed] == 0; kept entries are neither read nor written.  eff_tags holds at least
 * first_item + n words, allowed at least ceil(rows / rows_per_allowed).  rows_per_allowed maps the rows of a matrix with several rows per
 * query (the B * P_Q * P_X rows of the component scores: P_Q * P_X) to batch rows; rows_per_allowed = rows: one word for all.
 * run_if: the launch predicate. */
int rails_scores_mask_tags(float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const uint32_t* eff_tags, const uint32_t* allowed,
                           int32_t rows_per_allowed, float fill, const int32_t* run_if, void* stream);

/* ---- exact ranks of given items (added under ABI 15: new entries only; no counterpart in the reference) ----------------------------
 * The rank of target position x in row r of a (rows, n) fp32 score matrix with row stride ld, among the items the row may return:
 *   rank = 1 + #{ eligible y : key(r, y) > key(r, x) },   key(r, y) = (orderable(scores[r * ld + y]) << 32) | ~y
 * -- the selection key of rails_topk on the score's bit pattern (+-0, +-inf and NaN payloads rank as they do there; ties break by position
 * ascending), so rank - 1 is the index at which x stands in the row's exhaustive rails_topk list.  Rank 0: "not ranked" -- the target is
 * not a position of the matrix, or its own mask bit is clear.  1 <= t <= 64 targets per row and call, 1 <= rows <= 2^24 (rows = 0: nothing
 * to do), 1 <= n < 2^31, ld >= n. */
/* keys_out[r * t + j] = the key of position p = positions[r * t + j] read from row r, or 0 -- below every real key -- for p outside [0, n)
 * (the -1 of an unknown id). */
int rails_scores_rank_keys(const float* scores, int64_t ld, int32_t rows, int64_t n, const int64_t* positions, int32_t t, uint64_t* keys_out, void* stream);
/* ranks_out[r * t + j] = the rank of the target whose key is keys[r * t + j], every entry written.  mask_words: the item-mask rows of
 * rails_scores_mask (row r at mask_words + r * words_row_stride, words_row_stride = 0: one row shared by every r; otherwise at least
 * rails_item_mask_words(n)), bit set = eligible; NULL: every item is eligible.  Three launches -- zero, count, finish --: the count reads
 * every score once for all t targets of its row and adds integers, so the result does not depend on the order of arrival. */
int rails_scores_rank(const float* scores, int64_t ld, int32_t rows, int64_t n, const uint64_t* keys, int32_t t, const uint32_t* mask_words,
                      int64_t words_row_stride, int32_t* ranks_out, void* stream);
/* rails_item_mask_clear per row: the bits at positions[r * m .. r * m + m) of row r (at words + r * words_row_stride, words_row_stride >=
 * rails_item_mask_words(n)) are cleared, a 32-bit atomic AND-NOT each; positions outside [0, n) are skipped, repeats are harmless.  How a
 * row's seen ids leave its mask.  m = 0 or rows = 0: nothing to do. */
int rails_item_mask_clear_rows(const int64_t* positions, int32_t rows, int64_t m, int64_t n, uint32_t* words, int64_t words_row_stride, void* stream);

/* ---- softmax over the corpus (added under ABI 15: new entries only; no counterpart in the reference) ---------------------------------
 * Over the eligible columns of row r of a (rows, n) fp32 score matrix with row stride ld (mask_words / words_row_stride as in
 * rails_scores_rank: bit set = eligible, NULL = every column), with beta = inv_temperature, a finite fp32 > 0:
 *   y(x) = fl32(x * beta),  Y = y(M) for M the largest eligible x,  S = sum over the eligible x of expf(y(x) - Y),
 *   lse = fl32(Y + log S)  (the log, the add and every sum across lanes and workgroups in float64),  log_prob(x) = fl32(y(x) - lse).
 * Special rows: nothing eligible, or -inf alone -> lse = -inf; any eligible NaN -> NaN; otherwise any eligible +inf -> +inf; an eligible
 * -inf adds 0; one eligible finite entry -> lse = y.  0 <= rows <= 2^24 (rows = 0: nothing to do), 1 <= n < 2^31, ld >= n; rows may start
 * at any 4-byte alignment.  RAILS_EINVAL for a NULL pointer, a size outside these or an inv_temperature that is not a finite number > 0. */
/* lse_out[r], every entry written.  Two reads of the matrix (a row-maximum pass, then the sum with the known Y: no rescaling), per thread
 * an fp32 chain of at most 16 terms, everything above it in float64 in a fixed order, no floating-point atomics: the same bits on every
 * run.  workspace: rails_scores_lse_workspace_bytes(rows, n) bytes, 256-byte aligned (RAILS_ENOMEM if shorter). */
size_t rails_scores_lse_workspace_bytes(int32_t rows, int64_t n);
int rails_scores_lse(const float* scores, int64_t ld, int32_t rows, int64_t n, float inv_temperature, const uint32_t* mask_words, int64_t words_row_stride,
                     void* workspace, size_t workspace_bytes, float* lse_out, void* stream);
/* out[r * t + j] = fl32(y(scores[r * ld + p]) - lse[r]) for p = positions[r * t + j] when p lies inside [0, n) and is eligible, -inf
 * otherwise.  Any t >= 1. */
int rails_scores_log_prob(const float* scores, int64_t ld, int32_t rows, int64_t n, const int64_t* positions, int64_t t, float inv_temperature, const float* lse,
                          const uint32_t* mask_words, int64_t words_row_stride, float* out, void* stream);
/* Gumbel perturbation, out of place: out[r * out_ld + x] = fl32(y(x) + g(seed, first_row + r, x)) for eligible x, -inf for the others
 * (out_ld >= n; out must not overlap scores).  g = -logf(-logf(u)), u = ((w >> 9) + 0.5) * 2^-23 in [2^-24, 1 - 2^-24], w = word 0 of
 * Philox4x32-10 with counter (x, row & 0xFFFFFFFF, row >> 32, 0) and key (seed & 0xFFFFFFFF, seed >> 32), row = first_row + r >= 0: the noise
 * of (seed, row, x) does not depend on how a batch is sliced, on the grid or on the alignment of a row.  The top-k of a perturbed row is a
 * draw without replacement from softmax(scores / temperature) over the row's eligible columns, in draw order. */
int rails_scores_gumbel(const float* scores, int64_t ld, int32_t rows, int64_t n, float inv_temperature, uint64_t seed, int64_t first_row,
                        const uint32_t* mask_words, int64_t words_row_stride, float* out, int64_t out_ld, void* stream);

/* ---- range search over a score matrix (added under ABI 15: new entries only) -----------------------------------------------------------
 * Which columns of row r of a (rows, n) fp32 score matrix with row stride ld meet the row's threshold, as a ragged result.  Column x is a
 * HIT of row r when it is eligible (mask_words / words_row_stride as in rails_scores_rank: bit set = eligible, NULL = every column) and
 *   v >= thresholds[r]    (an IEEE fp32 compare: false when either side is NaN)
 * with v = scores[r * ld + x] when lse is NULL (the score form; inv_temperature is checked and not used) and
 * v = fl32(fl32(scores[r * ld + x] * inv_temperature) - lse[r]) otherwise (the log-probability form: rails_scores_log_prob's value for the
 * lse rails_scores_lse gave; one rounded multiply, not fused with the subtraction).  thresholds: rows fp32 values on the device.
 * No atomics: the same bits on every run, whatever the alignment of a row.  Rows in [1, 2^24], n in [1, 2^31), ld >= n; rows = 0: nothing
 * to do.  RAILS_EINVAL for a NULL pointer, a size outside these, an inv_temperature that is not a finite number > 0 or mask rows shorter
 * than n bits; RAILS_ENOMEM for a workspace shorter than rails_scores_range_workspace_bytes(rows, n) (256-byte aligned); every refusal
 * before any launch. */
size_t rails_scores_range_workspace_bytes(int32_t rows, int64_t n);
/* counts_out[r] = the hits of row r, lims_out[0] = 0, lims_out[r + 1] = lims_out[r] + counts_out[r] (rows + 1 entries).  One read of the
 * matrix.  The workspace keeps the per-slot counts and offsets rails_scores_range_write needs: a row's hits are counted per slot, in
 * position order [the unaligned head | every chunk of 4 096 aligned columns | the unaligned tail], then scanned by one workgroup. */
int rails_scores_range_count(const float* scores, int64_t ld, int32_t rows, int64_t n, const float* thresholds, float inv_temperature, const float* lse,
                             const uint32_t* mask_words, int64_t words_row_stride, void* workspace, size_t workspace_bytes, int64_t* counts_out,
                             int64_t* lims_out, void* stream);
/* After rails_scores_range_count with the same inputs and the workspace it filled: keys_out[lims[r] + j] = the 64-bit selection key
 * ((orderable(score) << 32) | ~position) of row r's j-th hit in POSITION order.  One more read of the matrix.  capacity: the entries of
 * keys_out (lims[rows] are written); every store is tested against it, and against the slot's count -- a pass that disagrees with its
 * count (the inputs changed in between) writes nothing out of bounds and sets the int32 word at the start of the workspace's last 256
 * bytes, which rails_scores_range_count zeroes.  capacity = 0: nothing to do. */
int rails_scores_range_write(const float* scores, int64_t ld, int32_t rows, int64_t n, const float* thresholds, float inv_temperature, const float* lse,
                             const uint32_t* mask_words, int64_t words_row_stride, void* workspace, size_t workspace_bytes, uint64_t* keys_out,
                             int64_t capacity, void* stream);
/* In place: keys[lims[r], lims[r + 1]) sorted descending for every row -- score descending, then position ascending, on the bit pattern: the
 * row's exhaustive top-k order.  max_count: at least the largest row's count; it sizes the launch's LDS, and a row beyond it is left as it
 * is.  RAILS_ENOTSUP for max_count > 16 384; max_count < 2: nothing to do. */
int rails_scores_range_sort(uint64_t* keys, const int64_t* lims, int32_t rows, int32_t max_count, void* stream);
/* scores_out[i] = the score of keys[i] (its bits), ids_out[i] = ids[position] (the position itself when ids is NULL; -1 for a position
 * outside [0, n)), i < total.  total = 0: nothing to do. */
int rails_scores_range_decode(const uint64_t* keys, int64_t total, const int64_t* ids, int64_t n, float* scores_out, int64_t* ids_out, void* stream);

/* ---- query fusion: several sub-query rows per user become one result row (added under ABI 15: new entries only) ---------------------------
 * lims: n_out + 1 int64 values ON THE DEVICE; fused row u owns the input rows [lims[u], lims[u + 1]).  The caller has checked lims[0] = 0,
 * lims[n_out] = rows_in and that it increases strictly; the kernels clamp every segment to [0, rows_in) all the same and read nothing outside
 * it. */
#define RAILS_FUSE_MAX 0
#define RAILS_FUSE_SUM 1
/* out[u * ld_out + x] = the fusion of scores[r * ld + x] over the rows r of segment u, ascending, for x < n:
 *   RAILS_FUSE_MAX   the element whose bit pattern is largest under the order of the selection key (sign-magnitude to unsigned: -0 < +0,
 *                    NaNs by their payload above +inf / below -inf): rails_topk's order, no float compare;  weights must be NULL
 *   RAILS_FUSE_SUM   weights == NULL: acc = s[r0], then acc = fl32(acc + s[r]);
 *                    weights (rows_in fp32): acc = fl32(w[r0] * s[r0]), then acc = fl32(acc + fl32(w[r] * s[r])) -- two roundings per term,
 *                    never an fma, so a float32 loop on the host reproduces it bit for bit
 * A segment of one row without weights is copied.  Every input is read once, every output written once; no atomics, no LDS, no scratch at any
 * segment size.  Rows of any 4-byte alignment: 16-byte loads and stores when scores and out are 16-byte aligned and ld and ld_out multiples of
 * 4, one column per thread otherwise -- the same bits.  run_if: the launch predicate (NULL: run).  0 <= rows_in, n_out <= 2^24, 1 <= n < 2^31,
 * ld >= n, ld_out >= n; n_out = 0: nothing to do.  RAILS_EINVAL for a NULL pointer, a size outside these, an unknown mode, weights with
 * RAILS_FUSE_MAX, or an out that overlaps scores. */
int rails_scores_fuse_rows(const float* scores, int64_t ld, int32_t rows_in, int64_t n, const int64_t* lims, int32_t n_out, int32_t mode, const float* weights,
                           float* out, int64_t ld_out, const int32_t* run_if, void* stream);
/* The merge of RAILS_FUSE_MAX on sorted lists: scores (rows_in, depth) fp32 with row stride ld and positions (rows_in, depth) int64, contiguous
 * -- row r's top-depth list under the selection key.  Per fused row, one workgroup: the entries with a position in [0, n_items) and a score
 * other than -inf (the padding of a short list) are sorted by (position, score), the best entry of every position becomes its selection key,
 * a second sort ranks them, and the first k whose id -- ids[position], the position itself when ids is NULL -- is not among
 * invalid_ids[u * width .. + width) are written to out_ids / out_scores (n_out * k each), the rest of a short row as (-1, -inf).
 * max_segment: at least the largest lims[u + 1] - lims[u]; it sizes the launch's LDS, and a longer segment is cut to it.  Exact for the top k
 * of the fused matrix when depth >= min(k + width, items a row may return) and no two items share an id.
 * RAILS_ENOTSUP (nothing launched) for max_segment * depth > 16 384, k > 512, width > 4 096 or n_items > 2^32 - 1. */
int rails_topk_fuse_lists(const float* scores, int64_t ld, const int64_t* positions, int32_t rows_in, int32_t depth, const int64_t* lims, int32_t n_out,
                          int32_t max_segment, int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids,
                          float* out_scores, void* stream);
/* The union of candidate lists: positions (rows_in, width) int64 with row stride ld -- row r's candidate positions, in any order, duplicates
 * allowed (int64 is what every candidate scan hands over; there is no int32 form).  Per fused row, one workgroup: the entries of its segment
 * with a position in [0, n_items) are sorted in LDS and the first of every run of equal positions is kept: out[u * w_out .. + counts[u]) holds
 * the segment's distinct positions ascending, out[u * w_out + counts[u] .. + w_out) holds -1.  counts (n_out int32) may be NULL.
 * max_segment: at least the largest lims[u + 1] - lims[u]; it sizes the launch's LDS, and a longer segment is cut to it.  One launch, no
 * atomics, no scratch, no host read.  n_out = 0: nothing to do.  RAILS_EINVAL for a NULL pointer, a size below 1 (rows_in, n_out, n_items
 * below 0), ld < width or w_out < max_segment * width; RAILS_ENOTSUP (nothing launched) for max_segment * width > 16 384 or
 * n_items > 2^32 - 1. */
int rails_lists_union(const int64_t* positions, int64_t ld, int32_t rows_in, int32_t width, const int64_t* lims, int32_t n_out, int32_t max_segment,
                      int64_t n_items, int64_t* out, int32_t w_out, int32_t* counts, void* stream);

/* Per-row candidates: out[bq * n_cand + x] = <queries[bq], items[bq / r][x]> for queries (n_queries, dim) and items
 * (n_queries / r, n_cand, dim) -- the two bmm branches of DotProductSimilarity.forward
 * (rails/similarities/dot_product_similarity_fn.py:55-68). */
int rails_dot_rowwise(const float* queries, const float* items, int64_t n_queries, int32_t n_cand, int32_t dim, int32_t r,
                      float* out, void* stream);

/* ---- coarse pass of the two-pass approximate top-k ---------------------------------------------
 * Replaces MoLAvgTopK.__init__'s averaged bf16 table (rails/indexing/mol_top_k.py:321-325) and the bf16 `mm`
 * of MoLAvgTopK.forward / topk_ids (mol_top_k.py:351-354, :418-425).  Every value the reference rounds to bf16
 * is rounded to bf16 here; scores come back as fp32 holding bf16 values.  The caller selects the K' best with
 * rails_topk and reranks with rails_mol_index_gather + rails_mol_score_candidates. */
size_t rails_mol_coarse_table_bytes(const rails_mol_shape* shape, int64_t n_items);   /* 2*d bytes per item */
int rails_mol_coarse_build(const rails_mol_shape* shape, const float* index, int64_t n_items, void* table, void* stream);
/* The rows of n_new positions (int64, device memory, unique, inside [0, n_items)) of an existing table, with rails_mol_coarse_build's arithmetic.
 * src_index is an fp32-format index: src_in_place != 0 -- the index the table belongs to, update j reads item positions[j]; 0 -- an index of the
 * n_new updated items alone (what a split-precision caller builds from their raw rows), update j reads item j.  2 d bytes written per update. */
int rails_mol_coarse_update(const rails_mol_shape* shape, const float* src_index, int32_t src_in_place, const int64_t* positions, int64_t n_new,
                            void* table, int64_t n_items, void* stream);
/* eq: plain (batch, P_Q, d) fp32 from rails_mol_query_prologue's eq_out.  average_queries 0: sum over P_Q
 * (forward), 1: mean over P_Q (topk_ids).  scores[b * ld + x]. */
int rails_mol_coarse_score(const rails_mol_shape* shape, const float* eq, int32_t batch, int32_t average_queries,
                           const void* table, int64_t n_items, float* scores, int64_t ld, const int32_t* run_if, void* stream);

/* Fused coarse scoring + exact top-K' (the same scores as rails_mol_coarse_score followed by rails_topk, without
 * materialising the (batch, n_items) matrix): per-group maxima of a strided sample of the table fix a per-query threshold,
 * one streaming pass collects the items at or above it, and the K' best of those are selected with the position tie rule.
 * Four launches.  out_scores / out_positions: (batch, k_prime), descending.  out_counts[b] = candidates query b collected;
 * the result for query b is exact iff k_prime <= out_counts[b] <= rails_mol_coarse_topk_capacity(batch, n_items, k_prime)
 * (min(24576, max(4096, 8 k_prime)) rounded up to a multiple of 64 for corpora beyond 4 Mi items; 4 k_prime below, where a denser
 * sample leaves ~1.8 k_prime candidates; capacity + 1 is reported when one of the 16 internal sub-lists overflowed) -- otherwise
 * (heavy ties at the threshold) the caller falls back to rails_mol_coarse_score + rails_topk; slots of an under-filled row
 * name position 0 with score -inf.  out_of_range (may be NULL): one int32 the call sets to 1 if some query's count is
 * outside that range and to 0 otherwise -- what rails_range_flag_i32 computes from out_counts, inside the call's own launches
 * (usable as the run_if predicate of the fallback).
 * k_prime <= 4096, batch <= 128 (slice larger batches).  rails_mol_coarse_topk_workspace_bytes returns 0 when the sizes are
 * unsupported. */
size_t rails_mol_coarse_topk_workspace_bytes(const rails_mol_shape* shape, int32_t batch, int64_t n_items, int32_t k_prime);
int32_t rails_mol_coarse_topk_capacity(int32_t batch, int64_t n_items, int32_t k_prime);   /* 0: unsupported sizes (ABI 10) */
int rails_mol_coarse_topk(const rails_mol_shape* shape, const float* eq, int32_t batch, int32_t average_queries,
                          const void* table, int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes,
                          float* out_scores, int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range,
                          void* prefilter, void* stream);
/* The same over the VISIBLE items only (added under ABI 15; hidden items, no counterpart in the reference): visible_words is one mask row
 * of rails_item_mask_words(n_items) words in device memory, bit set = the item may be returned, shared by the batch.  The sample scan
 * keeps hidden items out of the per-group maxima and the streaming pass drops them from the candidate lists, so the outputs are those of
 * rails_mol_coarse_score + rails_scores_mask(fill = -inf) + rails_topk under the same counts check (counts count visible candidates).
 * The call launches the scans' visible kernels; visible_words == NULL is rails_mol_coarse_topk itself, launch for launch.  With a
 * pre-filter the int8 pass is kept for d <= 64; at d = 128 the pass reads the bf16 table (same outputs). */
int rails_mol_coarse_topk_visible(const rails_mol_shape* shape, const float* eq, int32_t batch, int32_t average_queries,
                                  const void* table, int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes,
                                  float* out_scores, int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range,
                                  void* prefilter, const uint32_t* visible_words, void* stream);
/* The same with a PER-ROW filter by item tags (added under ABI 15): eff_tags holds the effective 32-bit tag word of each of the n_items items
 * (0 for a hidden item, rails_item_tags_effective), allowed one allow word per query b < batch; row b may return item x iff
 * eff_tags[x] & allowed[b] != 0.  The sample scan lets a score into row b's group maxima only where the test holds, the streaming pass
 * appends only such candidates (counts count them), so the outputs are those of rails_mol_coarse_score + rails_scores_mask_tags(fill =
 * -inf) + rails_topk under the same counts check.  The call launches the scans' tagged kernels; eff_tags == NULL is rails_mol_coarse_topk
 * itself, launch for launch.  With a pre-filter the int8 pass is kept for d <= 64 (its tagged kernel reads a fired tile's tag words and keeps
 * a row's allowed suspects only); at d = 128 the pass reads the bf16 table (same outputs), as for rails_mol_coarse_topk_visible. */
int rails_mol_coarse_topk_tagged(const rails_mol_shape* shape, const float* eq, int32_t batch, int32_t average_queries,
                                 const void* table, int64_t n_items, int32_t k_prime, void* workspace, size_t workspace_bytes,
                                 float* out_scores, int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range,
                                 void* prefilter, const uint32_t* eff_tags, const uint32_t* allowed, void* stream);
/* The numbers of the plan behind rails_mol_coarse_topk (comp_rows = 0, rows = batch) or rails_mol_component_topk (rows = batch * P_Q * P_X,
 * comp_rows = batch * P_Q) that the routing rule of a tagged call needs (added under ABI 15): out4 = {stride, r, G, s} -- the sample visits
 * every stride-th tile of 32 items, the threshold is the r-th largest of G per-group maxima and a group holds about s sampled items (G
 * counted for the d = 32 trip of four tiles: a lower bound at larger d).  Returns 1, or 0 where the sizes have no plan.  Host arithmetic. */
int32_t rails_mol_scan_plan(int32_t rows, int64_t n_items, int32_t k, int32_t comp_rows, int32_t* out4);
/* Optional int8 pre-filter of rails_mol_coarse_topk's streaming pass (no counterpart in the reference; it changes what the pass
 * READS, not what it returns): a copy of the coarse table as int8 with one scale (256-byte header + d bytes per item).  With it the
 * streaming pass reads the int8 copy, one int8 MFMA per 32 items, against a per-query integer bound that no item reaching the
 * query's threshold can miss (|bf16 dot - scaled int8 dot| <= s |q|_1 / 2 + s_q max|x|_1 / 2 + 3 s s_q d / 4), and scores only the
 * tiles that pass it from the bf16 table: same candidates, same counts, same output, about half the bytes.  prefilter == NULL: the
 * pass reads the bf16 table.  d in {32, 64, 128} (rails_mol_coarse_prefilter_bytes returns 0 otherwise).
 * The header keeps two running uint64 statistics the calls add to: bytes 32..39 = (32-item tile, 32-query tile) blocks that passed the
 * integer bound, bytes 40..47 = blocks tested.  A table whose single scale is set by a few outliers makes most blocks pass (the
 * output stays exact, the pass then reads both copies): a caller that reads a ratio near 1 should pass NULL from then on. */
size_t rails_mol_coarse_prefilter_bytes(const rails_mol_shape* shape, int64_t n_items);
int rails_mol_coarse_prefilter_build(const rails_mol_shape* shape, const void* table, int64_t n_items, void* prefilter, void* stream);

/* ---- per-component candidate generation (MoLNaiveTopK / MoLCombTopK) ------------------------------
 * Replaces the bf16 component table (rails/indexing/mol_top_k.py:61-73, :172-174) and the per-query-group bf16 `mm`
 * (mol_top_k.py:247-251, :498-502).  scores has batch * P_Q * P_X rows, row (b * P_Q + i) * P_X + m, n_items columns;
 * feed it to rails_topk with k = k_per_group and reshape the (rows, k) positions to (batch, P_Q * P_X * k). */
/* The table is ITEM-GROUP-major (ABI 9): table[m][x][:] = bf16(Ex[x, m, :]) for the n_total items of the corpus, so that a scan streams one group's
 * rows back to back.  rails_mol_component_build writes the rows of items [first_item, first_item + n_items) of every group from an index (chunk)
 * of n_items items -- one call with n_total = n_items, first_item = 0 for a whole index. */
size_t rails_mol_component_table_bytes(const rails_mol_shape* shape, int64_t n_items);   /* 2 * P_X * d bytes per item */
int rails_mol_component_build(const rails_mol_shape* shape, const float* index, int64_t n_items, void* table, int64_t n_total, int64_t first_item,
                              void* stream);
/* The rows of n_new positions in every item group of an existing table of n_total items (arguments as rails_mol_coarse_update). */
int rails_mol_component_update(const rails_mol_shape* shape, const float* src_index, int32_t src_in_place, const int64_t* positions, int64_t n_new,
                               void* table, int64_t n_total, void* stream);
int rails_mol_component_score(const rails_mol_shape* shape, const float* eq, int32_t batch, const void* table,
                              int64_t n_items, float* scores, int64_t ld, const int32_t* run_if, void* stream);
/* Fused scoring + exact top-k_group of every (query group, item group) row, without the (rows, n_items) score matrix:
 * same scheme, same outputs contract and same counts check as rails_mol_coarse_topk, over batch * P_Q * P_X rows.
 * out_scores / out_positions: (batch * P_Q * P_X, k_group); out_counts: (batch * P_Q * P_X).
 * batch * P_Q <= 256 query rows per call (128 at d = 128; a zero workspace size says "unsupported": callers slice the batch or take the materialising path).
 * out_of_range (optional, an int32 in device memory, zeroed by the call's first launch): raised when some row's candidate count left
 * [k_group, rails_mol_component_topk_capacity] -- the launch predicate of the caller's redo. */
size_t rails_mol_component_topk_workspace_bytes(const rails_mol_shape* shape, int32_t batch, int64_t n_items, int32_t k_group);
int32_t rails_mol_component_topk_capacity(const rails_mol_shape* shape, int32_t batch, int64_t n_items, int32_t k_group);
int rails_mol_component_topk(const rails_mol_shape* shape, const float* eq, int32_t batch, const void* table, int64_t n_items,
                             int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                             int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, void* stream);
/* The same over the visible items only (added under ABI 15): visible_words as for rails_mol_coarse_topk_visible, shared by every row. */
int rails_mol_component_topk_visible(const rails_mol_shape* shape, const float* eq, int32_t batch, const void* table, int64_t n_items,
                                     int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                                     int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, const uint32_t* visible_words,
                                     void* stream);
/* The same with a per-row filter by item tags (added under ABI 15): eff_tags / allowed as for rails_mol_coarse_topk_tagged, allowed[b] shared
 * by the P_Q * P_X rows of query b.  The tagged sample keeps four row tiles of maxima: batch * P_Q <= 128 query rows (RAILS_ENOTSUP beyond;
 * the caller slices the batch).  eff_tags == NULL is rails_mol_component_topk itself. */
int rails_mol_component_topk_tagged(const rails_mol_shape* shape, const float* eq, int32_t batch, const void* table, int64_t n_items,
                                    int32_t k_group, void* workspace, size_t workspace_bytes, float* out_scores,
                                    int64_t* out_positions, int32_t* out_counts, int32_t* out_of_range, const uint32_t* eff_tags,
                                    const uint32_t* allowed, void* stream);
/* ---- IVF-Flat index over the item components (MoLNaiveTopK use_faiss=True) ------------------------------------------
 * Replaces the per-item-group faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT) of rails/indexing/mol_top_k.py:176-199
 * and its search (:223-238): one independent index per item group m < P_X over the fp16-rounded components fp16(Ex[:, m, :]).
 * d in {32, 64, 128}, nlist <= 4096 (RAILS_ENOTSUP otherwise); n_items < nlist is RAILS_EINVAL.
 * The build entries read the components from exactly one source (the other NULL): `index`, an fp32-format item index, or `components16`,
 * the (P_X, n_items, d) fp16 table rails_ivf_components16_build writes chunk by chunk (for callers whose index is in a split-f16 format).
 *   centroids  (P_X, nlist, d) fp32, unit norm after training;
 *   vectors    (P_X, n_items, d) fp16 in list order;  positions (P_X, n_items) int32 item positions alongside (ascending inside a list);
 *   offsets    (P_X, nlist + 1) int32: list l of group m is [offsets[m][l], offsets[m][l + 1]).
 * rails_ivf_components16_build: components16[m][first_item + x][:] = fp16(Ex[x, m, :]) for the n_items items of an fp32-format index (chunk).
 * rails_ivf_train: spherical Lloyd k-means, `iters` iterations on the sample items sample_positions[0..n_sample) (drawn by the caller);
 * init != 0 first sets centroids to the first nlist sample items.  Assignment by the largest fp32 inner product (ties to the lower list),
 * per-list means summed in sample order, an empty list takes the largest list's centroid (ties to the lower id) and both are perturbed by
 * +-1/1024 per dimension, then every centroid is l2-normalised.  Deterministic: no float atomics.
 * rails_ivf_assign: assign[m][x] = the list of item x in group m, as training assigns (n_items * P_X int32).
 * rails_ivf_build_lists: assigns every item and writes vectors / positions / offsets with a stable counting sort.
 * workspace of both: rails_ivf_build_workspace_bytes(n_items, nlist, n_sample) bytes (n_sample = 0 for the list build). */
size_t rails_ivf_build_workspace_bytes(const rails_mol_shape* shape, int64_t n_items, int32_t nlist, int32_t n_sample);
int rails_ivf_components16_build(const rails_mol_shape* shape, const float* index, int64_t n_items, void* components16, int64_t n_total,
                                 int64_t first_item, void* stream);
int rails_ivf_train(const rails_mol_shape* shape, const float* index, const void* components16, int64_t n_items, const int32_t* sample_positions,
                    int32_t n_sample, int32_t nlist, int32_t iters, int32_t init, float* centroids, void* workspace, size_t workspace_bytes, void* stream);
int rails_ivf_assign(const rails_mol_shape* shape, const float* index, const void* components16, int64_t n_items, int32_t nlist,
                     const float* centroids, int32_t* assign, void* stream);
int rails_ivf_build_lists(const rails_mol_shape* shape, const float* index, const void* components16, int64_t n_items, int32_t nlist,
                          const float* centroids, void* vectors, int32_t* positions, int32_t* offsets, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Lists that follow an in-place change of the corpus under FROZEN centroids (FAISS IndexIVFFlat.add / remove_ids: the centroids are read,
 * never written).  rails_ivf_lists_edit reads the old lists of n_old entries per group -- every position 0 .. n_old - 1 once, as
 * rails_ivf_build_lists leaves them -- and writes FRESH buffers of n_new entries (no output may alias an input):
 *   dropped    every old entry whose position is >= n_keep or is one of positions[0..m) (device int64, unique; m may be 0);
 *   inserted   one entry per element of positions: its list by the assignment of rails_ivf_assign (the same kernel body: fma order and tie
 *              rule of a full assignment), its fp16 vector cut from the fp32-format index `source_index` -- item positions[j] when
 *              src_in_place != 0, item j otherwise (an index of the m new rows alone);
 *   order      every list ascending by position; new_offsets (P_X, nlist + 1).
 * The outputs are bit for bit what rails_ivf_build_lists writes from the resulting table with the same centroids, provided the result
 * holds every position 0 .. n_new - 1 once.  n_new is the caller's (host arithmetic), and must be exactly
 *   n_new = min(n_old, n_keep) - #{p in positions : p < min(n_old, n_keep)} + m.
 * An n_new above min(n_old, n_keep) + m is RAILS_EINVAL; any other wrong n_new cannot be told from the arguments and gives undefined list
 * CONTENTS (too small: entries are dropped; too large: the tail slots are not written) -- never a write outside the n_new entries.
 * Launches: drop mask, indexed assignment, one rails_sort_rows_i64 row per group over the inserted entries' (list, position) keys (hence
 * m <= 16384: RAILS_ENOTSUP beyond, rebuild with rails_ivf_build_lists), count / prefix / scan of the kept old slots in tiles of 4096, move,
 * insert, offsets.  Deterministic; no float atomics.  workspace: rails_ivf_lists_edit_workspace_bytes(shape, n_old, nlist, m) bytes, a pure host
 * function of its arguments; 0 with rails_last_error set: nlist outside [1, 4096], m outside [0, 16384], n_old outside [1, 2^31). */
size_t rails_ivf_lists_edit_workspace_bytes(const rails_mol_shape* shape, int64_t n_old, int32_t nlist, int64_t m);
int rails_ivf_lists_edit(const rails_mol_shape* shape, const float* source_index, int32_t src_in_place, const int64_t* positions, int64_t m,
                         int64_t n_keep, int32_t nlist, const float* centroids, const void* old_vectors, const int32_t* old_positions,
                         const int32_t* old_offsets, int64_t n_old, void* new_vectors, int32_t* new_positions, int32_t* new_offsets, int64_t n_new,
                         void* workspace, size_t workspace_bytes, void* stream);
/* HOST pointers: offsets is a host copy of the built offsets.  *max_probes = the probe capacity the short-list rule needs (the fewest
 * lists of any group whose sizes reach k_per_group, at least nprobe); *max_list = the largest list.  Both go to rails_ivf_search. */
int rails_ivf_plan(const rails_mol_shape* shape, const int32_t* offsets, int32_t nlist, int32_t nprobe, int32_t k_per_group, int32_t* max_probes,
                   int32_t* max_list);
/* out_positions (batch, P_Q * P_X * k_per_group) int64, row (b * P_Q + i) * P_X + m holding the k_per_group best items of group m for query
 * component eq[b, i, :] (eq: (batch, P_Q, d) fp32) by fp32 inner product with the fp16 vectors, best first (score desc, position asc),
 * among the nprobe lists of the best centroid scores (ties to the lower list).  Where those lists hold fewer than k_per_group items the
 * search goes on into further lists in centroid-score order until they do (FAISS returns -1 there); NaN scores rank last.  Three
 * launches per slice of 1024 / P_Q queries: centroid scores, the scan of each probed list for all its probes, the merge.
 * unfilled (optional, an int32 in device memory, zeroed by the call): raised when some row found fewer than k_per_group items, which
 * only a max_probes below rails_ivf_plan's can cause; such slots hold position 0.
 * nprobe <= min(64, nlist), k_per_group <= 128 (RAILS_ENOTSUP otherwise); 0 workspace bytes: arguments outside the limits. */
size_t rails_ivf_search_workspace_bytes(const rails_mol_shape* shape, int32_t batch, int32_t nlist, int32_t nprobe, int32_t max_probes,
                                        int32_t max_list, int32_t k_per_group);
int rails_ivf_search(const rails_mol_shape* shape, const float* eq, int32_t batch, const float* centroids, const void* vectors,
                     const int32_t* positions, const int32_t* offsets, int64_t n_items, int32_t nlist, int32_t nprobe, int32_t max_probes,
                     int32_t max_list, int32_t k_per_group, void* workspace, size_t workspace_bytes, int64_t* out_positions, int32_t* unfilled,
                     void* stream);
/* ---- filtered lists: the hidden set and allowed_tags inside the list scan (added under ABI 15: new entries only) -----
 * A filtered search returns, in the rows of query b, only items x with word(x) & allowed[b] != 0, and equals the plain search of an index built
 * with the same centroids from the kept items alone (positions mapped through the kept rows): the short-list rule counts a list's ELIGIBLE
 * entries, the scan drops the others before they are offered (their vectors are not read), the merge is rails_ivf_search's.
 * rails_ivf_list_words: list_words[m][slot] = word(positions[m][slot]) over the (groups, n_items) list entries, where word(x) = eff_tags[x]
 * (rails_item_tags_effective's array) or, with visible_words (one mask row of the corpus) instead, 0xffffffff for a visible item and 0 for a
 * hidden one.  Exactly one of the two is given.  One launch.
 * rails_ivf_list_counts: counts[r][m][l] = #{slot in list l of group m : list_words[m][slot] & allowed[r] != 0}, r < count_rows
 * ((count_rows, groups, nlist) int32).  One workgroup per (list, group), no atomics.
 * rails_ivf_plan_filtered: HOST pointers.  *max_probes = the probe capacity the short-list rule needs over every (row, group) of a host copy
 * of counts: the fewest lists whose counts reach k_per_group (nlist where they never do), at least nprobe, at most nlist.
 * rails_ivf_search_filtered: rails_ivf_search plus list_words, allowed (one word per BATCH row), counts and count_rows (1: one row of counts
 * shared by the batch; else batch).  list_words == NULL is rails_ivf_search itself.  max_list stays rails_ivf_plan's (the scan walks whole
 * lists); max_probes, the segments and the workspace only size the work.  A row whose eligible items are fewer than k_per_group raises
 * *unfilled: callers check the kept counts on the host first. */
int rails_ivf_list_words(const int32_t* positions, int32_t groups, int64_t n_items, const uint32_t* eff_tags, const uint32_t* visible_words,
                         uint32_t* list_words, void* stream);
int rails_ivf_list_counts(const uint32_t* list_words, const int32_t* offsets, int32_t groups, int64_t n_items, int32_t nlist, const uint32_t* allowed,
                          int32_t count_rows, int32_t* counts, void* stream);
int rails_ivf_plan_filtered(const int32_t* counts, int32_t count_rows, int32_t groups, int32_t nlist, int32_t nprobe, int32_t k_per_group,
                            int32_t* max_probes);
int rails_ivf_search_filtered(const rails_mol_shape* shape, const float* eq, int32_t batch, const float* centroids, const void* vectors,
                              const int32_t* positions, const int32_t* offsets, int64_t n_items, int32_t nlist, int32_t nprobe, int32_t max_probes,
                              int32_t max_list, int32_t k_per_group, void* workspace, size_t workspace_bytes, int64_t* out_positions,
                              int32_t* unfilled, const uint32_t* list_words, const uint32_t* allowed, const int32_t* counts, int32_t count_rows,
                              void* stream);
/* torch.sort(indices, dim=1) on (rows, n) int64, n <= 16384 (mol_top_k.py:257, :515); in == out allowed. */
int rails_sort_rows_i64(const int64_t* in, int32_t rows, int32_t n, int64_t* out, void* stream);
/* scores[r][j] = fill where sorted_idx[r][j] == sorted_idx[r][j-1] (mol_top_k.py:277-284, :535-542). */
int rails_mask_sorted_duplicates(const int64_t* sorted_idx, float* scores, int64_t ld, int32_t rows, int32_t n, float fill,
                                 void* stream);

/* ---- exact top-k -----------------------------------------------------------------------------
 * Replaces torch.topk(all_logits, dim=1, k, sorted, largest=True) + the id gather
 * (rails/indexing/mol_top_k.py:123-130).  Row b reads scores[b * ld + 0..n).  Ties are broken by
 * position ascending, so results are deterministic and identical for any sharding of the corpus.
 * If `ids` is non-NULL, out_ids[b][j] = ids[ids_row_stride * b + pos] (ids_row_stride 0 = one shared
 * id row, the reference's item_ids.squeeze(0)); else out_ids holds positions.
 * `sorted` == 0 still returns the exact top-k set (in descending order; unordered is a subset of valid
 * answers). */
size_t rails_topk_workspace_bytes(int32_t rows, int64_t n, int32_t k);
int rails_topk(const float* scores, int64_t ld, int32_t rows, int64_t n, int32_t k, int32_t sorted,
               const int64_t* ids, int64_t ids_row_stride, float* out_scores, int64_t* out_ids,
               void* workspace, size_t workspace_bytes, const int32_t* run_if, void* stream);

/* The final_topk of a candidate rerank (rails/indexing/mol_top_k.py:371-382: torch.topk over the candidates' scores,
 * torch.gather of their corpus positions, item_ids lookup) in one launch: row b holds n_cand <= 16384 scores, candidate j of row b
 * is corpus position positions[b * n_cand + j]; out_ids[b][j'] = ids[position] (ids: one shared id row, or NULL for the position
 * itself).  Same order and tie rule (candidate column ascending) as rails_topk on the same rows. */
int rails_topk_candidates(const float* scores, int64_t ld, int32_t rows, int32_t n_cand, int32_t k, const int64_t* positions,
                          const int64_t* ids, float* out_scores, int64_t* out_ids, void* stream);

/* The same selection with the seen-id filter of rails_filter_seen_ids applied to the k' winners inside the launch: what
 * CandidateIndex.get_top_k_outputs keeps of a candidate rerank (indexing/candidate_index.py:149-175 after rails/indexing/mol_top_k.py:260-293 /
 * :518-551, whose modules return ALL their candidates sorted: the first k unseen ones of that list are the first k unseen ones of its
 * top k + width, since a masked duplicate never outranks a scored candidate and at most `width` of the scored ones are seen) ->
 * (out_ids, out_scores) of k per row, the same bits as rails_topk_candidates(k') followed by rails_filter_seen_ids.
 * Sizes: 1024 < n_cand <= 8192, k <= k' <= 512, k' <= n_cand, width <= 256; RAILS_ENOTSUP otherwise (the caller composes the two calls). */
int rails_topk_candidates_filtered(const float* scores, int64_t ld, int32_t rows, int32_t n_cand, int32_t k_prime, const int64_t* positions,
                                   const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids,
                                   float* out_scores, void* stream);

/* The same result from candidates in ANY order, duplicates included (the union a Naive / Comb rerank collects, before the integer sort of
 * rails/indexing/mol_top_k.py:262 / :520 that makes duplicates neighbours): row b holds the scores of its n_cand candidate positions; of every
 * position the first copy counts, ranked by (score desc, position asc) -- the order of the sorted form -- then the top k' with the seen-id filter as
 * above.  Two launches (an LDS hash set of the row's positions writes the keys; the selection of rails_topk_candidates_filtered on them), no
 * sort.  *out_of_range (int32, device-visible, zeroed by the caller; may be pinned host memory) is set to 1 when a row holds fewer than k'
 * distinct positions: the outputs are then undefined and the caller takes the sorted form (rails_sort_rows_i64 -> score ->
 * rails_mask_sorted_duplicates -> rails_topk_candidates_filtered), which ranks masked duplicates as the reference does.  positions < 2^32 - 1.
 * Sizes as rails_topk_candidates_filtered; workspace: rails_rerank_workspace_bytes(rows, n_cand), 256-byte aligned. */
size_t rails_rerank_workspace_bytes(int32_t rows, int32_t n_cand);
int rails_rerank_topk_filtered(const float* scores, int64_t ld, int32_t rows, int32_t n_cand, int32_t k_prime, const int64_t* positions,
                               const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, void* workspace, size_t workspace_bytes,
                               int64_t* out_ids, float* out_scores, int32_t* out_of_range, void* stream);

/* ---- collapsing by item group (added under ABI 15; no counterpart in the reference) ------------------------------
 * At most one result per item group.  Every entry point takes DENSE group ranks: group_ranks[x] is an int32 in [0, n_groups) for each of the
 * n_items positions, equal for the items of one group, and an ungrouped item has a rank of its own (n_groups <= n_items).  ids: the id table
 * by position, NULL = a position is its own id.  invalid_ids: (rows, width) seen ids per row, unread when width == 0. */
/* The walk.  Row b holds a ranked list of `depth` entries (scores[b * ld + j], positions[b * depth + j]) that the caller guarantees to be in
 * key order (score descending, position ascending).  An entry is eligible iff its position lies in [0, n_items), its score is above -inf
 * and its id is not among the row's invalid_ids; the outputs are the first k eligible entries whose rank no earlier eligible entry of the
 * list has -- scores as given, positions, ids -- with (-inf, -1, -1) behind them where the list holds fewer than k.  out_counts[b]: how
 * many such entries the WHOLE list holds; *out_of_range (int32, device-visible, zeroed by the caller; may be pinned host memory) is set to 1
 * when some row holds fewer than k, and is usable as a run_if predicate.  One workgroup per row, one launch; 1 <= depth <= 16 384. */
int rails_topk_collapse(const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth, const int32_t* group_ranks,
                        int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, float* out_scores,
                        int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, void* stream);
/* The walk with a quota: at most max_per_group (>= 1) results per group.  Arguments, eligibility, outputs, out_counts and *out_of_range as
 * rails_topk_collapse; an eligible entry is kept iff FEWER THAN max_per_group earlier eligible entries of the list have its rank, and the
 * outputs are the first k kept entries.  max_per_group = 1 gives rails_topk_collapse's outputs bit for bit; a rank that occurs at most
 * max_per_group times among the eligible entries (every ungrouped item) never loses one.  One workgroup per row, one launch, no LDS beyond
 * rails_topk_collapse's; 1 <= depth <= 16 384.  RAILS_EINVAL for max_per_group < 1. */
int rails_topk_collapse_quota(const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth, const int32_t* group_ranks,
                              int64_t n_items, const int64_t* ids, const int64_t* invalid_ids, int32_t width, int32_t k, int32_t max_per_group,
                              float* out_scores, int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, void* stream);
/* One round of the per-group BEST-m of a score matrix.  The entries rails_scores_group_max considers, by the same tests (finite score, id not
 * among the row's invalid_ids, the same key); entry x of row b enters table[b * table_stride + r], r = group_ranks[first_item + x], by a
 * 64-bit integer maximum, only where below[b * below_stride + r] is non-zero and the entry's key is BELOW it.  below == NULL: no bound
 * (round 0, rails_scores_group_max's result).  With `below` the finished table of round t - 1, round t leaves in every slot the key of its
 * group's (t + 1)-th best eligible item, 0 once the group has fewer; the result does not depend on the order of arrival, and chunks of one
 * round may come in any order.  Strides count keys and are >= n_groups, so the m rounds of a row may lie side by side as one row of
 * m * n_groups keys (table = base + t * n_groups, below = base + (t - 1) * n_groups, both strides m * n_groups), which rails_topk_keys then
 * ranks: the keys stay distinct.  The CALLER zeroes a round's slots before its first chunk.  Limits as rails_scores_group_max. */
int rails_scores_group_next(const float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const int32_t* group_ranks, int64_t n_groups,
                            uint64_t* table, int64_t table_stride, const uint64_t* below, int64_t below_stride, const int64_t* ids,
                            const int64_t* invalid_ids, int32_t width, void* stream);
/* The per-group maxima of a score matrix: for every FINITE scores[b * ld + x], x < n, whose id is not among row b's invalid_ids,
 * table[b * n_groups + group_ranks[first_item + x]] = max(itself, key) with key = (orderable(score) << 32) | ~(first_item + x), the selection
 * key of rails_topk: afterwards a slot holds the key of its group's best eligible item under (score desc, position asc), 0 where the group
 * has none.  -inf entries (what rails_scores_mask* write) are skipped.  clear_table != 0: the (rows, n_groups) table is zeroed first, so a
 * chunked caller passes 1 with its first chunk and 0 after.  first_item + n < 2^32, width <= 4096, rows <= 65 535. */
int rails_scores_group_max(const float* scores, int64_t ld, int32_t rows, int64_t n, int64_t first_item, const int32_t* group_ranks, int64_t n_groups,
                           uint64_t* table, int32_t clear_table, const int64_t* ids, const int64_t* invalid_ids, int32_t width, void* stream);
/* The k largest keys of every row of such a table, descending, decoded: out_scores / out_positions / out_ids (rows, k), (-inf, -1, -1) where a
 * row has fewer than k non-zero keys; out_counts[b]: the row's non-zero keys.  The keys of a row are distinct, so there are no ties.  An MSD
 * radix selection over rows of any length, one workgroup per row; k <= 512. */
int rails_topk_keys(const uint64_t* table, int32_t rows, int64_t n_groups, int32_t k, const int64_t* ids, float* out_scores, int64_t* out_positions,
                    int64_t* out_ids, int32_t* out_counts, void* stream);

/* ---- diversifying a ranked list by maximal marginal relevance (added under ABI 15; no counterpart in the reference) ------------------------
 * Row b holds a ranked list of `depth` entries (scores[b * ld + j], positions[b * depth + j]).  Eligibility is rails_topk_collapse's: a position
 * in [0, n_items), a score above -inf (NaN is not), an id -- ids[position], or the position itself where ids == NULL -- not among the row's
 * `width` invalid_ids.  The POOL is the first `pool` eligible entries in list order, pool index c = 0 .. P - 1.  vectors: the (n_items, dim)
 * row-major fp32 item vectors, finite.  All arithmetic is fp32, round to nearest, unfused:  mu = 1.0f - lam;  sim(a, b) = the chain
 * acc = acc + a[e] * b[e], e = 0 .. dim - 1 ascending from acc = +0;  M[c] = +0 at first and fmaxf(M[c], sim(vec[c], vec[y])) after every pick
 * y;  val[c] = lam * s[c] - mu * M[c].  Step t = 0 .. k - 1 picks the unpicked pool entry with the largest 64-bit key
 * (orderable(val[c]) << 32) | ~c -- the largest val, ties to the smaller pool index.  Outputs in PICK order: the picked entries' own scores
 * (not val: a row is not monotone), positions and ids, with (-inf, -1, -1) behind them where P < k.  out_counts[b] = P; *out_of_range (int32,
 * device-visible, zeroed by the caller; may be pinned host memory) is set to 1 when some row has P < k.  One workgroup per row, one launch,
 * no atomics: the result is a function of the inputs, bit for bit.  lam = 1 returns the first k eligible entries of a list in key order.
 * 0 < lam <= 1 and k <= pool (RAILS_EINVAL otherwise); pool <= 1024, 1 <= dim <= 256, width <= 4096, 1 <= depth <= 16 384 (RAILS_ENOTSUP).
 * workspace: rails_topk_mmr_workspace_bytes(rows, pool, dim) bytes, 0 for dim <= 64 (workspace may then be NULL); every limit is checked
 * before any launch. */
size_t rails_topk_mmr_workspace_bytes(int32_t rows, int32_t pool, int32_t dim);
int rails_topk_mmr(const float* scores, int64_t ld, const int64_t* positions, int32_t rows, int32_t depth, const float* vectors, int64_t n_items,
                   int32_t dim, float lam, int32_t k, int32_t pool, const int64_t* ids, const int64_t* invalid_ids, int32_t width, void* workspace,
                   size_t workspace_bytes, float* out_scores, int64_t* out_positions, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range,
                   void* stream);

/* CandidateIndex.get_top_k_outputs' selection in ONE chain (reference indexing/candidate_index.py:149-175 after
 * rails/indexing/mol_top_k.py:123-130): exact top-k' of every row with the id map, then the seen-id filter of
 * rails_filter_seen_ids applied to the k' winners INSIDE the final selection launch -> (out_ids, out_scores) of k per row, the
 * same bits as rails_topk followed by rails_filter_seen_ids.  Sizes: rails_topk_filter_fusable(n, k', width, k) != 0
 * (n > 1024, k' <= 512, width <= 256); RAILS_ENOTSUP otherwise -- call the two entry points then. */
int rails_topk_filter_fusable(int64_t n, int32_t k_prime, int32_t width, int32_t k);
int rails_topk_filtered(const float* scores, int64_t ld, int32_t rows, int64_t n, int32_t k_prime, const int64_t* ids, int64_t ids_row_stride,
                        const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids, float* out_scores, void* workspace,
                        size_t workspace_bytes, const int32_t* run_if, void* stream);

/* ---- item-sharded top-k (no counterpart in the reference, whose eval is single-GPU: eval_from_checkpoint.py:554-555) ----
 * Each rank turns its local top-k into one message row of 2k int64 (k score words: fp32 bits in the low half | k ids;
 * rows with k_local < k are padded with (-inf, -1)); the caller all-gathers the messages in rank order; every rank
 * merges them.  Contiguous item-id shards + rank order keep the tie rule, so the result equals the unsharded top-k. */
int rails_pack_candidates(const float* scores, const int64_t* ids, int32_t rows, int32_t k_local, int32_t k, int64_t* msg,
                          void* stream);
/* gathered: (n_ranks, rows, 2k) int64.  n_ranks * k <= 16384.  k_out <= n_ranks * k. */
int rails_merge_candidates(const int64_t* gathered, int32_t n_ranks, int32_t rows, int32_t k, int32_t k_out,
                           float* out_scores, int64_t* out_ids, void* stream);
/* rails_merge_candidates followed by rails_filter_seen_ids in ONE launch (the sharded counterpart of rails_topk_filtered): the k_prime
 * merged winners of every row go through the seen-id filter inside the merge kernel and k_out (ids, scores) per row are written --
 * the same bits as the two calls.  k_prime <= 512, width <= 256 (RAILS_ENOTSUP otherwise). */
int rails_merge_candidates_filtered(const int64_t* gathered, int32_t n_ranks, int32_t rows, int32_t k, int32_t k_prime,
                                    const int64_t* invalid_ids, int32_t width, int32_t k_out, int64_t* out_ids, float* out_scores,
                                    void* stream);

/* rails_merge_candidates[_filtered] over the 2k + 2 wide messages of rails_candidates_finish's sharded form ([k score words | k ids | m | err] per
 * row and rank) WITH the global verdict of the item-sharded proved top-k in the same launch: row b is proved iff no rank reported a bad row
 * (err = inf), every guard value is within guard_limit, and  merged k_out-th score - max over ranks of m > eps  (eps as in rails_candidates_finish).
 * The last workgroup folds the rows into `state` (rails_rescore_verdict's layout) and mirrors it into state_host (optional, pinned host memory;
 * state_host[5], the call counter, is written last).  call_ws: 8 + 4 rows uint32 in device memory (16-byte aligned), zeroed once by the caller (every call leaves its first word, the arrival counter, zero).
 * Every rank computes the same verdict from the same gathered bytes, so the ranks agree on a redo without another exchange.
 * invalid_ids == NULL: (out_scores, out_ids) are (rows, k_out); else the seen-id filter runs inside the launch and they are (rows, f_k).
 * No counterpart in the reference (single-GPU eval: eval_from_checkpoint.py:554-555). */
int rails_merge_candidates_verdict(const int64_t* gathered, int32_t n_ranks, int32_t rows, int32_t k, int32_t k_out, float default_eps, float safety,
                                   const float* guard_values, int32_t guard_per_row, float guard_limit, float* state, float* state_host,
                                   void* call_ws, const int64_t* invalid_ids, int32_t width, int32_t f_k, int64_t* out_ids, float* out_scores,
                                   void* stream);

/* ---- candidate keys of the item-sharded MoLNaiveTopK / MoLCombTopK, global form (rails_amd/sharded.py; no counterpart in the reference) ----
 * The per-group component scores and the coarse scores are bf16 values carried in fp32, so ONE 64-bit key holds a candidate:
 *   bits 63..48  the order-preserving 16-bit image of the score: with h = the upper 16 bits of the fp32 word (the bf16 value; the
 *                lower 16 bits are not looked at), h | 0x8000 for a clear sign bit and ~h for a set one
 *   bits 47..0   2^48 - 1 - global position
 * so a LARGER unsigned key is the BETTER candidate and equal scores order by ascending global position.  This is rails_topk's total
 * order restricted to bf16: rails_topk compares the same image of the whole fp32 word (u | 0x80000000 / ~u), a bit-pattern order in
 * which +0 ranks above -0, +inf above every finite score, a NaN with a clear sign bit above +inf and a NaN with a set sign bit below
 * -inf; nothing is special-cased, here or there.  Key 0 is the pad: no candidate (a real candidate could only produce it as the
 * all-ones NaN at position 2^48 - 1).
 *
 * rails_group_keys_pack (one launch): scores / positions (rows, k_local), positions local in [0, n_local) (a negative one is written
 * as a pad) -> keys (rows, k_slots), k_slots >= k_local, the columns from k_local on padded with key 0.  The order of a row is kept, so
 * rows sorted best-first (what the scans and rails_topk leave) give descending keys.  offset = global position of the shard's item 0;
 * offset < 0 or offset + n_local > 2^48 is RAILS_EINVAL before any launch. */
int rails_group_keys_pack(const float* scores, const int64_t* positions, int32_t rows, int32_t k_local, int64_t offset, int64_t n_local,
                          int32_t k_slots, uint64_t* keys, void* stream);
/* 1 iff rails_group_keys_merge_own takes n_ranks lists of k keys per row (n_ranks * k <= 16384, the limit of rails_merge_candidates);
 * answers without a device. */
int rails_group_keys_supported(int32_t n_ranks, int32_t k);
/* rails_group_keys_merge_own (one launch): gathered = n_ranks messages in rank order, as an all-gather leaves them; the keys of rank r,
 * row b are gathered[r * rank_stride + b * k + j], j < k (rank_stride >= rows * k, in keys: a message may carry more than these rows).
 * Per row the best k of the n_ranks * k keys are selected (every list descending: merged by rank counting, one binary search per other
 * list; lists that are not descending are sorted in LDS instead) and per kept key, best first, two things are written:
 *   out_global[b * k + j]   the global position, -1 for a pad                                  (optional: may be NULL)
 *   out_local[(b / rows_per_out_row) * out_ld + out_col + (b % rows_per_out_row) * k + j]
 *                           position - lo where lo <= position < hi (this rank's items), else -1
 * so that the per-group rows of one query (rows_per_out_row = P_Q * P_X) and, in a second call, its coarse row (rows_per_out_row = 1,
 * out_col = P_Q * P_X * k_group) fill one (B, W) union buffer of row stride out_ld directly.  Equal keys (overlapping shards, pads)
 * keep rank order.  RAILS_ENOTSUP where rails_group_keys_supported is 0. */
int rails_group_keys_merge_own(const uint64_t* gathered, int32_t n_ranks, int64_t rank_stride, int32_t rows, int32_t k, int64_t lo, int64_t hi,
                               int64_t* out_global, int64_t* out_local, int64_t out_ld, int64_t out_col, int32_t rows_per_out_row,
                               void* stream);

/* Finish of a speculate-then-verify brute-force top-k (precision "f16x3-exact"; no counterpart in the reference, whose
 * MoLBruteForceTopK scores everything in one precision, mol_top_k.py:84-130).  Per row: n_cand entries with their exact fp32
 * logits (row stride ld) and corpus positions (< n_items <= 2^32).  The first n_ranked are the candidates: the top n_ranked items
 * by the approximate logits approx_scores (rows, n_ranked), same order.  The rest are probes: arbitrary items whose approximate
 * logit is read from the dense matrix approx_dense (row stride ld_dense) at their position.
 * Writes the candidates' top k by (exact score desc, position asc) -- the dense path's total order -- as (scores, ids[position]
 * or the position when ids is NULL), and row_ok[row] = 1 iff  k-th exact score > min candidate approx + margin_eps  and
 * |exact - approx| <= check_eps on every candidate and probe  (then no item outside the candidates can belong to the row's
 * top k, given |approx - exact| <= margin_eps everywhere; the probes watch that bound outside the candidates).  n_cand <= 16384.
 * row_stats (rows x 2 floats, optional): [largest |exact - approx| over the row's candidates and probes (inf for a NaN), k-th exact
 * score - min candidate approx], for callers that calibrate the bound from what they observe; row_ok or row_stats may be NULL.
 * one_sided != 0: approx_scores are UPPER BOUNDS of the exact scores (rails_mol_score_dense_upper): the monitored error is
 * max(0, exact - approx) -- zero while the bound holds -- and margin_eps = 0 is the proof (every item outside the candidates has
 * exact <= approx <= min candidate approx < k-th exact score). */
/* *flag |= 1 if any of the n int32 values lies outside [lo, hi]: the validity check of the fused scans' candidate counts
 * (rails_mol_coarse_topk / rails_mol_component_topk) on the device, feeding the launch predicate (run_if) of their materialising
 * redo (rails_mol_coarse_score / rails_mol_component_score + rails_topk).  The caller zeroes *flag. */
int rails_range_flag_i32(const int32_t* values, int32_t n, int32_t lo, int32_t hi, int32_t* flag, void* stream);

/* Verdict of a speculate-then-verify call, on the device: from the row_stats of rails_rescore_select (rows x 2 floats) and the
 * caller's calibration state (8 floats in device memory, zero-initialised once):
 *   state[0]  largest |first pass - fp32| ever observed (updated here; never decreases)
 *   state[1]  REDO flag, an int32 (written here): 1 iff some row's margin <= eps or a NaN or an infinite error was seen (a bad call: state[0] keeps its value), eps = max(default_eps, safety * state[0])
 *   state[2]  eps   state[3] / state[4]  this call's largest error / smallest margin   state[5] / state[6]  calls / redone calls so far
 *   state[7]  largest |guard value| ever observed
 * guard_values (optional, may be NULL): guard_count floats whose magnitudes must not exceed guard_limit for the caller's bound on
 * |first pass - fp32| to hold -- the proved exact top-k passes the batch's prescaled query-gate rows gq' (the one data-dependent magnitude of
 * its a-priori bound, rails_amd/f16x3_bound.py); a larger value or a NaN raises REDO like a failed margin.
 * No counterpart in the reference (rails/indexing/mol_top_k.py:99-130 scores every item in one precision). */
int rails_rescore_verdict(const float* row_stats, int32_t rows, float default_eps, float safety, const float* guard_values, int64_t guard_count,
                          float guard_limit, float* state, void* stream);

/* row_stats for a GLOBAL verdict of the item-sharded proved top-k (rails_amd/sharded.py; no counterpart in the reference, whose eval is
 * single-GPU: eval_from_checkpoint.py:554-555): row_stats[row] = [err_max[0], kth_scores[row * ld + col] - m_max[row]], where kth_scores
 * holds the merged top-k' (col = k' - 1), m_max the all-reduced maximum over ranks of the best first-pass score each rank left outside its
 * candidates, err_max the all-reduced largest |first pass - fp32| seen on any candidate.  Feed it to rails_rescore_verdict. */
int rails_margin_stats(const float* kth_scores, int64_t ld, int32_t col, const float* m_max, const float* err_max, int32_t rows, float* row_stats, void* stream);

int rails_rescore_select(const float* exact_scores, int64_t ld, const float* approx_scores, const float* approx_dense, int64_t ld_dense,
                         const int64_t* positions, const int64_t* ids, int64_t n_items, int32_t rows, int32_t n_ranked, int32_t n_cand,
                         int32_t k, float margin_eps, float check_eps, int32_t one_sided, float* out_scores, int64_t* out_ids, int32_t* row_ok,
                         float* row_stats, void* stream);

/* ---- candidates of the proved exact top-k: threshold selection and fused finish (round 6) -------------------------------------------
 * No counterpart in the reference (its MoLBruteForceTopK scores every item in one precision and calls torch.topk,
 * rails/indexing/mol_top_k.py:99-130; the seen-id filter fused below is indexing/candidate_index.py:149-175).  The speculate-then-verify
 * flow needs, per row, a candidate SET C and a value m such that every item outside C has a first-pass score <= m -- not the exact kc
 * best.  rails_candidates_select takes a threshold: with b(s) = the bin of score s among 4 096 equal bins of [lo, hi] (scores outside are
 * clamped; b is monotone), C = {x : b(s_x) >= b_t} for the LOWEST bin b_t that leaves at most `cap` candidates, and m = min over C of s.
 * One histogram launch + one compaction launch (rows of <= 65 536 scores: one launch), against the ten launches of an exact rails_topk
 * with k = kc.
 *   workspace: rails_candidates_workspace_bytes(rows) bytes, ZEROED ONCE by the caller; every select + finish pair leaves it zeroed.  Its
 *              first `rows` int32 are the rows' candidate counts between the two calls (rails_mol_score_indexed_rows' cand_counts).
 *   out_positions (rows, cand_ld) int64 / out_approx (rows, cand_ld) float: the candidates (in no particular order) and their first-pass
 *              scores; cand_ld >= cap; cap <= 16384; n < 2^32.  A NaN score raises the row's flag (the finish then fails the row).
 * rails_candidates_finish, one workgroup per row: the row's candidates sorted by (exact fp32 score desc, position asc) -- the dense
 * path's total order -- and the best k written as (out_scores, out_ids = ids[position] or the position when ids is NULL); the row FAILS
 * unless it has >= k candidates, no NaN, every guard value within guard_limit, and  k-th exact score - m > eps  with eps = max(default_eps,
 * safety * largest |exact - approx| seen so far (state[0]) or on this row)  -- then no item outside the candidates can belong to the row's
 * top k given |approx - exact| <= eps everywhere (one_sided != 0: approx are UPPER bounds of the exact scores, the monitored error is
 * max(0, exact - approx), default_eps = 0 is the proof).  A row whose candidates are all n_items items passes on that alone.
 * The last workgroup folds the rows into `state` (rails_rescore_verdict's layout; state[1] = the REDO flag, the launch predicate of the
 * caller's fallback) and mirrors it into state_host (optional; PINNED HOST memory mapped into the device: the words first, state_host[5],
 * the call counter the host polls, last -- no copy launch).  guard: rows x guard_per_row floats (the batch's prescaled query-gate rows).
 * invalid_ids != NULL: the seen-id filter of the candidate index over the k winners inside the same launch -> f_out_ids / f_out_scores
 * (rows, f_k); k <= 512, width <= 256.
 * msg != NULL (item-sharded form, rails_amd/sharded.py): instead of outputs and verdict, row b of msg (rows, 2k + 2) int64 receives
 * [k score words | k ids | m | largest error (inf: the row is bad)] -- short rows padded with (-inf, -1) -- for ONE all-gather; the verdict
 * is rails_merge_candidates_verdict's, after the merge. */
size_t rails_candidates_workspace_bytes(int32_t rows);
int rails_candidates_select(const float* scores, int64_t ld, int32_t rows, int64_t n, int32_t cap, float lo, float hi, void* workspace,
                            int64_t* out_positions, float* out_approx, int64_t cand_ld, void* stream);
int rails_candidates_finish(const float* exact_scores, int64_t ld, const float* approx, const int64_t* positions, int64_t cand_ld, int32_t cap,
                            void* workspace, const int64_t* ids, int64_t n_items, int32_t rows, int32_t k, float default_eps, float safety,
                            int32_t one_sided, const float* guard_values, int32_t guard_per_row, float guard_limit, float* out_scores,
                            int64_t* out_ids, const int64_t* invalid_ids, int32_t width, int32_t f_k, int64_t* f_out_ids, float* f_out_scores,
                            float* state, float* state_host, int64_t* msg, void* stream);

/* ---- arithmetic-model probes (test infrastructure of the proved exact top-k; no counterpart in the reference) -------------------------
 * The a-priori bound on |first pass - fp32 logit| (rails_amd/f16x3_bound.py) models the two matrix instructions and the two
 * transcendentals the scoring kernels are made of; these entry points run ONE such instruction per element on caller-supplied operands so
 * that tests can measure the model on the part (tests/test_gpu_parity.py::test_f16_mfma_accumulation_model and neighbours).
 *   rails_mfma_probe_f16: n independent D = C + A B with v_mfma_f32_32x32x16_f16; A (32 x 16) and B (16 x 32) row-major f16 bit patterns,
 *                         C and D (32 x 32) row-major fp32, n of each back to back.
 *   rails_mfma_probe_f32: the same with v_mfma_f32_32x32x2_f32; A (32 x 2), B (2 x 32) fp32.
 *   rails_scalar_probe_f32: out[0..n) = v_exp_f32(x), out[n..2n) = v_rcp_f32(x), out[2n..3n) = x / (1 + 2^x) as the kernels compute it. */
int rails_mfma_probe_f16(const uint16_t* a, const uint16_t* b, const float* c, float* d, int64_t n, void* stream);
int rails_mfma_probe_f32(const float* a, const float* b, const float* c, float* d, int64_t n, void* stream);
int rails_scalar_probe_f32(const float* x, int64_t n, float* out, void* stream);

/* ---- synthetic corpora (measurement and test infrastructure; no counterpart in the reference, whose item tables are trained) ----
 * out[(i - first_item) * dim + c] for items first_item <= i < first_item + n_items: a counter-based hash of (seed, i, c) --
 *   h = splitmix64((i * dim + c) ^ (seed * 0xD1B54A32D192ED03));  value = float(sum of h's four 16-bit lanes - 131070) * scale
 * -- so any shard or sub-range of a corpus is reproducible without materialising the table, on the device and (bit for bit) on the
 * host (oracle/mol_oracle.py hash_item_table, scale = float32(sigma * sqrt(3) / 65536): Irwin-Hall(4), std sigma). */
int rails_hash_item_table(uint64_t seed, int64_t first_item, int64_t n_items, int32_t dim, float scale, float* out, void* stream);

/* ---- seen-id filter --------------------------------------------------------------------------
 * Replaces the row-wise masking of CandidateIndex.get_top_k_outputs (indexing/candidate_index.py:154-178):
 * keep the first k ids of each row of (rows, k_prime) that do not occur in invalid_ids (rows, width),
 * back-filling from the filtered-out ones (in order) when fewer than k survive. */
int rails_filter_seen_ids(const int64_t* top_ids, const float* top_scores, int32_t rows, int32_t k_prime,
                          const int64_t* invalid_ids, int32_t width, int32_t k, int64_t* out_ids,
                          float* out_scores, void* stream);

/* ---- HSTU query encoder, eval path -----------------------------------
 * The step upstream of the retrieval path: modeling/sequential/hstu.py (HSTU.encode; its cache / delta path is rails_hstu_decode), without
 * fbgemm-gpu.  All tensors are fp32 and padded: (batch, seq_len, ...) with `lengths[b]` valid positions per row; rows at
 * positions >= lengths[b] are held at zero, which is what the reference's jagged layout amounts to.
 * rails_amd/hstu.py chains these per layer; a non-Python host would do the same. */
/* x = [ids != 0 and n < lengths[b]] * (embeddings * scale + pos_emb[n])      input_features_preprocessors.py:75-92 */
int rails_hstu_preprocess(const float* embeddings, const int64_t* ids, const int64_t* lengths, const float* pos_emb,
                          int32_t batch, int32_t seq_len, int32_t dim, float scale, float* out, void* stream);
/* out[r] = F.layer_norm(x[r], eps) (no affine) [* mul[r]]; ld* are row strides in floats.  hstu.py:268-276, :419-424 */
int rails_rows_layer_norm(const float* x, int64_t ldx, int64_t rows, int32_t dim, float eps, const float* mul, int64_t ldm,
                          float* out, int64_t ldo, void* stream);
/* C = act(A W + bias) + residual.  w_is_nk 0: W is (K, N) row-major (the `_uvqk` parameter); 1: W is (N, K), a torch Linear
 * weight (`_o.weight`).  act RAILS_ACT_*: 0 none / 1 silu / 2 relu / 3 gelu (erf, torch.nn.GELU()).  With lengths != NULL rows
 * r = b * seq_len + n, n >= lengths[b], are written as zeros.  hstu.py:374-378 (torch.mm + silu), :426-434 (the output Linear +
 * residual). */
#define RAILS_ACT_NONE 0
#define RAILS_ACT_SILU 1
#define RAILS_ACT_RELU 2
#define RAILS_ACT_GELU 3
int rails_gemm_f32(const float* a, int64_t lda, const float* w, int32_t w_is_nk, const float* bias, const float* residual,
                   int64_t ldr, int64_t m, int32_t n, int32_t k, int32_t act, const int64_t* lengths, int32_t seq_len, float* c,
                   int64_t ldc, void* stream);
/* The same GEMM with SASRec's row mask instead of the lengths mask: rows r with row_ids[r] == 0 are written as zeros
 * (sasrec.py:213, `user_embeddings *= valid_mask`; row_ids is the (m) id array of the rows). */
int rails_gemm_f32_id_masked(const float* a, int64_t lda, const float* w, int32_t w_is_nk, const float* bias, const float* residual,
                             int64_t ldr, int64_t m, int32_t n, int32_t k, int32_t act, const int64_t* row_ids, float* c, int64_t ldc,
                             void* stream);
/* MoLGatingFn.forward's combination + SoftmaxDropoutCombiner.forward as a stand-alone unit (reference
 * rails/similarities/mol/similarity_fn.py:148-201 and :31-46/:66-96, eval mode), for callers that use the modules on their own --
 * inside the scoring path all of this is fused into the scoring kernels.  Row r = b * items_per_query + x:
 *   g = query_part[b] * item_part[x or r] + pair_part[r]   (RAILS_COMBINE_GLU_SILU: w = g * sigmoid(g))
 *   g = the sum of the parts that are not NULL             (RAILS_COMBINE_NONE: w = g)
 *   pi = softmax(w) [/ clamp(sum pi, eps) if renormalise: the combiner does that whenever its dropout rate is > 0]
 *   out[r] = sum_l pi[l] * logits[r][l];  probs_out (rows, num_logits), optional, receives pi.
 * The combiner alone: pair_part = the gating weights, the other parts NULL, RAILS_COMBINE_NONE.  num_logits <= 1024. */
int rails_mol_gate_combine(const float* logits, int64_t ld_logits, const float* pair_part, int64_t ld_pair, const float* query_part,
                           const float* item_part, int64_t rows, int32_t items_per_query, int32_t num_logits, int32_t item_part_per_row,
                           int32_t combination, int32_t renormalise, float eps, float* out, float* probs_out, void* stream);

/* out = act(l) * g with [l | g] = x W + b: GeGLU (act = erf gelu) / SwiGLU (act = silu) as stand-alone layers
 * (reference rails/similarities/layers.py:19-74; `kind` RAILS_GEGLU | RAILS_SWIGLU).  w is the `_w` parameter, (in_features,
 * 2 * out_features) row-major; b the `_b` parameter (2 * out_features) or NULL; scratch holds rows * 2 * out_features floats
 * (the pre-activations); out is (rows, out_features) dense.  Inside the MoL path the same unit is fused into the query prologue
 * and the index build; this entry point serves callers that use the layer on its own. */
int rails_glu_f32(const float* x, int64_t ldx, const float* w, const float* b, int64_t rows, int32_t in_features, int32_t out_features,
                  int32_t kind, float* scratch, float* out, void* stream);
/* buckets[b][j][i] = #{t : thresholds[t] <= |ts[b, min(i+1, seq_len-1)] - ts[b, j]|} (uint8, key-major): the time bucket of
 * (query i, key j) of RelativeBucketedTimeAndPositionBasedBias (hstu.py:107-138); thresholds (num_buckets int64, ascending)
 * are the bucket edges of floor(log(max(|dt|, 1)) / 0.301) evaluated in float32 exactly as torch does.  Once per batch:
 * it depends on neither the layer nor the head. */
int rails_hstu_time_buckets(const int64_t* timestamps, int32_t batch, int32_t seq_len, const int64_t* thresholds,
                            int32_t num_buckets, uint8_t* out, void* stream);
/* uvqk: (batch * seq_len, ld) rows [u | v | q | k] (u, v: heads * dv wide; q, k: heads * dqk wide), the SiLU'd GEMM output.
 * out[b, i, h, :] = sum_{j <= i} silu(q_i . k_j + pos_w[seq_len - 1 + j - i] + ts_w[buckets[b, j, i]]) / seq_len * v_j ;
 * no bias at all when buckets == NULL (the reference without timestamps).  hstu.py:144-213.  dv <= 32, dqk <= 32. */
int rails_hstu_attention(const float* uvqk, int64_t ld, int32_t batch, int32_t seq_len, int32_t heads, int32_t dqk, int32_t dv,
                         const int64_t* lengths, const uint8_t* buckets, const float* ts_w, const float* pos_w,
                         int32_t num_buckets, float* out, void* stream);
/* The whole eval-path encoder in ONE launch for short sequences (seq_len <= 64 and the LDS bound checked by
 * rails_hstu_fused_supported): one workgroup per sequence keeps the residual stream, the uvqk activations and the bias tables
 * in LDS and runs all blocks back to back; writes the postprocessed embedding at position lengths[b] - 1 (HSTU.encode,
 * hstu.py:741-803).  `layers`: DEVICE array of n_blocks rails_hstu_layer (device pointers to each block's parameters; ts_w /
 * pos_w are only read when buckets != NULL).  buckets as for rails_hstu_attention.  RAILS_ENOTSUP for other geometries: the
 * caller then chains the per-layer entry points above. */
typedef struct rails_hstu_layer {
  const float* uvqk;   /* (dim, 2 * heads * (dv + dqk)) */
  const float* o_w;    /* (dim, heads * dv), a torch Linear weight */
  const float* o_b;    /* (dim) */
  const float* ts_w;   /* (num_buckets + 1) */
  const float* pos_w;  /* (2 * seq_len - 1) */
} rails_hstu_layer;
int rails_hstu_fused_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets);
int rails_hstu_encode_fused(const float* embeddings, const int64_t* ids, const int64_t* lengths, const uint8_t* buckets,
                            const float* pos_emb, const rails_hstu_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len,
                            int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets, int32_t postproc_mode, float eps,
                            float* out, void* stream);
/* Cached incremental decoding (HSTU.encode / generate_user_embeddings with delta_x_offsets and cache, hstu.py:144-213,
 * :276-433): ONE launch re-encodes one row per sequence, position positions[b] < lengths[b], through all n_blocks layers
 * against the K / V of every other position held in the cache, and writes that row's v, q, k and layer output into the cache
 * in place.  The jagged row of sequence b is sum_{b' < b} lengths[b'] + positions[b], derived from the lengths (no caller
 * offsets).  Per layer the cache is the reference's (v, padded_q, padded_k, outputs): v (cache_rows, heads * dv) and outputs
 * (cache_rows, dim) jagged, q / k (batch, seq_len, heads * dqk) padded; every layer's v / outputs have the same cache_rows.
 * Inputs: embeddings (batch, seq_len, dim) and ids (batch, seq_len) are read at row positions[b] only; timestamps
 * (batch, seq_len) or NULL (no bias); thresholds as for rails_hstu_time_buckets; pos_emb (>= seq_len, dim); linear_act
 * RAILS_ACT_NONE / RAILS_ACT_SILU (the uvqk activation).  out (batch, dim): the postprocessed last layer's outputs row at
 * lengths[b] - 1 (the cached row when positions[b] < lengths[b] - 1, as the reference returns).  A sequence whose length lies
 * outside [1, seq_len], whose position lies outside [0, length), or whose rows fall outside cache_rows is left alone: no cache
 * row is written and its out row is NaN.  `layers`: DEVICE array of n_blocks rails_hstu_decode_layer entries, ts_w / pos_w NULL for a
 * layer without relative bias.  dim <= 1024, dqk and dv <= 32, num_buckets <= 255 and an LDS bound, checked by
 * rails_hstu_decode_supported; RAILS_ENOTSUP otherwise. */
typedef struct rails_hstu_decode_layer {
  const float* uvqk;   /* parameters as in rails_hstu_layer */
  const float* o_w;
  const float* o_b;
  const float* ts_w;
  const float* pos_w;
  float* v;            /* (cache_rows, heads * dv) */
  float* q;            /* (batch, seq_len, heads * dqk) */
  float* k;            /* (batch, seq_len, heads * dqk) */
  float* outputs;      /* (cache_rows, dim) */
} rails_hstu_decode_layer;
int rails_hstu_decode_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets);
int rails_hstu_decode(const float* embeddings, const int64_t* ids, const int64_t* positions, const int64_t* lengths,
                      const int64_t* timestamps, const int64_t* thresholds, const float* pos_emb, const rails_hstu_decode_layer* layers,
                      int32_t n_blocks, int32_t batch, int32_t seq_len, int64_t cache_rows, int32_t dim, int32_t heads, int32_t dqk,
                      int32_t dv, int32_t num_buckets, int32_t linear_act, int32_t postproc_mode, float eps, float* out, void* stream);
/* Several rows per sequence in one step: the contiguous run of rows positions[b] .. positions[b] + m_b - 1 of sequence b is
 * re-encoded in ascending order through all layers against the cache, which gains those rows in place (per layer: v / outputs at
 * the jagged rows off_b + p, q / k at (b, p)); every other cache element keeps its bits.  The step equals m_b calls of the
 * single-row step at ascending positions, and an append must start at the OLD last row (the relative bias gives query row p the
 * timestamp of row p + 1, so row len_old - 1 changes when the sequence grows): positions = len_old - 1, m_b = len_new - len_old + 1.
 * counts: device int64 (batch), or NULL for m_b = max_rows everywhere; a count is clamped on the device into
 * [1, min(max_rows, lengths[b] - positions[b])].  The step runs batch * max_rows work-row slots (slot b * max_rows + t is idle when
 * t >= m_b); a row's arithmetic depends on neither its slot nor max_rows, so one step is bit for bit the max_rows = 1 calls at
 * ascending positions.  embeddings / ids are read at the run's rows only; out (batch, dim) is the postprocessed last layer's
 * outputs row at lengths[b] - 1 (the cached row when the run ends below it).  The jagged offsets are derived from `lengths` by a
 * scan into the workspace: no caller offset addresses a write.  A sequence whose length lies outside [1, seq_len] (or which
 * follows a length outside [0, seq_len]), whose start lies outside [0, length) or whose rows fall outside cache_rows is left
 * alone: no cache row written, a NaN out row; the others are unaffected.  Other arguments as rails_hstu_decode (`layers` a DEVICE
 * array).  work: device scratch of rails_hstu_decode_rows_workspace_floats(batch * max_rows, batch, ...) floats.  3 * n_blocks + 2
 * launches on `stream`, each layer's weights read once per 32 work rows.  rails_hstu_decode_rows_supported:
 * dim <= 1024, dqk and dv <= 32, num_buckets <= 255, and the LDS bound heads * dv <= 1024 (a tile of 32 rows of max(dim,
 * heads * dv) floats is staged: 128 KiB at the limit); RAILS_ENOTSUP otherwise.  RAILS_EINVAL: max_rows outside [1, seq_len], or
 * batch * max_rows > RAILS_HSTU_DECODE_MAX_ROWS (checked before any launch: the row tiles sit on a launch grid's y). */
#define RAILS_HSTU_DECODE_MAX_ROWS 2097120   /* 65535 launch-grid rows of 32 work rows */
int rails_hstu_decode_rows_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets);
int64_t rails_hstu_decode_rows_workspace_floats(int64_t work_rows, int32_t batch, int32_t dim, int32_t heads, int32_t dqk, int32_t dv);
int rails_hstu_decode_rows(const float* embeddings, const int64_t* ids, const int64_t* positions, const int64_t* counts, int32_t max_rows,
                           const int64_t* lengths, const int64_t* timestamps, const int64_t* thresholds, const float* pos_emb,
                           const rails_hstu_decode_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len, int64_t cache_rows,
                           int32_t dim, int32_t heads, int32_t dqk, int32_t dv, int32_t num_buckets, int32_t linear_act,
                           int32_t postproc_mode, float eps, float* work, float* out, void* stream);
/* ---- SASRec query encoder, eval path ----------------------------------------------------------------------------------
 * modeling/sequential/sasrec.py (SASRec.encode / forward, dropout off).  The per-layer route: rails_hstu_preprocess with every
 * length = seq_len (x = (ids != 0) * (emb * sqrt(dim) + pos_emb)), then per block rails_rows_layer_norm (eps 1e-8),
 * rails_gemm_f32 (the in-projection, unmasked: q from LN(x), k / v from x), rails_sasrec_attention, rails_gemm_f32 (out_proj +
 * the LN(x) residual), rails_rows_layer_norm, rails_gemm_f32 (conv1 + relu / gelu), rails_gemm_f32_id_masked (conv2 + residual,
 * times the id mask); rails_rows_normalize last.
 *
 * Causal softmax attention (torch.nn.MultiheadAttention with the bool causal mask): qkv is (batch * seq_len, ld) with rows
 * [q | k | v], each `dim` wide (heads x head_dim, head_dim = dim / heads <= 64); out (batch * seq_len, dim) dense:
 *   out[b, i, h, :] = sum_{j <= i} softmax_j(q_i . k_j / sqrt(head_dim)) v_j      (every key j <= i; no key is masked by id) */
int rails_sasrec_attention(const float* qkv, int64_t ld, int32_t batch, int32_t seq_len, int32_t dim, int32_t heads, float* out,
                           void* stream);
/* The whole encoder in ONE launch for short sequences (rails_sasrec_fused_supported: seq_len <= 64, dim <= 128, ffn_dim <= 128,
 * head_dim <= 64): one workgroup per sequence, everything in LDS; writes the postprocessed embedding at position lengths[b] - 1
 * (SASRec.encode).  `layers`: DEVICE array of n_blocks rails_sasrec_layer.  ffn_act RAILS_ACT_RELU / RAILS_ACT_GELU;
 * postproc_mode 0 LayerNorm, 1 L2 norm, with eps.  RAILS_ENOTSUP for other geometries: chain the per-layer entries instead. */
typedef struct rails_sasrec_layer {
  const float* in_proj_weight;   /* (3 * dim, dim) */
  const float* in_proj_bias;     /* (3 * dim) */
  const float* out_proj_weight;  /* (dim, dim) */
  const float* out_proj_bias;    /* (dim) */
  const float* conv1_weight;     /* (ffn_dim, dim[, 1]) */
  const float* conv1_bias;       /* (ffn_dim) */
  const float* conv2_weight;     /* (dim, ffn_dim[, 1]) */
  const float* conv2_bias;       /* (dim) */
} rails_sasrec_layer;
int rails_sasrec_fused_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t ffn_dim);
int rails_sasrec_encode_fused(const float* embeddings, const int64_t* ids, const int64_t* lengths, const float* pos_emb,
                              const rails_sasrec_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len, int32_t dim,
                              int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps, float* out,
                              void* stream);
/* Cached incremental decoding (SASRec.encode with cache=): for every sequence b, p = lengths[b] - 1 is re-encoded through all
 * n_blocks blocks against the key / value rows 0..p-1 of each block's cache, and the block's fresh k / v row is written to cache
 * row p in place (rows > p are neither read nor written).  Causal attention and the per-row id mask make this exact: out equals
 * the encode of the updated sequence up to fp32 summation order.  embeddings (batch, seq_len, dim) and ids (batch, seq_len) are
 * read at row p only; pos_emb (>= seq_len, dim); out (batch, dim) the postprocessed row p (postproc_mode / eps as
 * rails_sasrec_encode_fused).  A length outside [1, seq_len] is clamped into it (the caller validates).  `layers`: HOST array of
 * n_blocks rails_sasrec_decode_layer, each cache k / v a dense (batch, seq_len, dim) float32 device array holding the
 * in-projection's key / value rows (bias included) of the block's input.  work: device scratch of
 * rails_sasrec_decode_workspace_floats(batch, dim, ffn_dim) floats.  5 * n_blocks + 1 launches on `stream`, every output column
 * split across workgroups.  rails_sasrec_decode_supported: seq_len <= 2048, dim and ffn_dim <= 1024,
 * head_dim <= 64; RAILS_ENOTSUP otherwise. */
typedef struct rails_sasrec_decode_layer {
  const float* in_proj_weight;   /* parameters as in rails_sasrec_layer */
  const float* in_proj_bias;
  const float* out_proj_weight;
  const float* out_proj_bias;
  const float* conv1_weight;
  const float* conv1_bias;
  const float* conv2_weight;
  const float* conv2_bias;
  float* k;                      /* (batch, seq_len, dim) */
  float* v;                      /* (batch, seq_len, dim) */
} rails_sasrec_decode_layer;
int rails_sasrec_decode_supported(int32_t seq_len, int32_t dim, int32_t heads, int32_t ffn_dim);
int64_t rails_sasrec_decode_workspace_floats(int32_t batch, int32_t dim, int32_t ffn_dim);
int rails_sasrec_decode(const float* embeddings, const int64_t* ids, const int64_t* lengths, const float* pos_emb,
                        const rails_sasrec_decode_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len, int32_t dim,
                        int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps, float* work, float* out,
                        void* stream);
/* Several rows per sequence in one step: the last m_b rows of sequence b, positions lengths[b] - m_b .. lengths[b] - 1, are
 * re-encoded in order through all blocks and their k / v written to those cache rows in place; every other cache row keeps its
 * bits.  Appending m_b events (lengths grew by m_b) and editing an interior row (lengths unchanged, the rows from the edited one on
 * re-encoded) are the same call.  new_counts: device int64 (batch), or NULL for m_b = max_new everywhere; a count is clamped on the
 * device into [1, min(max_new, lengths[b])].  embeddings / ids are read at the new rows only; out (batch, dim) is the postprocessed
 * row lengths[b] - 1.  The step runs batch * max_new work-row slots (slot b * max_new + t is idle when t >= m_b): work holds
 * rails_sasrec_decode_workspace_floats(batch * max_new, dim, ffn_dim) floats, and still 5 * n_blocks + 1 launches.  A row's
 * arithmetic does not depend on its slot: the step is bit for bit max_new calls of rails_sasrec_decode at growing lengths, and
 * rails_sasrec_decode is the max_new = 1, NULL-counts call.  RAILS_ENOTSUP with a message: max_new outside [1, seq_len], or
 * batch * max_new > RAILS_SASREC_DECODE_MAX_ROWS (checked before any launch; the only limit on the batch, at any head count:
 * the step's attention launch has its work rows on grid.x and the heads on grid.y). */
#define RAILS_SASREC_DECODE_MAX_ROWS 2097120   /* 65535 launch-grid rows of 32 work rows */
int rails_sasrec_decode_rows(const float* embeddings, const int64_t* ids, const int64_t* lengths, const int64_t* new_counts, int32_t max_new,
                             const float* pos_emb, const rails_sasrec_decode_layer* layers, int32_t n_blocks, int32_t batch, int32_t seq_len,
                             int32_t dim, int32_t heads, int32_t ffn_dim, int32_t ffn_act, int32_t postproc_mode, float eps, float* work,
                             float* out, void* stream);
/* out[r] = normalise(x[row_index ? row_index[r] : r]); mode 0 LayerNorm (no affine), 1 x / max(||x||, eps).
 * output_postprocessors.py:38-85 + get_current_embeddings (modeling/sequential/utils.py:74-90). */
int rails_rows_normalize(const float* x, int64_t ldx, const int64_t* row_index, int64_t rows, int32_t dim, int32_t mode, float eps,
                         float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RAILS_AMD_H_ */
