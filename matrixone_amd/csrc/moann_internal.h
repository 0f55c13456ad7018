/* Internal interfaces between moann_lib.cpp (host/ABI) and
 * moann_kernels.hip (CDNA4 device code). Not part of the public ABI. */

#ifndef MOANN_INTERNAL_H
#define MOANN_INTERNAL_H

#include <hip/hip_runtime.h>
#include <cstdint>

#include "moann_scan_plan.h" /* MetricKind, ScanVariant */

namespace moann {

/* One scan job: a (list segment, query tile) pair. SoA device arrays; the
 * scan kernels take the whole table as one by-value argument and read their
 * row of it through JobView (moann_scan_device.h). */
struct ScanJobs {
    const int64_t* databaseg;  /* [njobs] base group index of the list       */
    const int32_t* gstart;     /* [njobs] first group (list-relative)        */
    const int32_t* gcount;     /* [njobs] groups this job scans              */
    const int32_t* rows;       /* [njobs] valid rows in the WHOLE list       */
    const int32_t* nq;         /* [njobs] queries in the tile (<= QT)        */
    const int32_t* qbase;      /* [njobs] offset into qslot arrays           */
    const int32_t* qslot_query;   /* [nqslots] query index                   */
    const int64_t* qslot_outbase; /* [nqslots] output base in dists buffer   */
    const int64_t* slot_base;     /* [njobs] global slot of list row 0 (for
                                     the membership filter; may be null)     */
    int njobs;
};

/* Launch the distance scan over interleaved packed data.
 * packed layout: group g, dim-quad j4, lane l, c -> packed[((g*dpad + 4*j4)*64) + l*4 + c]
 * i.e. [g][dpad/4][64][4] floats; row (g*64+l) holds vector dims 4*j4+c.
 * queries: [nq_total][dpad] device, zero-padded.
 * qnorms: [nq_total] sum-of-squares (cos only, else nullptr).
 * dists_out: ragged candidate buffer, written at qslot_outbase + row.
 *
 * The three scan launchers take the ScanVariant the job table was planned
 * with (pick_scan) and switch on it, never re-deriving a kernel or width; a
 * variant without a kernel throws std::logic_error before any HIP call. */
void launch_scan(int metric, ScanVariant variant, const float* packed,
                 const float* queries, const float* qnorms, int dpad,
                 const ScanJobs& jobs, float* dists_out, hipStream_t stream,
                 const uint32_t* filter_bitset = nullptr);

/* Hand-scheduled asm specialization of the scan for the flagship shape
 * (scan_asm768.hip): METRIC=L2SQ, dpad=768, QT=16, one group per wave.
 * launch_scan dispatches here for ScanKind::F32_ASM768. */
void launch_scan_asm768(const float* packed, const float* queries,
                        int dpad, const ScanJobs& jobs, float* dists_out,
                        hipStream_t stream,
                        const uint32_t* filter_bitset = nullptr);

/* Per-query ascending top-k select (radix select + in-LDS bitonic sort).
 * Candidates for query q live at dists[off(q) .. off(q)+count(q)) where
 * off/count come from qoffs (ragged, [nq+1]) or uniform n (qoffs==nullptr).
 * out_slots: [nq][k] candidate index within the query's range, -1 padding.
 * out_dists: [nq][k] ascending, FLT_MAX padding. k <= 4096. */
void launch_topk(const float* dists, const int64_t* qoffs, int64_t uniform_n,
                 int nq, int k, int32_t* out_slots, float* out_dists,
                 hipStream_t stream);

/* The same selection for long ragged rows (qoffs required, dists 16-byte
 * aligned): rows the rule of moann_select_plan.h admits are selected in one
 * read against a sampled threshold (select_filter_kernel), every other row,
 * and a row whose threshold turns out bad, by the radix select above. The
 * output is the k smallest by (key, index): what launch_topk writes whenever
 * it does not end in its level-3 tie mode. stats (device, [2]) is added to:
 * [0] rows the filter finished, [1] rows that fell back. */
void launch_select(const float* dists, const int64_t* qoffs, int nq, int k,
                   int32_t* out_slots, float* out_dists,
                   unsigned long long* stats, hipStream_t stream);

/* Map selected candidate slots to entry ids + apply the score transform
 * (scoreFromQuantized: raw/mul^2, then sqrt for orig-l2 — ivfflat/search.go:
 * 1062-1077). probe_lists/-offs describe each query's probed lists in rank
 * order. list_slot_base maps list -> base slot of id_by_slot. */
void launch_gather(const int32_t* sel_slots, const float* sel_dists,
                   const int32_t* probe_lists, const int64_t* probe_offs,
                   const int64_t* list_slot_base, const int64_t* id_by_slot,
                   int nprobe, int nq, int k, int do_sqrt, double inv_mul2,
                   int64_t* out_ids, float* out_dists, hipStream_t stream);

/* Same transform for uniform (brute-force / centroid) results where the slot
 * IS the row: id = id_by_slot ? id_by_slot[slot] : slot. */
void launch_gather_uniform(const int32_t* sel_slots, const float* sel_dists,
                           const int64_t* id_by_slot, int nq, int k,
                           int do_sqrt, double inv_mul2,
                           int64_t* out_ids, float* out_dists,
                           hipStream_t stream);

/* Pack rows into the interleaved layout.
 * group_rowbase[g]: index into slot_rows of the group's first row;
 * group_valid[g]: valid rows in group g; slot_rows: slot -> source row. */
void launch_pack(const float* vecs, int dim, int dpad,
                 const int64_t* group_rowbase, const int32_t* group_valid,
                 const int64_t* slot_rows, int64_t ngroups, float* packed,
                 hipStream_t stream);

/* Inverse of pack (save_dir): packed -> row-major rows in slot order. */
void launch_unpack(const float* packed, int dim, int dpad,
                   const int64_t* group_slotbase, const int32_t* group_valid,
                   int64_t ngroups, int64_t slot_lo, int64_t slot_hi,
                   float* out, hipStream_t stream);

/* MFMA f32 centroid-rank GEMM (mfma_rank.hip). Returns false when the
 * metric has no MFMA path (L1). */
bool launch_rank_gemm(int metric, const float* queries, const float* cents,
                      const float* qnorms, const float* cnorms, int nq,
                      int nlist, int dpad, float* out, hipStream_t stream);

/* ---- native k-means build (kmeans_kernels.hip) ----
 * A row set is a view of the staged f32 rows: row i of the set is staged row
 * (i*num)/den — the training sample's stride rule (moann_kmeans_plan.h) with
 * num = n, den = n_train; num == den is the identity. Nothing is copied. */
struct KmRowMap {
    int64_t num, den;
};

/* Fused nearest-centroid assignment: assign[i] = argmin_c dist(row i, c),
 * best[i] = that distance, for KM_L2SQ (expanded, clamped at 0), KM_IP and
 * KM_COS — rank_gemm_kernel's distances. Ties go to the lowest index. cents
 * is the zero-padded [k][dpad] matrix; rows have stride row_stride (= dim).
 * No [n][k] buffer; throws std::logic_error for KM_L1. */
void launch_km_assign(int metric, const float* rows, int64_t row_stride,
                      KmRowMap map, int64_t n, const float* cents,
                      const float* cnorms, int k, int dim, int dpad,
                      int32_t* assign, float* best, hipStream_t stream);
/* out[i] = |row i|^2, or 1/|row i| (0 for a zero row) when inverse_norm */
void launch_km_row_sumsq(bool inverse_norm, const float* rows,
                         int64_t row_stride, KmRowMap map, int64_t n, int dim,
                         float* out, hipStream_t stream);
/* Deterministic centroid update from a CSR of the assignment (offs [k+1],
 * members = set rows grouped by centroid, ascending inside a group): mean of
 * the members, rows scaled by inv_norm[i] when non-null (spherical k-means).
 * Fixed order, no atomics; an empty centroid keeps its value. */
void launch_km_update(const float* rows, int64_t row_stride, KmRowMap map,
                      const int64_t* offs, const int32_t* members,
                      const float* inv_norm, int k, int dim, int dpad,
                      float* cents, hipStream_t stream);
/* cents[cidx[b]][0..dim) = set row trow[b], b < count (init and reseed) */
void launch_km_set_centroids(const float* rows, int64_t row_stride,
                             KmRowMap map, const int32_t* cidx,
                             const int64_t* trow, int count, int dim, int dpad,
                             float* cents, hipStream_t stream);
/* set rows [i0, i0+count) -> out[count][dpad], zero-padded */
void launch_km_gather_pad(const float* rows, int64_t row_stride, KmRowMap map,
                          int64_t i0, int64_t count, int dim, int dpad,
                          float* out, hipStream_t stream);

/* ---- resident brute-force index (bf_kernels.hip) ----
 * The candidate buffer of a search is [nq][slices][k] (distance, row) pairs,
 * each slice's segment sorted ascending by (distance, row) and padded with
 * (FLT_MAX, -1); rows are indices into the row store. `mask` has one bit per
 * row, cleared = excluded, null = every row passes. */
struct BfPlan; /* moann_bf_plan.h */

/* Fused exact distance + per-slice top-k for KM_L2SQ, KM_IP and KM_COS
 * (rank_gemm_kernel's distances from the given norms), k <= BF_FUSED_KMAX:
 * fills the whole candidate buffer of `plan` (slices, tiles_per_slice) for
 * these nq queries. Deterministic; throws std::logic_error for KM_L1 or a
 * larger k. */
void launch_bf_fused_topk(int metric, const float* rows, const float* xnorms,
                          const uint32_t* mask, int64_t n,
                          const float* queries, const float* qnorms, int nq,
                          int dpad, int k, const BfPlan& plan, float* cand_d,
                          int32_t* cand_r, hipStream_t stream);
/* The same over an f16 row store (bf_half_kernels.hip): rows and queries are
 * binary16 [.][dpad], dpad % 8 == 0, zero-padded; the dot product comes from
 * the f16 MFMA (exact products, f32 accumulation), the norms are f32. */
void launch_bf_fused_topk_h(int metric, const uint16_t* rows,
                            const float* xnorms, const uint32_t* mask,
                            int64_t n, const uint16_t* queries,
                            const float* qnorms, int nq, int dpad, int k,
                            const BfPlan& plan, float* cand_d, int32_t* cand_r,
                            hipStream_t stream);
/* binary16 [nrows][dpad_h] -> f32 [nrows][dpad_w] (dpad_w <= dpad_h), exact:
 * the gemm mode's operand over an f16 store */
void launch_bf_widen_half(const uint16_t* in, int64_t nrows, int dpad_h,
                          int dpad_w, float* out, hipStream_t stream);
/* dmat [nq][len] holds rows [row0, row0+len): excluded rows -> FLT_MAX */
void launch_bf_mask(float* dmat, int nq, int64_t len, int64_t row0,
                    const uint32_t* mask, hipStream_t stream);
/* one chunk's launch_topk output [nq][k] -> segment `slice` of the candidate
 * buffer; slots that are padding or carry FLT_MAX become (FLT_MAX, -1) */
void launch_bf_stash(const int32_t* sel_slots, const float* sel_dists, int nq,
                     int k, int64_t row0, int64_t slice, int64_t nslices,
                     float* cand_d, int32_t* cand_r, hipStream_t stream);
/* final launch_topk slots -> candidate row -> id; (-1, FLT_MAX) for padding;
 * do_sqrt takes the square root of the selected distances (L2sqrt) */
void launch_bf_gather(const int32_t* sel_slots, const float* sel_dists,
                      const int32_t* cand_r, int64_t cand_per_q,
                      const int64_t* ids, int nq, int k, int do_sqrt,
                      int64_t* out_ids, float* out_dists, hipStream_t stream);

/* Quantized (int8/uint8) list scan + helpers. `layout` is the byte order of
 * `packed` (moann_scan_plan.h): ROWS16 takes the variant's dot or uchar4
 * kernel, MFMA64 takes scan_i8_mfma_kernel and throws for a variant, metric
 * or dpad that kernel does not cover. */
void launch_scan_i8(int metric, ScanVariant variant, bool uns,
                    ByteImageLayout layout, const uint8_t* packed,
                    const uint8_t* queries_q, const int32_t* qnorms,
                    const int32_t* rownorms, int dpad, const ScanJobs& jb,
                    float* dists_out, hipStream_t stream,
                    const uint32_t* filter_bitset = nullptr);
/* pack row-major quantized rows in MFMA order (dpad % 64 == 0) */
void launch_bytes_pack_mfma(const uint8_t* rows_q, int dpad,
                            const int64_t* group_rowbase,
                            const int32_t* group_valid,
                            const int64_t* slot_rows, int64_t ngroups,
                            uint8_t* packed, hipStream_t stream);
/* per-(group,lane) sum-of-squares over the packed byte rows (build-time,
 * feeds the dot-form scan's rn + qn - 2*dot L2) */
void launch_bytes_pack16(const uint8_t* rows_q, int dpad,
                         const int64_t* group_rowbase,
                         const int32_t* group_valid,
                         const int64_t* slot_rows, int64_t ngroups,
                         uint8_t* packed, hipStream_t stream);
void launch_rownorms_i8(bool uns, ByteImageLayout layout,
                        const uint8_t* packed, int64_t ngroups, int dpad,
                        int32_t* out, hipStream_t stream);
void launch_unpack_bytes(const uint8_t* packed, int dim, int dpad,
                         const int64_t* group_slotbase,
                         const int32_t* group_valid, int64_t ngroups,
                         int64_t slot_lo, int64_t slot_hi, uint8_t* out,
                         hipStream_t stream);
/* exact f32 re-rank of byte-stage top-R (two-stage scan; SQ8 + refine) */
void launch_refine(int metric, const float* rows_f32, const float* queries,
                   const float* qnorms, int dim, int dpad, int R, int nq,
                   const int32_t* rsel_slots, const float* rsel_dists,
                   const int32_t* probe_lists, const int64_t* probe_offs,
                   const int64_t* list_slot_base, int nprobe, float* refined,
                   hipStream_t stream);
void launch_compose_select(const int32_t* sel2, const int32_t* rsel_slots,
                           int R, int k, int nq, int32_t* out,
                           hipStream_t stream);
/* launch_refine -> launch_topk over [nq][R] -> launch_compose_select ->
 * launch_gather as one kernel, same ids and distance bits; for the R and
 * dpad refine_finish_applies admits (R <= 1024, LDS), k <= R */
bool refine_finish_applies(int R, int dpad);
void launch_refine_finish(int metric, const float* rows_f32,
                          const float* queries, const float* qnorms, int dim,
                          int dpad, int R, int nq, const int32_t* rsel_slots,
                          const float* rsel_dists, const int32_t* probe_lists,
                          const int64_t* probe_offs,
                          const int64_t* list_slot_base,
                          const int64_t* id_by_slot, int nprobe, int k,
                          int do_sqrt, double inv_mul2, int64_t* out_ids,
                          float* out_dists, hipStream_t stream);
void launch_quantize_rows(bool uns, const float* in, int64_t nrows,
                          int in_stride, int dim, int dpad, float fmul,
                          float fadd, uint8_t* out, hipStream_t stream);
void launch_pq_pack(const uint8_t* codes_rowmajor, int nsub,
                    const int64_t* group_rowbase, const int32_t* group_valid,
                    const int64_t* slot_rows, int64_t ngroups, uint8_t* packed,
                    hipStream_t stream);
/* half (f16/bf16) storage: plain-cast quantization + decoded-f32 scan */
void launch_quantize_half_rows(bool bf, const float* in, int64_t nrows,
                               int in_stride, int dim, int dpad,
                               uint16_t* out, hipStream_t stream);
void launch_qnorms_h(bool bf, const uint16_t* q, int nq, int dpad,
                     float* out, hipStream_t stream);
void launch_scan_h(int metric, ScanVariant variant, bool bf,
                   const uint16_t* packed, const uint16_t* queries_h,
                   const float* qnorms, int dpad, const ScanJobs& jb,
                   float* dists_out, hipStream_t stream,
                   const uint32_t* filter_bitset = nullptr);
void launch_qnorms_i8(bool uns, const uint8_t* q, int nq, int dpad,
                      int32_t* out, hipStream_t stream);

/* 1xN pairwise distances (SQL builtin batch / mocl.cu counterpart). */
void launch_pairwise(int metric, const float* rows, const float* query,
                     float qnorm, int64_t n, int dim, float* out,
                     hipStream_t stream);

/* Sum-of-squares per query row (cosine). queries: [nq][dpad]. */
void launch_qnorms(const float* queries, int nq, int dpad, float* qnorms,
                   hipStream_t stream);

}  // namespace moann

#endif
