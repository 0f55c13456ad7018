/* libmoann_hip — resident brute-force index, host side (include/moann.h,
 * "resident brute force"). The rows stay in HBM as
 * [cap][dpad], f32 or binary16, with their norms, ids and an alive bitset; a
 * search plans its slices (moann_bf_plan.h), fills the candidate buffer with
 * the fused kernel of the storage (bf_kernels.hip, bf_half_kernels.hip) or
 * the rank-GEMM + launch_topk composition, and ends in one launch_topk and a
 * gather. An f16 store narrows what it is given (rows and queries) with
 * round-to-nearest-even and refuses what has no finite binary16 value. Same
 * conventions as the other families: errmsg out-params, grow-only workspaces,
 * fail-loud. */

#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/moann.h"
#include "moann_bf_plan.h"
#include "moann_host_common.h"

namespace {

using namespace moann;

#define HIP_CHECK MOANN_HIP_CHECK /* local short names */
#define KCHECK MOANN_KCHECK

struct BfIndex {
    int device = 0, cus = 1;
    uint32_t dim = 0, dpad = 0; /* dpad in elements of the storage type    */
    quantization_t storage = Quantization_F32;
    uint32_t esz = 4;   /* bytes per stored element                        */
    uint32_t dpad4 = 0; /* (dim+3)&~3: f32 row of the gemm mode's operands */
    distance_type_t metric = DistanceType_L2Expanded;
    int kmetric = KM_L2SQ;
    int64_t cap = 0, len = 0;
    int mode = BF_AUTO;
    int64_t slice_rows = 0;

    hipStream_t stream = nullptr;
    void* d_rows = nullptr;      /* [cap][dpad], zero-padded        */
    float* d_xn = nullptr;       /* [cap] |x|^2                     */
    int64_t* d_ids = nullptr;    /* [cap]                           */
    uint32_t* d_alive = nullptr; /* [(cap+31)/32], bit set = alive  */
    std::vector<uint32_t> h_alive;
    bool any_deleted = false, alive_dirty = false;
    /* id -> rows; kept only once an add has passed ids of its own (until
     * then id == row) */
    bool seq_ids = true;
    std::unordered_multimap<int64_t, int64_t> row_of_id;

    MoannDevBuf w_queries, w_qnorms, w_mask, w_cand_d, w_cand_r, w_dmat,
        w_sel_slots, w_sel_dists, w_fin_slots, w_fin_dists, w_out_ids,
        w_out_dists;
    /* f16 store: f32 input on its way to the narrowing kernel, the narrowed
     * queries, and the gemm mode's widened slice */
    MoannDevBuf w_stage, w_queries_h, w_wide;
    std::vector<uint32_t> h_mask; /* alive AND filter, staged for the H2D */

    std::mutex mu;
    moann_perf_t perf {};
    hipEvent_t ev[3] {}; /* scan begin, scan end, select end */
    bool ev_made = false;

    ~BfIndex() {
        (void)hipSetDevice(device);
        for (auto p : {d_rows, (void*)d_xn, (void*)d_ids,
                       (void*)d_alive})
            if (p) (void)hipFree(p);
        if (ev_made)
            for (auto& e : ev) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

BfIndex* BX(moann_bf_c h) {
    if (!h) throw std::runtime_error("null index");
    return (BfIndex*)h;
}

/* Grow the four row-store arrays to `ncap` rows: new allocations, a
 * device-to-device copy of the rows held, nothing re-packed. */
void grow(BfIndex* ix, int64_t ncap) {
    const hipStream_t s = ix->stream;
    void* rows = nullptr;
    float* xn = nullptr;
    int64_t* ids = nullptr;
    uint32_t* alive = nullptr;
    const size_t aw = (size_t)((ncap + 31) / 32);
    try {
        HIP_CHECK(hipMalloc(&rows, (size_t)ncap * ix->dpad * ix->esz));
        HIP_CHECK(hipMalloc(&xn, (size_t)ncap * 4));
        HIP_CHECK(hipMalloc(&ids, (size_t)ncap * 8));
        HIP_CHECK(hipMalloc(&alive, aw * 4));
        if (ix->len) {
            HIP_CHECK(hipMemcpyAsync(rows, ix->d_rows,
                                     (size_t)ix->len * ix->dpad * ix->esz,
                                     hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(xn, ix->d_xn, (size_t)ix->len * 4,
                                     hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(ids, ix->d_ids, (size_t)ix->len * 8,
                                     hipMemcpyDeviceToDevice, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        for (auto p : {rows, (void*)xn, (void*)ids, (void*)alive})
            if (p) (void)hipFree(p);
        throw;
    }
    for (auto p : {ix->d_rows, (void*)ix->d_xn, (void*)ix->d_ids,
                   (void*)ix->d_alive})
        if (p) (void)hipFree(p);
    ix->d_rows = rows;
    ix->d_xn = xn;
    ix->d_ids = ids;
    ix->d_alive = alive;
    ix->h_alive.resize(aw, 0u);
    ix->alive_dirty = true; /* the device copy is rebuilt from the host's */
    ix->cap = ncap;
}

/* First of n rows [.][dim] that holds a value without a finite binary16
 * value: NaN, an infinity, or |v| >= 65520, which rounds to infinity. -1 if
 * there is none. */
int64_t first_unhalfable_row(const float* v, uint64_t n, uint32_t dim) {
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < dim; ++c)
            if (!(std::fabs(v[r * dim + c]) < 65520.0f)) return (int64_t)r;
    return -1;
}

/* The same for binary16 input: an exponent of all ones. */
int64_t first_nonfinite_half_row(const uint16_t* v, uint64_t n, uint32_t dim) {
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < dim; ++c)
            if ((v[r * dim + c] & 0x7c00u) == 0x7c00u) return (int64_t)r;
    return -1;
}

void pad_results(uint64_t nq, uint32_t k, int64_t* out_ids, float* out_dists) {
    for (uint64_t i = 0; i < nq * (uint64_t)k; ++i) {
        out_ids[i] = -1;
        out_dists[i] = FLT_MAX;
    }
}

void run_search(BfIndex* ix, const float* queries, bool on_device,
                uint64_t nq, uint32_t dim, uint32_t k,
                const uint32_t* row_bitset, uint64_t nbits, bool filtered,
                int64_t* out_ids, float* out_dists) {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (dim != ix->dim)
        throw std::runtime_error("query dimension " + std::to_string(dim) +
                                 " != index dimension " +
                                 std::to_string(ix->dim));
    if (k < 1 || k > (uint32_t)BF_K_LIMIT)
        throw std::runtime_error("k must be in [1, 4096]");
    if (filtered && !row_bitset) throw std::runtime_error("null row_bitset");
    if (filtered && nbits < (uint64_t)ix->len)
        throw std::runtime_error("row_bitset covers " + std::to_string(nbits) +
                                 " rows, the index holds " +
                                 std::to_string(ix->len));
    if (nq == 0) return;
    if (!queries || !out_ids || !out_dists)
        throw std::runtime_error("null queries or output buffer");
    const bool half = ix->storage == Quantization_F16;
    if (half && !on_device) {
        const int64_t bad = first_unhalfable_row(queries, nq, dim);
        if (bad >= 0)
            throw std::runtime_error(
                "query " + std::to_string(bad) +
                " holds a value with no finite f16 value (|v| >= 65520, inf "
                "or NaN); the index stores and compares f16");
    }
    if (ix->len == 0) {
        pad_results(nq, k, out_ids, out_dists);
        return;
    }
    const auto wall0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipSetDevice(ix->device));
    const hipStream_t s = ix->stream;
    const int64_t n = ix->len;
    const int dpad = (int)ix->dpad;
    const BfPlan plan =
        bf_plan(n, (int64_t)nq, k, ix->mode, ix->slice_rows, ix->cus,
                half ? (int64_t)ix->dpad4 * 4 : 0);
    if (!ix->ev_made) {
        for (auto& e : ix->ev) HIP_CHECK(hipEventCreate(&e));
        ix->ev_made = true;
    }

    /* one bitset for the kernels: alive AND filter */
    const size_t words = (size_t)((n + 31) / 32);
    const uint32_t* d_mask = nullptr;
    if (filtered) {
        ix->h_mask.resize(words);
        for (size_t w = 0; w < words; ++w)
            ix->h_mask[w] = row_bitset[w] & ix->h_alive[w];
        upload_vector(ix->w_mask, ix->h_mask, s);
        d_mask = ix->w_mask.as<uint32_t>();
    } else if (ix->any_deleted) {
        if (ix->alive_dirty) {
            HIP_CHECK(hipMemcpyAsync(ix->d_alive, ix->h_alive.data(),
                                     words * 4, hipMemcpyHostToDevice, s));
            /* h_alive may change right after this call returns, and the
             * stream is synchronised before it does */
            ix->alive_dirty = false;
        }
        d_mask = ix->d_alive;
    }

    ix->w_out_ids.ensure((size_t)plan.q_batch * k * 8);
    ix->w_out_dists.ensure((size_t)plan.q_batch * k * 4);
    ix->w_cand_d.ensure((size_t)plan.cand_entries * 4);
    ix->w_cand_r.ensure((size_t)plan.cand_entries * 4);
    ix->w_fin_slots.ensure((size_t)plan.q_batch * k * 4);
    ix->w_fin_dists.ensure((size_t)plan.q_batch * k * 4);
    if (plan.mode == BF_GEMM) {
        ix->w_dmat.ensure((size_t)plan.dmat_entries * 4);
        ix->w_sel_slots.ensure((size_t)plan.q_batch * k * 4);
        ix->w_sel_dists.ensure((size_t)plan.q_batch * k * 4);
        if (half) ix->w_wide.ensure((size_t)plan.wide_bytes);
    }
    float* cand_d = ix->w_cand_d.as<float>();
    int32_t* cand_r = ix->w_cand_r.as<int32_t>();
    const int do_sqrt = ix->metric == DistanceType_L2SqrtExpanded;
    double scan_ms = 0, select_ms = 0;

    for (int64_t q0 = 0; q0 < (int64_t)nq; q0 += plan.q_batch) {
        const int qb = (int)std::min<int64_t>(plan.q_batch, (int64_t)nq - q0);
        const float* d_q = nullptr; /* f32 queries: f32 store, or gemm mode */
        const uint16_t* d_qh = nullptr;
        const float* d_qn = nullptr;
        if (ix->kmetric != KM_IP) {
            ix->w_qnorms.ensure((size_t)qb * 4);
            d_qn = ix->w_qnorms.as<float>();
        }
        if (!half) {
            d_q = stage_padded_queries(
                ix->w_queries, queries + (size_t)q0 * dim, on_device,
                (uint64_t)qb, ix->dim, ix->dpad, s);
            if (d_qn) {
                launch_qnorms(d_q, qb, dpad, ix->w_qnorms.as<float>(), s);
                KCHECK("bf qnorms");
            }
        } else {
            /* narrow to [qb][dpad] f16; norms of the rounded values; the
             * gemm mode runs over those values widened back to f32 */
            const float* src = queries + (size_t)q0 * dim;
            if (!on_device) {
                ix->w_stage.ensure((size_t)qb * dim * 4);
                HIP_CHECK(hipMemcpyAsync(ix->w_stage.ptr, src,
                                         (size_t)qb * dim * 4,
                                         hipMemcpyHostToDevice, s));
                src = ix->w_stage.as<float>();
            }
            ix->w_queries_h.ensure((size_t)qb * dpad * 2);
            launch_quantize_half_rows(false, src, qb, (int)dim, (int)dim,
                                      dpad, ix->w_queries_h.as<uint16_t>(),
                                      s);
            KCHECK("bf narrow queries");
            d_qh = ix->w_queries_h.as<uint16_t>();
            if (d_qn) {
                launch_qnorms_h(false, d_qh, qb, dpad,
                                ix->w_qnorms.as<float>(), s);
                KCHECK("bf qnorms");
            }
            if (plan.mode == BF_GEMM) {
                ix->w_queries.ensure((size_t)qb * ix->dpad4 * 4);
                launch_bf_widen_half(d_qh, qb, dpad, (int)ix->dpad4,
                                     ix->w_queries.as<float>(), s);
                KCHECK("bf widen queries");
                d_q = ix->w_queries.as<float>();
            }
        }
        HIP_CHECK(hipEventRecord(ix->ev[0], s));
        if (plan.mode == BF_FUSED && half) {
            launch_bf_fused_topk_h(ix->kmetric, (const uint16_t*)ix->d_rows,
                                   ix->d_xn, d_mask, n, d_qh, d_qn, qb, dpad,
                                   (int)k, plan, cand_d, cand_r, s);
            KCHECK("bf_fused_topk_h");
        } else if (plan.mode == BF_FUSED) {
            launch_bf_fused_topk(ix->kmetric, (const float*)ix->d_rows,
                                 ix->d_xn, d_mask, n, d_q, d_qn, qb, dpad,
                                 (int)k, plan, cand_d, cand_r, s);
            KCHECK("bf_fused_topk");
        } else {
            for (int64_t sl = 0; sl < plan.slices; ++sl) {
                int64_t lo, hi;
                bf_slice_range(plan, n, sl, &lo, &hi);
                const int64_t len = hi - lo;
                const float* xs;
                int xpad = dpad;
                if (half) {
                    launch_bf_widen_half(
                        (const uint16_t*)ix->d_rows + (size_t)lo * dpad, len,
                        dpad, (int)ix->dpad4, ix->w_wide.as<float>(), s);
                    KCHECK("bf widen rows");
                    xs = ix->w_wide.as<float>();
                    xpad = (int)ix->dpad4;
                } else {
                    xs = (const float*)ix->d_rows + (size_t)lo * dpad;
                }
                if (!launch_rank_gemm(ix->kmetric, d_q, xs, d_qn,
                                      ix->d_xn + lo, qb, (int)len, xpad,
                                      ix->w_dmat.as<float>(), s))
                    throw std::logic_error("metric has no GEMM form");
                KCHECK("bf rank_gemm");
                launch_bf_mask(ix->w_dmat.as<float>(), qb, len, lo, d_mask, s);
                KCHECK("bf_mask");
                launch_topk(ix->w_dmat.as<float>(), nullptr, len, qb, (int)k,
                            ix->w_sel_slots.as<int32_t>(),
                            ix->w_sel_dists.as<float>(), s);
                KCHECK("bf chunk topk");
                launch_bf_stash(ix->w_sel_slots.as<int32_t>(),
                                ix->w_sel_dists.as<float>(), qb, (int)k, lo,
                                sl, plan.slices, cand_d, cand_r, s);
                KCHECK("bf_stash");
            }
        }
        HIP_CHECK(hipEventRecord(ix->ev[1], s));
        /* position order of the candidates is (distance, row) order: slices
         * ascend with the rows and each segment is sorted */
        launch_topk(cand_d, nullptr, plan.slices * k, qb, (int)k,
                    ix->w_fin_slots.as<int32_t>(),
                    ix->w_fin_dists.as<float>(), s);
        KCHECK("bf final topk");
        launch_bf_gather(ix->w_fin_slots.as<int32_t>(),
                         ix->w_fin_dists.as<float>(), cand_r,
                         plan.slices * k, ix->d_ids, qb, (int)k, do_sqrt,
                         ix->w_out_ids.as<int64_t>(),
                         ix->w_out_dists.as<float>(), s);
        KCHECK("bf_gather");
        HIP_CHECK(hipEventRecord(ix->ev[2], s));
        HIP_CHECK(hipMemcpyAsync(out_ids + (size_t)q0 * k, ix->w_out_ids.ptr,
                                 (size_t)qb * k * 8, hipMemcpyDeviceToHost,
                                 s));
        HIP_CHECK(hipMemcpyAsync(out_dists + (size_t)q0 * k,
                                 ix->w_out_dists.ptr, (size_t)qb * k * 4,
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float a = 0, b = 0;
        HIP_CHECK(hipEventElapsedTime(&a, ix->ev[0], ix->ev[1]));
        HIP_CHECK(hipEventElapsedTime(&b, ix->ev[1], ix->ev[2]));
        scan_ms += a;
        select_ms += b;
        ix->perf.scan_launches += plan.mode == BF_FUSED ? 1 : plan.slices;
    }
    const double wall_ms =
        std::chrono::duration<double, std::milli>(
            std::chrono::steady_clock::now() - wall0).count();
    ix->perf.scan_ms += scan_ms;
    ix->perf.select_ms += select_ms;
    ix->perf.other_ms += std::max(0.0, wall_ms - scan_ms - select_ms);
    ix->perf.scan_rows += (uint64_t)n * nq;
    ix->perf.scan_bytes +=
        (uint64_t)n * ix->dim * ix->esz * (uint64_t)plan.passes;
}

template <typename F>
void guarded(void* errmsg, const char* where, F&& f) {
    try {
        f();
    } catch (const std::exception& e) {
        moann_set_errmsg(errmsg, where, e.what());
    }
}

moann_bf_c bf_new(const char* where, uint32_t dimension,
                  distance_type_t metric, quantization_t storage,
                  uint64_t capacity_hint, const int* devices, int device_count,
                  void* errmsg) {
    try {
        if (storage != Quantization_F32 && storage != Quantization_F16)
            throw std::runtime_error(
                "storage must be Quantization_F32 or Quantization_F16");
        if (dimension == 0) throw std::runtime_error("dimension must be > 0");
        if (metric == DistanceType_L1)
            throw std::runtime_error(
                "L1 has no GEMM form; use the one-shot "
                "moann_brute_force_search for L1");
        if (metric != DistanceType_L2Expanded &&
            metric != DistanceType_L2SqrtExpanded &&
            metric != DistanceType_InnerProduct &&
            metric != DistanceType_CosineExpanded)
            throw std::runtime_error("unsupported metric");
        if (capacity_hint > (uint64_t)BF_MAX_ROWS)
            throw std::runtime_error("the index holds at most 2^31-1 rows");
        auto ix = std::make_unique<BfIndex>();
        ix->device = (devices && device_count > 0) ? devices[0] : 0;
        HIP_CHECK(hipSetDevice(ix->device));
        int cus = 0;
        HIP_CHECK(hipDeviceGetAttribute(
            &cus, hipDeviceAttributeMultiprocessorCount, ix->device));
        ix->cus = cus > 0 ? cus : 1;
        HIP_CHECK(hipStreamCreate(&ix->stream));
        ix->dim = dimension;
        ix->storage = storage;
        ix->dpad4 = (dimension + 3) & ~3u;
        if (storage == Quantization_F16) {
            ix->esz = 2;
            ix->dpad = (dimension + 7) & ~7u; /* rows start on 16 bytes */
        } else {
            ix->dpad = ix->dpad4;
        }
        ix->metric = metric;
        ix->kmetric = metric_kind(metric);
        if (capacity_hint) grow(ix.get(), (int64_t)capacity_hint);
        return (moann_bf_c)ix.release();
    } catch (const std::exception& e) {
        moann_set_errmsg(errmsg, where, e.what());
        return nullptr;
    }
}

/* n rows from host memory to the end of an f16 store, with their norms (of
 * the values stored). Exactly one of rows_f (narrowed on the device, through
 * a bounded staging buffer) and rows_h (copied as they are) is given. */
void upload_half_rows(BfIndex* ix, const float* rows_f, const uint16_t* rows_h,
                      uint64_t n) {
    const hipStream_t s = ix->stream;
    const int64_t l0 = ix->len;
    const uint32_t dim = ix->dim, dpad = ix->dpad;
    uint16_t* dst = (uint16_t*)ix->d_rows + (size_t)l0 * dpad;
    if (rows_h) {
        if (dim != dpad)
            HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)n * dpad * 2, s));
        HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dpad * 2, rows_h,
                                   (size_t)dim * 2, (size_t)dim * 2, n,
                                   hipMemcpyHostToDevice, s));
    } else {
        /* 64 MiB of f32 rows at a time, one row at least */
        uint64_t chunk = ((uint64_t)64 << 20) / ((uint64_t)dim * 4);
        chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, n));
        ix->w_stage.ensure((size_t)chunk * dim * 4);
        for (uint64_t o = 0; o < n; o += chunk) {
            const uint64_t c = std::min<uint64_t>(chunk, n - o);
            HIP_CHECK(hipMemcpyAsync(ix->w_stage.ptr, rows_f + (size_t)o * dim,
                                     (size_t)c * dim * 4,
                                     hipMemcpyHostToDevice, s));
            launch_quantize_half_rows(false, ix->w_stage.as<float>(),
                                      (int64_t)c, (int)dim, (int)dim,
                                      (int)dpad, dst + (size_t)o * dpad, s);
            KCHECK("bf narrow rows");
        }
    }
    /* one block per row: chunks that keep the grid inside int32 */
    for (uint64_t o = 0; o < n; o += (1u << 30)) {
        const int c = (int)std::min<uint64_t>(n - o, 1u << 30);
        launch_qnorms_h(false, dst + (size_t)o * dpad, c, (int)dpad,
                        ix->d_xn + l0 + o, s);
        KCHECK("bf row norms");
    }
}

/* moann_bf_add (rows_f) and moann_bf_add_half (rows_h) */
void add_rows(moann_bf_c h, const float* rows_f, const uint16_t* rows_h,
              uint64_t n, const int64_t* ids) {
    auto ix = BX(h);
    std::lock_guard<std::mutex> lk(ix->mu);
    const bool half = ix->storage == Quantization_F16;
    if (rows_h && !half)
        throw std::runtime_error(
            "the index stores f32: f16 rows go to an index made with "
            "moann_bf_new_typed(Quantization_F16)");
    if (n == 0) return;
    if (!rows_f && !rows_h) throw std::runtime_error("null rows");
    if (n > (uint64_t)BF_MAX_ROWS)
        throw std::runtime_error("the index holds at most 2^31-1 rows");
    if (half) { /* on the host, before anything is stored or copied */
        const int64_t bad =
            rows_h ? first_nonfinite_half_row(rows_h, n, ix->dim)
                   : first_unhalfable_row(rows_f, n, ix->dim);
        if (bad >= 0)
            throw std::runtime_error(
                "row " + std::to_string(bad) +
                " of this add holds a value with no finite f16 value "
                "(|v| >= 65520, inf or NaN); nothing was added");
    }
    HIP_CHECK(hipSetDevice(ix->device));
    const int64_t ncap = bf_next_capacity(ix->cap, ix->len, (int64_t)n);
    if (ncap != ix->cap) grow(ix, ncap);
    const hipStream_t s = ix->stream;
    const int64_t l0 = ix->len;
    if (half) {
        upload_half_rows(ix, rows_f, rows_h, n);
    } else {
        const float* rows = rows_f;
        float* dst = (float*)ix->d_rows + (size_t)l0 * ix->dpad;
        if (ix->dim != ix->dpad)
            HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)n * ix->dpad * 4, s));
        HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ix->dpad * 4, rows,
                                   (size_t)ix->dim * 4,
                                   (size_t)ix->dim * 4, n,
                                   hipMemcpyHostToDevice, s));
        /* |x|^2 in chunks that keep launch_qnorms' int row count */
        for (uint64_t o = 0; o < n; o += (1u << 30)) {
            const int c = (int)std::min<uint64_t>(n - o, 1u << 30);
            launch_qnorms(dst + (size_t)o * ix->dpad, c, (int)ix->dpad,
                          ix->d_xn + l0 + o, s);
            KCHECK("bf row norms");
        }
    }
    std::vector<int64_t> seq;
    const int64_t* src = ids;
    if (!ids) {
        seq.resize(n);
        for (uint64_t i = 0; i < n; ++i) seq[i] = l0 + (int64_t)i;
        src = seq.data();
    }
    HIP_CHECK(hipMemcpyAsync(ix->d_ids + l0, src, (size_t)n * 8,
                             hipMemcpyHostToDevice, s));
    if (ids && ix->seq_ids) { /* first ids of the caller's own */
        for (int64_t r = 0; r < l0; ++r) ix->row_of_id.emplace(r, r);
        ix->seq_ids = false;
    }
    if (!ix->seq_ids)
        for (uint64_t i = 0; i < n; ++i)
            ix->row_of_id.emplace(src[i], l0 + (int64_t)i);
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = l0 + (int64_t)i;
        ix->h_alive[(size_t)(r >> 5)] |= 1u << (r & 31);
    }
    ix->alive_dirty = true;
    HIP_CHECK(hipStreamSynchronize(s)); /* `rows`, `seq` may go away */
    ix->len = l0 + (int64_t)n;
}

}  // namespace

extern "C" {

moann_bf_c moann_bf_new(uint32_t dimension, distance_type_t metric,
                        uint64_t capacity_hint, const int* devices,
                        int device_count, void* errmsg) {
    return bf_new("moann_bf_new", dimension, metric, Quantization_F32,
                  capacity_hint, devices, device_count, errmsg);
}

moann_bf_c moann_bf_new_typed(uint32_t dimension, distance_type_t metric,
                              quantization_t storage, uint64_t capacity_hint,
                              const int* devices, int device_count,
                              void* errmsg) {
    return bf_new("moann_bf_new_typed", dimension, metric, storage,
                  capacity_hint, devices, device_count, errmsg);
}

void moann_bf_add(moann_bf_c h, const float* rows, uint64_t n,
                  const int64_t* ids, void* errmsg) {
    guarded(errmsg, "moann_bf_add",
            [&] { add_rows(h, rows, nullptr, n, ids); });
}

void moann_bf_add_half(moann_bf_c h, const uint16_t* rows, uint64_t n,
                       const int64_t* ids, void* errmsg) {
    guarded(errmsg, "moann_bf_add_half", [&] {
        if (!rows && n) throw std::runtime_error("null rows");
        /* a non-null marker keeps the entry's identity for n = 0 */
        static const uint16_t none = 0;
        add_rows(h, nullptr, rows ? rows : &none, n, ids);
    });
}

void moann_bf_delete_id(moann_bf_c h, int64_t id, void* errmsg) {
    guarded(errmsg, "moann_bf_delete_id", [&] {
        auto ix = BX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        auto kill = [&](int64_t r) {
            ix->h_alive[(size_t)(r >> 5)] &= ~(1u << (r & 31));
            ix->any_deleted = true;
            ix->alive_dirty = true;
        };
        if (ix->seq_ids) {
            if (id >= 0 && id < ix->len) kill(id);
            return;
        }
        auto range = ix->row_of_id.equal_range(id);
        for (auto it = range.first; it != range.second; ++it)
            kill(it->second);
    });
}

void moann_bf_set_params(moann_bf_c h, uint32_t mode, uint32_t slice_rows,
                         void* errmsg) {
    guarded(errmsg, "moann_bf_set_params", [&] {
        auto ix = BX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (mode > (uint32_t)BF_GEMM)
            throw std::runtime_error(
                "mode must be 0 (auto), 1 (fused) or 2 (gemm)");
        if (slice_rows % (uint32_t)BF_TILE != 0)
            throw std::runtime_error(
                "slice_rows must be 0 or a multiple of the 128-row tile");
        ix->mode = (int)mode;
        ix->slice_rows = slice_rows;
    });
}

void moann_bf_search(moann_bf_c h, const float* queries, uint64_t nq,
                     uint32_t dim, uint32_t k, int64_t* out_ids,
                     float* out_dists, void* errmsg) {
    guarded(errmsg, "moann_bf_search", [&] {
        run_search(BX(h), queries, false, nq, dim, k, nullptr, 0, false,
                   out_ids, out_dists);
    });
}

void moann_bf_search_device(moann_bf_c h, const void* queries_dev, uint64_t nq,
                            uint32_t dim, uint32_t k, int64_t* out_ids,
                            float* out_dists, void* errmsg) {
    guarded(errmsg, "moann_bf_search_device", [&] {
        run_search(BX(h), (const float*)queries_dev, true, nq, dim, k, nullptr,
                   0, false, out_ids, out_dists);
    });
}

void moann_bf_search_filtered(moann_bf_c h, const float* queries, uint64_t nq,
                              uint32_t dim, uint32_t k,
                              const uint32_t* row_bitset, uint64_t nbits,
                              int64_t* out_ids, float* out_dists,
                              void* errmsg) {
    guarded(errmsg, "moann_bf_search_filtered", [&] {
        run_search(BX(h), queries, false, nq, dim, k, row_bitset, nbits, true,
                   out_ids, out_dists);
    });
}

uint64_t moann_bf_len(moann_bf_c h) { return h ? (uint64_t)((BfIndex*)h)->len : 0; }

uint32_t moann_bf_storage(moann_bf_c h) {
    return h ? (uint32_t)((BfIndex*)h)->storage : (uint32_t)Quantization_F32;
}

uint32_t moann_bf_fused_kmax(void) { return (uint32_t)BF_FUSED_KMAX; }

void moann_bf_perf(moann_bf_c h, moann_perf_t* out) {
    if (!h || !out) return;
    auto ix = (BfIndex*)h;
    std::lock_guard<std::mutex> lk(ix->mu);
    *out = ix->perf;
}

void moann_bf_destroy(moann_bf_c h, void* errmsg) {
    guarded(errmsg, "moann_bf_destroy", [&] { delete (BfIndex*)h; });
}

}  // extern "C"
