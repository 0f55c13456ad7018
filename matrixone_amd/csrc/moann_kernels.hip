/* CDNA4 (gfx950) device kernels for the MatrixOne ANN search hot path.
 *
 * Written MI355X-first (not a port): 64-wide wavefronts, coalesced
 * float4 streams over an interleaved HBM layout, LDS-staged query tiles,
 * per-query radix select. The list-scan kernel replaces the reference's
 * per-row SimSIMD distance loop (pkg/vectorindex/ivfflat/relation_search.go:
 * 334-368 + pkg/sql/plan/function/func_binary.go:9045-9175) and the cuVS
 * ivf_flat list-scan launch (cgo/cuvs/ivf_flat.hpp:921-945 precedent);
 * results follow MO's distance conventions (metric/distance_func.go:
 * IP = -x.q at :207, cosine clamp + denom-0 at :211-286).
 *
 * Data layout: vectors are packed per list into groups of 64 rows,
 * dim-major inside the group in float4 quads:
 *   packed[(g*dpad + 4*j4)*64 + lane*4 + c] = row(g*64+lane) dim(4*j4+c)
 * so one wave reading quad j4 for its 64 rows issues one fully coalesced
 * 1 KiB load (16 B/lane). Queries are tiled (QT<=8 per workgroup) in LDS and
 * broadcast-read, so each HBM byte of list data serves QT queries.
 */

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "moann_internal.h"
#include "moann_scan_device.h"
#include "moann_select_plan.h"

namespace moann {

#define WAVE 64

/* Run f with the metric as a compile-time constant:
 * f(std::integral_constant<int, KM_...>{}). */
template <typename F>
static void with_metric(int metric, F&& f) {
    switch (metric) {
    case KM_L2SQ: f(std::integral_constant<int, KM_L2SQ>{}); break;
    case KM_IP:   f(std::integral_constant<int, KM_IP>{}); break;
    case KM_COS:  f(std::integral_constant<int, KM_COS>{}); break;
    default:      f(std::integral_constant<int, KM_L1>{}); break;
    }
}

/* monotone float -> u32 key (ascending order preserved) */
__device__ __forceinline__ uint32_t f2u(float f) {
    uint32_t u = __float_as_uint(f);
    return u ^ (((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float u2f(uint32_t u) {
    u ^= (((int32_t)(u ^ 0x80000000u)) >> 31) | 0x80000000u;
    return __uint_as_float(u);
}

/* ------------------------------ scan -------------------------------------
 * One workgroup (256 threads = 4 waves) per job. Each wave walks a pair of
 * adjacent 64-row groups so every LDS broadcast of a query quad feeds two
 * 16 B data quads (halves LDS traffic per byte). Per j4 step and query:
 * 8 fma-class VALU ops per 32 B/lane -> VALU ceiling ~19 TB/s equivalent,
 * comfortably above the ~6.3 TB/s HBM bound this kernel targets. */
template <int METRIC, int QT>
__global__ __launch_bounds__(256) void scan_kernel(
    const float* __restrict__ packed, const float* __restrict__ queries,
    const float* __restrict__ qnorms, int dpad, const ScanJobs jobs,
    const uint32_t* __restrict__ filter_bitset, /* null = unfiltered */
    float* __restrict__ dists_out) {
    extern __shared__ float lds[];  /* [QT][dpad] (+[QT] qnorm for cos) */
    float* ldsq = lds;
    float* ldsn = lds + QT * dpad;

    const JobView jv = load_job(jobs);
    stage_query_tile<QT, METRIC == KM_COS>(jv, jobs.qslot_query, queries,
                                           qnorms, dpad, ldsq, ldsn);

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gend = jv.gstart + jv.gcount;
    const int d4 = dpad >> 2;

    /* each wave walks ADJACENT group pairs: one LDS broadcast feeds 32 B of
     * data */
    for (int g0 = jv.gstart + 2 * wave; g0 < gend; g0 += 8) {
        const bool has1 = (g0 + 1) < gend;
        const int g1 = has1 ? g0 + 1 : g0;
        const float4* __restrict__ d0 =
            (const float4*)(packed + (jv.baseg + g0) * (int64_t)64 * dpad) + lane;
        const float4* __restrict__ d1 =
            (const float4*)(packed + (jv.baseg + g1) * (int64_t)64 * dpad) + lane;

        float acc0[QT], acc1[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) acc0[t] = acc1[t] = 0.f;
        float rn0 = 0.f, rn1 = 0.f;

#pragma unroll 2 /* two iterations in flight: 4 dwordx4 issued together,
                    counted vmcnt waits */
        for (int q4 = 0; q4 < d4; ++q4) {
            const float4 x0 = d0[q4 * 64];
            const float4 x1 = d1[q4 * 64];
            if (METRIC == KM_COS) {
                rn0 += x0.x * x0.x + x0.y * x0.y + x0.z * x0.z + x0.w * x0.w;
                rn1 += x1.x * x1.x + x1.y * x1.y + x1.z * x1.z + x1.w * x1.w;
            }
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const float4 qv = ((const float4*)(ldsq + t * dpad))[q4];
                if (METRIC == KM_L2SQ) {
                    float e;
                    e = x0.x - qv.x; acc0[t] = fmaf(e, e, acc0[t]);
                    e = x0.y - qv.y; acc0[t] = fmaf(e, e, acc0[t]);
                    e = x0.z - qv.z; acc0[t] = fmaf(e, e, acc0[t]);
                    e = x0.w - qv.w; acc0[t] = fmaf(e, e, acc0[t]);
                    e = x1.x - qv.x; acc1[t] = fmaf(e, e, acc1[t]);
                    e = x1.y - qv.y; acc1[t] = fmaf(e, e, acc1[t]);
                    e = x1.z - qv.z; acc1[t] = fmaf(e, e, acc1[t]);
                    e = x1.w - qv.w; acc1[t] = fmaf(e, e, acc1[t]);
                } else if (METRIC == KM_IP || METRIC == KM_COS) {
                    acc0[t] = fmaf(x0.x, qv.x, acc0[t]);
                    acc0[t] = fmaf(x0.y, qv.y, acc0[t]);
                    acc0[t] = fmaf(x0.z, qv.z, acc0[t]);
                    acc0[t] = fmaf(x0.w, qv.w, acc0[t]);
                    acc1[t] = fmaf(x1.x, qv.x, acc1[t]);
                    acc1[t] = fmaf(x1.y, qv.y, acc1[t]);
                    acc1[t] = fmaf(x1.z, qv.z, acc1[t]);
                    acc1[t] = fmaf(x1.w, qv.w, acc1[t]);
                } else { /* KM_L1 */
                    acc0[t] += fabsf(x0.x - qv.x) + fabsf(x0.y - qv.y) +
                               fabsf(x0.z - qv.z) + fabsf(x0.w - qv.w);
                    acc1[t] += fabsf(x1.x - qv.x) + fabsf(x1.y - qv.y) +
                               fabsf(x1.z - qv.z) + fabsf(x1.w - qv.w);
                }
            }
        }

        store_group_pair<QT, METRIC == KM_COS>(
            jobs, jv, lane, g0, g1, has1, acc0, acc1, rn0, rn1, ldsn,
            filter_bitset, dists_out, [](float acc, float rn, float qn) {
                return finish_f32<METRIC>(acc, rn, qn);
            });
    }
}

/* planner/launcher disagreement (the bug class that leaves tile lanes
 * unscanned): reported by name, before anything is enqueued */
[[noreturn]] static void bad_variant(const char* launcher, ScanVariant v) {
    throw std::logic_error(std::string(launcher) + ": no kernel for scan " +
                           scan_kind_name(v.kind) + " qt=" +
                           std::to_string(v.qt));
}

void launch_scan(int metric, ScanVariant v, const float* packed,
                 const float* queries, const float* qnorms, int dpad,
                 const ScanJobs& jb, float* dists_out, hipStream_t stream,
                 const uint32_t* filter_bitset) {
    const int qt = v.qt;
    const bool asm768 = v.kind == ScanKind::F32_ASM768 && qt == 16 &&
                        metric == KM_L2SQ && dpad == 768;
    const bool generic = v.kind == ScanKind::F32 &&
                         (qt == 8 || qt == 4 || qt == 2 || qt == 1);
    if (!asm768 && !generic) bad_variant("launch_scan", v);
    if (jb.njobs == 0) return;
    if (asm768) { /* flagship shape: hand-scheduled kernel (scan_asm768.hip) */
        launch_scan_asm768(packed, queries, dpad, jb, dists_out, stream,
                           filter_bitset);
        return;
    }
    with_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const dim3 grid(jb.njobs), block(256);
        const size_t shmem = (size_t)(qt * dpad + qt) * sizeof(float);
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, packed,
                               queries, qnorms, dpad, jb, filter_bitset,
                               dists_out);
        };
        switch (qt) { /* only the four widths admitted above */
        case 8:  launch(scan_kernel<M, 8>); break;
        case 4:  launch(scan_kernel<M, 4>); break;
        case 2:  launch(scan_kernel<M, 2>); break;
        default: launch(scan_kernel<M, 1>); break;
        }
    });
}

/* ------------------------------ top-k ------------------------------------
 * One workgroup per query: 4-level 8-bit radix select over the monotone u32
 * keys (exact kth threshold), then gather of the k winners and an in-LDS
 * bitonic sort of packed (key32|slot32) u64s — ascending by distance, slot as
 * the tie-breaker, giving deterministic output. k <= 4096.
 * Replaces the bounded heaps of pkg/vectorindex/index.go:135-309 and the
 * cuVS select::topk stage. Padding: (-1, FLT_MAX) per cgo/cuvs/helper.h:160. */
/* LDS of one radix-select block: 2 KiB of histogram and state, then the sort
 * buffer */
__host__ __device__ constexpr size_t topk_radix_lds(int sortP) {
    return 2048 + (size_t)sortP * 8;
}

/* Tail of every block select: keys[0, nkeys) hold the collected
 * (key << 32 | index) pairs, P >= nkeys is a power of two within the buffer.
 * Pads to P, sorts ascending and writes the first m <= k entries of row q,
 * (-1, FLT_MAX) behind them. Called by every thread of the block. */
__device__ __forceinline__ void topk_sort_write(
    uint64_t* keys, int nkeys, int P, int m, int q, int k,
    int32_t* __restrict__ out_slots, float* __restrict__ out_dists) {
    const int tid = threadIdx.x;
    for (int i = nkeys + tid; i < P; i += blockDim.x) keys[i] = ~0ULL;
    __syncthreads();

    /* bitonic sort ascending over P u64 keys */
    for (int ks = 2; ks <= P; ks <<= 1) {
        for (int jj = ks >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P; i += blockDim.x) {
                const int l = i ^ jj;
                if (l > i) {
                    const uint64_t a = keys[i], b = keys[l];
                    const bool up = (i & ks) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    }

    for (int i = tid; i < k; i += blockDim.x) {
        if (i < m) {
            const uint64_t kv = keys[i];
            out_slots[(int64_t)q * k + i] = (int32_t)(kv & 0xFFFFFFFFu);
            out_dists[(int64_t)q * k + i] = u2f((uint32_t)(kv >> 32));
        } else {
            out_slots[(int64_t)q * k + i] = -1;
            out_dists[(int64_t)q * k + i] = FLT_MAX;
        }
    }
}

/* One block's radix select of row q = dists[off, off+count) into row q of
 * the outputs; smem holds topk_radix_lds(sortP) bytes and needs no set-up.
 * Called by every thread of the block: topk_kernel's whole body, and the
 * fallback of select_filter_kernel. */
__device__ __forceinline__ void topk_radix_block(
    const float* __restrict__ dists, int64_t off, int64_t count, int q, int k,
    int sortP, unsigned char* smem, int32_t* __restrict__ out_slots,
    float* __restrict__ out_dists) {
    uint32_t* hist = (uint32_t*)smem;                    /* 256 */
    uint32_t* ctr = hist + 256;                          /* n_lt, n_tie */
    uint32_t* st = ctr + 8;  /* prefix, c_sure, tieval, need_ties, done */
    uint64_t* keys = (uint64_t*)(smem + 2048);           /* [sortP] */

    const int tid = threadIdx.x;
    const int m = (int)(count < (int64_t)k ? count : k);
    int nkeys;

    if (count > (int64_t)k) {
        /* radix select for the exact threshold. Each full-array read is
         * 4x unrolled so every wave keeps 4 loads in flight (a single
         * strided scalar load per wave is latency-bound at ~1.3 TB/s;
         * measured r01_fetch_10M_asm_cg8.csv). */
        if (tid == 0) { st[0] = 0; st[1] = 0; st[3] = 0; st[4] = 0; st[5] = 0; }
        __syncthreads();
        for (int level = 0; level < 4 && !st[4]; ++level) {
            const int shift = 24 - 8 * level;
            for (int b = tid; b < 256; b += blockDim.x) hist[b] = 0;
            __syncthreads();
            const uint32_t pref = st[0];
            const int64_t step = blockDim.x;
            int64_t i = tid;
#define MOANN_HISTO(u)                                                                  if (level == 0 || ((u) >> (shift + 8)) == (pref >> (shift + 8)))                atomicAdd(&hist[((u) >> shift) & 255], 1u);
            for (; i + 3 * step < count; i += 4 * step) {
                const uint32_t u0 = f2u(dists[off + i]);
                const uint32_t u1 = f2u(dists[off + i + step]);
                const uint32_t u2 = f2u(dists[off + i + 2 * step]);
                const uint32_t u3 = f2u(dists[off + i + 3 * step]);
                MOANN_HISTO(u0) MOANN_HISTO(u1) MOANN_HISTO(u2) MOANN_HISTO(u3)
            }
            for (; i < count; i += step) {
                const uint32_t u = f2u(dists[off + i]);
                MOANN_HISTO(u)
            }
#undef MOANN_HISTO
            __syncthreads();
            if (tid == 0) {
                const uint32_t need = (uint32_t)k - st[1];
                uint32_t cum = 0; int b = 0;
                for (; b < 256; ++b) {
                    if (cum + hist[b] >= need) break;
                    cum += hist[b];
                }
                st[0] = pref | ((uint32_t)b << shift);
                st[1] += cum;
                if (cum + hist[b] == need) {
                    /* whole bin selected: no tie resolution needed */
                    st[1] += hist[b];
                    st[0] |= (shift ? ((1u << shift) - 1u) : 0u);
                    st[3] = 0; st[4] = 1;
                } else if (st[1] + hist[b] <= (uint32_t)sortP) {
                    /* boundary GROUP fits in the sort buffer: collect the
                     * whole prefix group and let the bitonic sort truncate.
                     * Exact (every candidate strictly below the group is
                     * kept) and deterministic (full keys are distinct), and
                     * it usually ends the scan at level 0 or 1 instead of
                     * re-reading the array for levels 2-3. */
                    st[2] = st[0];
                    st[3] = hist[b];
                    st[5] = (uint32_t)shift;
                    st[4] = 1;
                } else if (level == 3) {
                    st[2] = st[0];
                    st[3] = need - cum;
                    st[5] = 0;
                }
            }
            __syncthreads();
        }
        const uint32_t c_sure = st[1];
        const uint32_t tieval = st[2];
        const uint32_t need_ties = st[3];
        const uint32_t tie_shift = st[5];
        const int exact = st[4] && !need_ties;
        /* strict-below bound: exact-exit keeps everything <= prefix (low
         * bits already forced to 1); group/tie modes keep u < prefix (low
         * bits zero, so < excludes the whole boundary group) */
        const uint64_t below = (uint64_t)st[0] + (exact ? 1u : 0u);
        if (tid == 0) { ctr[0] = 0; ctr[1] = 0; }
        __syncthreads();
        {
            const int64_t step = blockDim.x;
            int64_t i = tid;
#define MOANN_COLLECT(u, idx)                                                           if ((uint64_t)(u) < below) {                                                    const uint32_t pos = atomicAdd(&ctr[0], 1u);                                keys[pos] = ((uint64_t)(u) << 32) | (uint32_t)(idx);                    } else if (need_ties &&                                                                ((u) >> tie_shift) == (tieval >> tie_shift)) {                       const uint32_t t = atomicAdd(&ctr[1], 1u);                                  if (t < need_ties)                                                              keys[c_sure + t] = ((uint64_t)(u) << 32) | (uint32_t)(idx);             }
            for (; i + 3 * step < count; i += 4 * step) {
                const uint32_t u0 = f2u(dists[off + i]);
                const uint32_t u1 = f2u(dists[off + i + step]);
                const uint32_t u2 = f2u(dists[off + i + 2 * step]);
                const uint32_t u3 = f2u(dists[off + i + 3 * step]);
                MOANN_COLLECT(u0, i) MOANN_COLLECT(u1, i + step)
                MOANN_COLLECT(u2, i + 2 * step) MOANN_COLLECT(u3, i + 3 * step)
            }
            for (; i < count; i += step) {
                const uint32_t u = f2u(dists[off + i]);
                MOANN_COLLECT(u, i)
            }
#undef MOANN_COLLECT
        }
        __syncthreads();
        nkeys = (int)(c_sure + need_ties);
    } else {
        for (int64_t i = tid; i < count; i += blockDim.x)
            keys[i] = ((uint64_t)f2u(dists[off + i]) << 32) | (uint32_t)i;
        __syncthreads();
        nkeys = m;
    }

    /* pad from the number of COLLECTED keys (group-collect gathers up to
     * sortP entries, more than k) and let the sort truncate to k */
    topk_sort_write(keys, nkeys, sortP, m, q, k, out_slots, out_dists);
}

__global__ __launch_bounds__(256) void topk_kernel(
    const float* __restrict__ dists, const int64_t* __restrict__ qoffs,
    int64_t uniform_n, int k, int sortP,
    int32_t* __restrict__ out_slots, float* __restrict__ out_dists) {
    extern __shared__ unsigned char smem[];
    const int q = blockIdx.x;
    const int64_t off = qoffs ? qoffs[q] : (int64_t)q * uniform_n;
    const int64_t count = (qoffs ? qoffs[q + 1] : (int64_t)(q + 1) * uniform_n) - off;
    topk_radix_block(dists, off, count, q, k, sortP, smem, out_slots,
                     out_dists);
}

/* ---------------- threshold-filter select for long ragged rows -----------
 * The k smallest of a long row in ONE read (rule and constants:
 * moann_select_plan.h). One block per row:
 *  1. sample: m keys in runs spread evenly over the whole row (the candidate
 *     buffer is ordered by probe rank, a prefix is no sample), one run of 16
 *     per thread, kept in registers; the key of rank t among them, found by a bitwise
 *     binary search on counts, is the threshold;
 *  2. one pass of 16-byte loads, four in flight per thread; a key <= thr is
 *     appended to the LDS buffer through one LDS counter (hits are under 1 %
 *     of the row, so the counter is not contended);
 *  3. >= k collected and no more than the capacity: sort them, write k. Any
 *     other outcome runs topk_radix_block on the row: a bad threshold costs
 *     time, never the result.
 * Rows the plan does not admit (short, or k > SELECT_KMAX) go straight to
 * the radix function. stats[0] counts filtered rows, stats[1] fallen-back
 * ones. Output: the k smallest by (key, index), as topk_kernel. */
__device__ __forceinline__ void select_hit(uint32_t u, uint32_t thr,
                                           int64_t idx, uint32_t* cnt,
                                           uint64_t* keys) {
    if (u <= thr) {
        const uint32_t pos = atomicAdd(cnt, 1u);
        if (pos < (uint32_t)SELECT_CAPACITY)
            keys[pos] = ((uint64_t)u << 32) | (uint32_t)idx;
    }
}

__global__ __launch_bounds__(SELECT_THREADS) void select_filter_kernel(
    const float* __restrict__ dists, const int64_t* __restrict__ qoffs,
    int k, int sortP, int32_t* __restrict__ out_slots,
    float* __restrict__ out_dists, unsigned long long* __restrict__ stats) {
    extern __shared__ unsigned char smem[];
    /* the radix function's layout, so the fallback reuses the same bytes:
     * words of the first 2 KiB, then the key buffer */
    uint32_t* cnt = (uint32_t*)smem;          /* collected keys            */
    constexpr int NWAVES = SELECT_THREADS / WAVE;
    static_assert(SELECT_THREADS % WAVE == 0 && 4 + 2 * NWAVES <= 512,
                  "per-wave counts live in the 2 KiB state area");
    uint32_t* wsum = cnt + 4;                 /* [2][NWAVES] wave counts   */
    uint64_t* keys = (uint64_t*)(smem + 2048);/* [SELECT_CAPACITY]         */

    const int q = blockIdx.x;
    const int64_t off = qoffs[q];
    const int64_t count = qoffs[q + 1] - off;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const SelectPlan plan = select_plan(count, k);
    const float* row = dists + off;
    bool radix = !plan.filter; /* block-uniform, like all that follows */
    if (plan.filter) {
        /* 1. sample -> threshold */
        constexpr int SPT = SELECT_SAMPLE / SELECT_THREADS;
        static_assert(SPT == SELECT_CLUSTER, "one sampled run per thread");
        uint32_t s[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j)
            s[j] = f2u(row[select_sample_pos(count, SELECT_SAMPLE,
                                             tid * SPT + j)]);
        if (tid == 0) *cnt = 0;
        /* thr = t-th smallest sample = the largest v with #(s < v) < t,
         * built from the top bit down; one barrier per bit, on alternating
         * slots */
        uint32_t thr = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = thr | (1u << bit);
            int c = 0;
#pragma unroll
            for (int j = 0; j < SPT; ++j) c += s[j] < cand;
            for (int o = 32; o; o >>= 1) c += __shfl_down(c, o, 64);
            uint32_t* slot = wsum + NWAVES * (bit & 1);
            if (lane == 0) slot[wave] = (uint32_t)c;
            __syncthreads();
            uint32_t below = 0;
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) below += slot[w];
            if (below < (uint32_t)plan.t) thr = cand;
        }

        /* 2. one pass: scalar head up to 16-byte alignment, float4 body,
         * scalar tail. dists is 16-byte aligned (a device allocation), off
         * is not. */
        int64_t head = (4 - (off & 3)) & 3;
        if (head > count) head = count;
        const int64_t nvec = (count - head) >> 2;
        const int64_t tail0 = head + 4 * nvec;
        if (tid < head) select_hit(f2u(row[tid]), thr, tid, cnt, keys);
        if (tail0 + tid < count)
            select_hit(f2u(row[tail0 + tid]), thr, tail0 + tid, cnt, keys);
        const float4* body = (const float4*)(row + head);
#define MOANN_SEL4(v, vi)                                                   \
    select_hit(f2u((v).x), thr, head + 4 * (vi), cnt, keys);                \
    select_hit(f2u((v).y), thr, head + 4 * (vi) + 1, cnt, keys);            \
    select_hit(f2u((v).z), thr, head + 4 * (vi) + 2, cnt, keys);            \
    select_hit(f2u((v).w), thr, head + 4 * (vi) + 3, cnt, keys);
        int64_t i = tid;
        const int64_t step = SELECT_THREADS;
        for (; i + 3 * step < nvec; i += 4 * step) {
            const float4 v0 = body[i], v1 = body[i + step];
            const float4 v2 = body[i + 2 * step], v3 = body[i + 3 * step];
            MOANN_SEL4(v0, i) MOANN_SEL4(v1, i + step)
            MOANN_SEL4(v2, i + 2 * step) MOANN_SEL4(v3, i + 3 * step)
        }
        for (; i < nvec; i += step) {
            const float4 v = body[i];
            MOANN_SEL4(v, i)
        }
#undef MOANN_SEL4
        __syncthreads();

        /* 3. finish (count >= SELECT_MIN_COUNT > k here) */
        const uint32_t got = *cnt;
        radix = got < (uint32_t)k || got > (uint32_t)SELECT_CAPACITY;
        if (tid == 0) atomicAdd(&stats[radix ? 1 : 0], 1ull);
        if (!radix) {
            int P = 1;
            while (P < (int)got) P <<= 1;
            topk_sort_write(keys, (int)got, P, k, q, k, out_slots, out_dists);
        }
        __syncthreads(); /* every thread has read cnt */
    }
    if (radix)
        topk_radix_block(dists, off, count, q, k, sortP, smem, out_slots,
                         out_dists);
}

/* sort buffer of the radix select for this k */
static int topk_sort_size(int k) {
    int sortP = 1;
    while (sortP < k) sortP <<= 1;
    /* A larger sort buffer makes the group-collect exit fire at level 0
     * (strict-below <= k plus a ~count/256 boundary group): 2 full-array
     * reads instead of 3 for the big per-query candidate selections. The
     * extra bitonic work (1024 u64 keys) is microseconds per block; LDS
     * 2048+8*1024 = 10 KB still keeps several blocks per CU. */
    return sortP < 1024 ? 1024 : sortP;
}

void launch_topk(const float* dists, const int64_t* qoffs, int64_t uniform_n,
                 int nq, int k, int32_t* out_slots, float* out_dists,
                 hipStream_t stream) {
    if (nq == 0) return;
    const int sortP = topk_sort_size(k);
    hipLaunchKernelGGL(topk_kernel, dim3(nq), dim3(256),
                       topk_radix_lds(sortP), stream, dists, qoffs, uniform_n,
                       k, sortP, out_slots, out_dists);
}

void launch_select(const float* dists, const int64_t* qoffs, int nq, int k,
                   int32_t* out_slots, float* out_dists,
                   unsigned long long* stats, hipStream_t stream) {
    if (nq == 0) return;
    const int sortP = topk_sort_size(k);
    /* 18 KiB at k <= SELECT_KMAX: eight blocks per CU */
    const size_t shmem = std::max(topk_radix_lds(sortP),
                                  topk_radix_lds(SELECT_CAPACITY));
    hipLaunchKernelGGL(select_filter_kernel, dim3(nq), dim3(SELECT_THREADS),
                       shmem, stream, dists, qoffs, k, sortP, out_slots,
                       out_dists, stats);
}

/* ------------------------------ gather ----------------------------------- */

__device__ __forceinline__ float transform_score_dev(float raw, int do_sqrt,
                                                     double inv_mul2) {
    /* ivfflat/search.go:1062-1077 + metric/types.go:245-251 */
    double r = (double)raw * inv_mul2;
    if (do_sqrt) r = sqrt(r);
    return (float)r;
}

__global__ void gather_kernel(
    const int32_t* __restrict__ sel_slots, const float* __restrict__ sel_dists,
    const int32_t* __restrict__ probe_lists, const int64_t* __restrict__ probe_offs,
    const int64_t* __restrict__ list_slot_base, const int64_t* __restrict__ id_by_slot,
    int nprobe, int nq, int k, int do_sqrt, double inv_mul2,
    int64_t* __restrict__ out_ids, float* __restrict__ out_dists) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nq * k) return;
    const int q = (int)(idx / k);
    const int32_t slot = sel_slots[idx];
    /* FLT_MAX marks padding AND membership-filtered rows */
    if (slot < 0 || sel_dists[idx] == FLT_MAX) {
        out_ids[idx] = -1; out_dists[idx] = FLT_MAX; return;
    }
    /* binary search rank r: probe_offs[q][r] <= slot < probe_offs[q][r+1] */
    const int64_t* offs = probe_offs + (int64_t)q * (nprobe + 1);
    int lo = 0, hi = nprobe - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= slot) lo = mid; else hi = mid - 1;
    }
    const int32_t list = probe_lists[(int64_t)q * nprobe + lo];
    const int64_t local = slot - offs[lo];
    out_ids[idx] = id_by_slot[list_slot_base[list] + local];
    out_dists[idx] = transform_score_dev(sel_dists[idx], do_sqrt, inv_mul2);
}

void launch_gather(const int32_t* sel_slots, const float* sel_dists,
                   const int32_t* probe_lists, const int64_t* probe_offs,
                   const int64_t* list_slot_base, const int64_t* id_by_slot,
                   int nprobe, int nq, int k, int do_sqrt, double inv_mul2,
                   int64_t* out_ids, float* out_dists, hipStream_t stream) {
    const int64_t total = (int64_t)nq * k;
    if (!total) return;
    const int block = 256;
    const int grid = (int)((total + block - 1) / block);
    hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(block), 0, stream,
                       sel_slots, sel_dists, probe_lists, probe_offs,
                       list_slot_base, id_by_slot, nprobe, nq, k, do_sqrt,
                       inv_mul2, out_ids, out_dists);
}

__global__ void gather_uniform_kernel(
    const int32_t* __restrict__ sel_slots, const float* __restrict__ sel_dists,
    const int64_t* __restrict__ id_by_slot, int nq, int k, int do_sqrt,
    double inv_mul2, int64_t* __restrict__ out_ids,
    float* __restrict__ out_dists) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nq * k) return;
    const int32_t slot = sel_slots[idx];
    if (slot < 0) { out_ids[idx] = -1; out_dists[idx] = FLT_MAX; return; }
    out_ids[idx] = id_by_slot ? id_by_slot[slot] : (int64_t)slot;
    out_dists[idx] = transform_score_dev(sel_dists[idx], do_sqrt, inv_mul2);
}

void launch_gather_uniform(const int32_t* sel_slots, const float* sel_dists,
                           const int64_t* id_by_slot, int nq, int k,
                           int do_sqrt, double inv_mul2, int64_t* out_ids,
                           float* out_dists, hipStream_t stream) {
    const int64_t total = (int64_t)nq * k;
    if (!total) return;
    const int block = 256;
    const int grid = (int)((total + block - 1) / block);
    hipLaunchKernelGGL(gather_uniform_kernel, dim3(grid), dim3(block), 0,
                       stream, sel_slots, sel_dists, id_by_slot, nq, k,
                       do_sqrt, inv_mul2, out_ids, out_dists);
}

/* ------------------------------ pack -------------------------------------
 * One-time permutation into the interleaved layout: thread = one output
 * float4; writes coalesced, reads gather (4 B x 4 from the source row). */
__global__ void pack_kernel(const float* __restrict__ vecs, int dim, int dpad,
                            const int64_t* __restrict__ group_rowbase,
                            const int32_t* __restrict__ group_valid,
                            const int64_t* __restrict__ slot_rows,
                            int64_t ngroups, float* __restrict__ packed) {
    const int64_t nquads = ngroups * (dpad >> 2) * 64;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < nquads; idx += stride) {
        const int lane = (int)(idx & 63);
        const int64_t rest = idx >> 6;
        const int j4 = (int)(rest % (dpad >> 2));
        const int64_t g = rest / (dpad >> 2);
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (lane < group_valid[g]) {
            const int64_t row = slot_rows[group_rowbase[g] + lane];
            const float* src = vecs + row * (int64_t)dim;
            const int base = 4 * j4;
            v.x = base + 0 < dim ? src[base + 0] : 0.f;
            v.y = base + 1 < dim ? src[base + 1] : 0.f;
            v.z = base + 2 < dim ? src[base + 2] : 0.f;
            v.w = base + 3 < dim ? src[base + 3] : 0.f;
        }
        ((float4*)packed)[idx] = v;
    }
}

void launch_pack(const float* vecs, int dim, int dpad,
                 const int64_t* group_rowbase, const int32_t* group_valid,
                 const int64_t* slot_rows, int64_t ngroups, float* packed,
                 hipStream_t stream) {
    const int64_t nquads = ngroups * (int64_t)(dpad >> 2) * 64;
    if (!nquads) return;
    const int block = 256;
    const int64_t grid = std::min<int64_t>((nquads + block - 1) / block,
                                           1 << 22);
    hipLaunchKernelGGL(pack_kernel, dim3((uint32_t)grid), dim3(block), 0,
                       stream, vecs, dim, dpad, group_rowbase, group_valid,
                       slot_rows, ngroups, packed);
}

/* ------------------------------ unpack -----------------------------------
 * Inverse of pack_kernel for save_dir: packed groups -> row-major f32 rows
 * in SLOT order (valid slots only), one chunk of slots at a time. */
__global__ void unpack_kernel(const float* __restrict__ packed, int dim,
                              int dpad,
                              const int64_t* __restrict__ group_slotbase,
                              const int32_t* __restrict__ group_valid,
                              int64_t ngroups, int64_t slot_lo,
                              int64_t slot_hi, float* __restrict__ out) {
    const int64_t nquads = ngroups * (dpad >> 2) * 64;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < nquads; idx += stride) {
        const int lane = (int)(idx & 63);
        const int64_t rest = idx >> 6;
        const int j4 = (int)(rest % (dpad >> 2));
        const int64_t g = rest / (dpad >> 2);
        if (lane >= group_valid[g]) continue;
        const int64_t slot = group_slotbase[g] + lane;
        if (slot < slot_lo || slot >= slot_hi) continue;
        const float4 v = ((const float4*)packed)[idx];
        float* dst = out + (slot - slot_lo) * (int64_t)dim;
        const int base = 4 * j4;
        if (base + 0 < dim) dst[base + 0] = v.x;
        if (base + 1 < dim) dst[base + 1] = v.y;
        if (base + 2 < dim) dst[base + 2] = v.z;
        if (base + 3 < dim) dst[base + 3] = v.w;
    }
}

void launch_unpack(const float* packed, int dim, int dpad,
                   const int64_t* group_slotbase, const int32_t* group_valid,
                   int64_t ngroups, int64_t slot_lo, int64_t slot_hi,
                   float* out, hipStream_t stream) {
    const int64_t nquads = ngroups * (int64_t)(dpad >> 2) * 64;
    if (!nquads) return;
    const int block = 256;
    const int64_t grid = std::min<int64_t>((nquads + block - 1) / block,
                                           1 << 22);
    hipLaunchKernelGGL(unpack_kernel, dim3((uint32_t)grid), dim3(block), 0,
                       stream, packed, dim, dpad, group_slotbase, group_valid,
                       ngroups, slot_lo, slot_hi, out);
}

/* byte-storage inverse of pack: packed bytes -> row-major [slot][dim]
 * bytes, both layouts (layout16 = [g][dpad/16][64][16] when dpad%16==0,
 * else the uchar4 [g][dpad/4][64][4]). save_dir for narrow storage. */
template <bool L16>
__global__ void unpack_bytes_kernel(const uint8_t* __restrict__ packed,
                                    int dim, int dpad,
                                    const int64_t* __restrict__ group_slotbase,
                                    const int32_t* __restrict__ group_valid,
                                    int64_t ngroups, int64_t slot_lo,
                                    int64_t slot_hi,
                                    uint8_t* __restrict__ out) {
    const int U = L16 ? 16 : 4;
    const int64_t nunits = ngroups * (int64_t)(dpad / U) * 64;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < nunits; idx += stride) {
        const int lane = (int)(idx & 63);
        const int64_t rest = idx >> 6;
        const int m = (int)(rest % (dpad / U));
        const int64_t g = rest / (dpad / U);
        if (lane >= group_valid[g]) continue;
        const int64_t slot = group_slotbase[g] + lane;
        if (slot < slot_lo || slot >= slot_hi) continue;
        const uint8_t* src = packed + idx * U;
        uint8_t* dst = out + (slot - slot_lo) * (int64_t)dim;
        const int base = m * U;
#pragma unroll
        for (int b = 0; b < U; ++b)
            if (base + b < dim) dst[base + b] = src[b];
    }
}

void launch_unpack_bytes(const uint8_t* packed, int dim, int dpad,
                         const int64_t* group_slotbase,
                         const int32_t* group_valid, int64_t ngroups,
                         int64_t slot_lo, int64_t slot_hi, uint8_t* out,
                         hipStream_t stream) {
    const bool l16 = (dpad & 15) == 0;
    const int U = l16 ? 16 : 4;
    const int64_t nunits = ngroups * (int64_t)(dpad / U) * 64;
    if (!nunits) return;
    const int block = 256;
    const int64_t grid = std::min<int64_t>((nunits + block - 1) / block,
                                           1 << 22);
    if (l16)
        hipLaunchKernelGGL(unpack_bytes_kernel<true>, dim3((uint32_t)grid),
                           dim3(block), 0, stream, packed, dim, dpad,
                           group_slotbase, group_valid, ngroups, slot_lo,
                           slot_hi, out);
    else
        hipLaunchKernelGGL(unpack_bytes_kernel<false>, dim3((uint32_t)grid),
                           dim3(block), 0, stream, packed, dim, dpad,
                           group_slotbase, group_valid, ngroups, slot_lo,
                           slot_hi, out);
}

/* ---------------- half-precision (f16 / bf16) storage -------------------
 * MO's float16/bf16 quantization is a PLAIN CAST (quantizer.go:50-58,
 * CastSQL:179-183): entries and the query are narrowed with
 * round-to-nearest-even (float16.go:53-63 BF16FromFloat32 incl. its NaN
 * rule; f32bitsToF16bits:114-160 == IEEE RTNE, which v_cvt_f16_f32
 * implements) and distances decode back to f32 and accumulate in f32
 * (distance_func_narrow.go:27-52). Layout: 16-byte units of u16 elements
 * ([g][dpad/8][64][8 halves]); dpad is padded to a multiple of 8 for
 * half-typed indexes. */

__device__ __forceinline__ float moann_h2f(uint16_t b) {
    __half_raw r;
    r.x = b;
    return __half2float((__half)r);
}
__device__ __forceinline__ float moann_bf2f(uint16_t b) {
    return __uint_as_float((uint32_t)b << 16);
}
__device__ __forceinline__ uint16_t moann_f2h(float f) {
    __half_raw r = (__half_raw)__float2half(f); /* RTNE */
    return r.x;
}
__device__ __forceinline__ uint16_t moann_f2bf(float f) {
    const uint32_t x = __float_as_uint(f);
    if (((x >> 23) & 0xff) == 0xff && (x & 0x7fffff))
        return (uint16_t)((x >> 16) | 0x0040); /* quiet the NaN */
    return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1)) >> 16);
}

/* f32 rows -> u16 rows (pad columns 0); mirrors quantize_rows_kernel */
template <bool BF>
__global__ void quantize_half_rows_kernel(const float* __restrict__ in,
                                          int64_t nrows, int in_stride,
                                          int dim, int dpad,
                                          uint16_t* __restrict__ out) {
    const int64_t total = nrows * (int64_t)dpad;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x; /* see
        quantize_rows_kernel: 32-bit work-item grids */
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int64_t r = idx / dpad;
        const int c = (int)(idx % dpad);
        uint16_t v = 0;
        if (c < dim) {
            const float x = in[r * (int64_t)in_stride + c];
            v = BF ? moann_f2bf(x) : moann_f2h(x);
        }
        out[idx] = v;
    }
}

void launch_quantize_half_rows(bool bf, const float* in, int64_t nrows,
                               int in_stride, int dim, int dpad,
                               uint16_t* out, hipStream_t stream) {
    const int64_t total = nrows * (int64_t)dpad;
    if (!total) return;
    const int64_t grid = std::min<int64_t>((total + 255) / 256, 1 << 22);
    if (bf)
        hipLaunchKernelGGL(quantize_half_rows_kernel<true>,
                           dim3((uint32_t)grid), dim3(256), 0, stream, in,
                           nrows, in_stride, dim, dpad, out);
    else
        hipLaunchKernelGGL(quantize_half_rows_kernel<false>,
                           dim3((uint32_t)grid), dim3(256), 0, stream, in,
                           nrows, in_stride, dim, dpad, out);
}

/* |q|^2 over DECODED query halves (cosine denominators) */
template <bool BF>
__global__ void qnorms_h_kernel(const uint16_t* __restrict__ q, int nq,
                                int dpad, float* __restrict__ out) {
    const int i = blockIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x >= 64 || i >= nq) return;
    float acc = 0.f;
    for (int t = lane; t < dpad; t += 64) {
        const float x = BF ? moann_bf2f(q[(int64_t)i * dpad + t])
                           : moann_h2f(q[(int64_t)i * dpad + t]);
        acc = fmaf(x, x, acc);
    }
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) out[i] = acc;
}

void launch_qnorms_h(bool bf, const uint16_t* q, int nq, int dpad, float* out,
                     hipStream_t stream) {
    if (!nq) return;
    if (bf)
        hipLaunchKernelGGL(qnorms_h_kernel<true>, dim3(nq), dim3(64), 0,
                           stream, q, nq, dpad, out);
    else
        hipLaunchKernelGGL(qnorms_h_kernel<false>, dim3(nq), dim3(64), 0,
                           stream, q, nq, dpad, out);
}

/* half-storage list scan: dwordx4 = 8 halves/lane per step, decoded to
 * f32, same job/filter/output semantics as the other scans. QT=8. */
template <int METRIC, bool BF>
__global__ __launch_bounds__(256) void scan_h_kernel(
    const uint16_t* __restrict__ packed, const uint16_t* __restrict__ queries_h,
    const float* __restrict__ qnorms, int dpad, const ScanJobs jobs,
    const uint32_t* __restrict__ filter_bitset,
    float* __restrict__ dists_out) {
    constexpr int QT = 8;
    extern __shared__ float ldsf[];
    uint16_t* ldsq = (uint16_t*)ldsf;           /* [QT][dpad] halves */
    float* ldsn = (float*)(ldsq + QT * dpad);

    const JobView jv = load_job(jobs);
    stage_query_tile<QT, METRIC == KM_COS>(jv, jobs.qslot_query, queries_h,
                                           qnorms, dpad, ldsq, ldsn);

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gend = jv.gstart + jv.gcount;
    const int d8 = dpad >> 3;

#define MOANN_H8(w, out0, out1)                                                  {                                                                                const float va = BF ? moann_bf2f((uint16_t)((w) & 0xFFFF))                                       : moann_h2f((uint16_t)((w) & 0xFFFF));                   const float vb = BF ? moann_bf2f((uint16_t)((w) >> 16))                                          : moann_h2f((uint16_t)((w) >> 16));                      out0 = va;                                                                   out1 = vb;                                                               }

    for (int g0 = jv.gstart + 2 * wave; g0 < gend; g0 += 8) {
        const bool has1 = (g0 + 1) < gend;
        const int g1 = has1 ? g0 + 1 : g0;
        const uint4* __restrict__ d0 =
            (const uint4*)(packed + (jv.baseg + g0) * (int64_t)64 * dpad) + lane;
        const uint4* __restrict__ d1 =
            (const uint4*)(packed + (jv.baseg + g1) * (int64_t)64 * dpad) + lane;

        float acc0[QT], acc1[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) acc0[t] = acc1[t] = 0.f;
        float rn0 = 0.f, rn1 = 0.f;

#pragma unroll 2
        for (int j8 = 0; j8 < d8; ++j8) {
            const uint4 c0 = d0[j8 * 64];
            const uint4 c1 = d1[j8 * 64];
            float x0[8], x1[8];
            MOANN_H8(c0.x, x0[0], x0[1]) MOANN_H8(c0.y, x0[2], x0[3])
            MOANN_H8(c0.z, x0[4], x0[5]) MOANN_H8(c0.w, x0[6], x0[7])
            MOANN_H8(c1.x, x1[0], x1[1]) MOANN_H8(c1.y, x1[2], x1[3])
            MOANN_H8(c1.z, x1[4], x1[5]) MOANN_H8(c1.w, x1[6], x1[7])
            if (METRIC == KM_COS) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    rn0 = fmaf(x0[u], x0[u], rn0);
                    rn1 = fmaf(x1[u], x1[u], rn1);
                }
            }
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const uint4 qw =
                    *(const uint4*)(ldsq + t * dpad + j8 * 8);
                float qv[8];
                MOANN_H8(qw.x, qv[0], qv[1]) MOANN_H8(qw.y, qv[2], qv[3])
                MOANN_H8(qw.z, qv[4], qv[5]) MOANN_H8(qw.w, qv[6], qv[7])
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (METRIC == KM_L2SQ) {
                        const float e0 = x0[u] - qv[u];
                        acc0[t] = fmaf(e0, e0, acc0[t]);
                        const float e1 = x1[u] - qv[u];
                        acc1[t] = fmaf(e1, e1, acc1[t]);
                    } else if (METRIC == KM_IP || METRIC == KM_COS) {
                        acc0[t] = fmaf(x0[u], qv[u], acc0[t]);
                        acc1[t] = fmaf(x1[u], qv[u], acc1[t]);
                    } else {
                        acc0[t] += fabsf(x0[u] - qv[u]);
                        acc1[t] += fabsf(x1[u] - qv[u]);
                    }
                }
            }
        }
#undef MOANN_H8

        store_group_pair<QT, METRIC == KM_COS>(
            jobs, jv, lane, g0, g1, has1, acc0, acc1, rn0, rn1, ldsn,
            filter_bitset, dists_out, [](float acc, float rn, float qn) {
                return finish_f32<METRIC>(acc, rn, qn);
            });
    }
}

void launch_scan_h(int metric, ScanVariant v, bool bf,
                   const uint16_t* packed, const uint16_t* queries_h,
                   const float* qnorms, int dpad, const ScanJobs& jb,
                   float* dists_out, hipStream_t stream,
                   const uint32_t* filter_bitset) {
    if (v.kind != ScanKind::HALF || v.qt != 8) bad_variant("launch_scan_h", v);
    if (!jb.njobs) return;
    with_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const dim3 grid(jb.njobs), block(256);
        const size_t shmem = 8 * dpad * 2 + 8 * 4 + 16;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, packed,
                               queries_h, qnorms, dpad, jb, filter_bitset,
                               dists_out);
        };
        bf ? launch(scan_h_kernel<M, true>) : launch(scan_h_kernel<M, false>);
    });
}

/* ---------------- exact f32 refine (two-stage scan) ---------------------
 * Re-rank the byte-stage top-R candidates with exact f32 distances over a
 * row-major copy of the entries (SQ8-with-refine, the standard recall
 * recovery; the byte stage reads 1/4 the bytes of the f32 scan). One
 * workgroup per query: query row cached in LDS, one WAVE per candidate,
 * lane-parallel over dims, shfl reduce. Distance semantics identical to
 * the f32 scan kernel (MO conventions incl. cosine's double denom). */
template <int METRIC>
__global__ __launch_bounds__(256) void refine_kernel(
    const float* __restrict__ rows_f32, /* [count][dim] slot-major */
    const float* __restrict__ queries,  /* [nq][dpad] */
    const float* __restrict__ qnorms,   /* [nq] |q|^2 (cos) */
    int dim, int dpad, int R,
    const int32_t* __restrict__ rsel_slots, /* [nq][R] candidate positions */
    const float* __restrict__ rsel_dists,   /* [nq][R] byte dists (padding) */
    const int32_t* __restrict__ probe_lists,
    const int64_t* __restrict__ probe_offs,
    const int64_t* __restrict__ list_slot_base, int nprobe,
    float* __restrict__ refined /* [nq][R] */) {
    extern __shared__ float ldsq[]; /* [dpad] */
    const int q = blockIdx.x;
    const float* qv = queries + (int64_t)q * dpad;
    for (int e = threadIdx.x; e < dpad; e += blockDim.x) ldsq[e] = qv[e];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t* offs = probe_offs + (int64_t)q * (nprobe + 1);

    for (int c = wave; c < R; c += 4) {
        const int64_t idx = (int64_t)q * R + c;
        const int32_t pos = rsel_slots[idx];
        if (pos < 0 || rsel_dists[idx] == FLT_MAX) {
            if (lane == 0) refined[idx] = FLT_MAX;
            continue;
        }
        /* candidate position -> (probed list, local row) -> global slot */
        int lo = 0, hi = nprobe - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= pos) lo = mid; else hi = mid - 1;
        }
        const int32_t list = probe_lists[(int64_t)q * nprobe + lo];
        const int64_t slot = list_slot_base[list] + (pos - offs[lo]);
        const float* row = rows_f32 + slot * (int64_t)dim;
        float acc = 0.f, rn = 0.f;
        for (int t = lane; t < dim; t += 64) {
            const float x = row[t], qq = ldsq[t];
            if (METRIC == KM_L2SQ) {
                const float e = x - qq;
                acc = fmaf(e, e, acc);
            } else if (METRIC == KM_IP || METRIC == KM_COS) {
                acc = fmaf(x, qq, acc);
                if (METRIC == KM_COS) rn = fmaf(x, x, rn);
            } else {
                acc += fabsf(x - qq);
            }
        }
        for (int off = 32; off; off >>= 1) {
            acc += __shfl_down(acc, off, 64);
            if (METRIC == KM_COS) rn += __shfl_down(rn, off, 64);
        }
        if (lane == 0) { /* qnorms is null unless cos */
            float dist;
            if (METRIC == KM_IP) dist = -acc;
            else if (METRIC == KM_COS)
                dist = mo_cos_distance(acc, rn, qnorms[q]);
            else dist = acc;
            refined[idx] = dist;
        }
    }
}

void launch_refine(int metric, const float* rows_f32, const float* queries,
                   const float* qnorms, int dim, int dpad, int R, int nq,
                   const int32_t* rsel_slots, const float* rsel_dists,
                   const int32_t* probe_lists, const int64_t* probe_offs,
                   const int64_t* list_slot_base, int nprobe, float* refined,
                   hipStream_t stream) {
    if (!nq) return;
    const size_t shmem = (size_t)dpad * 4;
    with_metric(metric, [&](auto m) {
        hipLaunchKernelGGL(refine_kernel<decltype(m)::value>, dim3(nq),
                           dim3(256), shmem, stream, rows_f32, queries, qnorms,
                           dim, dpad, R, rsel_slots, rsel_dists, probe_lists,
                           probe_offs, list_slot_base, nprobe, refined);
    });
}

/* final-selection composition: sel2 indexes into the refine set; map back
 * to candidate positions so the shared gather kernel applies unchanged */
__global__ void compose_select_kernel(const int32_t* __restrict__ sel2,
                                      const int32_t* __restrict__ rsel_slots,
                                      int R, int k, int64_t total,
                                      int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int32_t s2 = sel2[i];
    const int64_t q = i / k;
    out[i] = s2 < 0 ? -1 : rsel_slots[q * R + s2];
}

void launch_compose_select(const int32_t* sel2, const int32_t* rsel_slots,
                           int R, int k, int nq, int32_t* out,
                           hipStream_t stream) {
    const int64_t total = (int64_t)nq * k;
    if (!total) return;
    hipLaunchKernelGGL(compose_select_kernel,
                       dim3((uint32_t)((total + 255) / 256)), dim3(256), 0,
                       stream, sel2, rsel_slots, R, k, total, out);
}

/* ---------------- fused refine tail (R <= REFINE_FINISH_RMAX) ------------
 * refine_kernel -> topk_kernel over [nq][R] -> compose_select_kernel ->
 * gather_kernel in one block per query:
 *  1. threads c < R resolve candidate position -> global slot, once, into
 *     LDS (-1: padding, or a byte distance of FLT_MAX);
 *  2. a wave takes candidates four at a time and loads from all four rows
 *     before it accumulates, so four rows are in flight per wave where
 *     refine_kernel has one behind a chain of dependent loads. Each
 *     candidate keeps refine_kernel's arithmetic: lane l sums dims l, l+64,
 *     ... in ascending order, the same shfl tree, the same finish — the
 *     exact distances are bit-identical;
 *  3. bitonic sort of (f2u(dist) << 32 | c) over next_pow2(R) keys: what
 *     topk_kernel returns for a row of R <= 1024 values;
 *  4. thread i < k writes id and transformed distance, gather_kernel's
 *     padding rule.
 * LDS: [dpad] f32 query, [P] u64 keys, [R] i64 slots. */
constexpr int REFINE_FINISH_RMAX = 1024;

template <int METRIC>
__global__ __launch_bounds__(256) void refine_finish_kernel(
    const float* __restrict__ rows_f32, const float* __restrict__ queries,
    const float* __restrict__ qnorms, int dim, int dpad, int R, int P,
    const int32_t* __restrict__ rsel_slots,
    const float* __restrict__ rsel_dists,
    const int32_t* __restrict__ probe_lists,
    const int64_t* __restrict__ probe_offs,
    const int64_t* __restrict__ list_slot_base,
    const int64_t* __restrict__ id_by_slot, int nprobe, int k, int do_sqrt,
    double inv_mul2, int64_t* __restrict__ out_ids,
    float* __restrict__ out_dists) {
    extern __shared__ unsigned char rf_smem[];
    uint64_t* keys = (uint64_t*)rf_smem;         /* [P]    */
    int64_t* slots = (int64_t*)(keys + P);       /* [R]    */
    float* ldsq = (float*)(slots + R);           /* [dpad] */
    const int q = blockIdx.x, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const float* qv = queries + (int64_t)q * dpad;
    for (int e = tid; e < dpad; e += blockDim.x) ldsq[e] = qv[e];

    /* 1. candidate position -> (probed list, local row) -> global slot */
    const int64_t* offs = probe_offs + (int64_t)q * (nprobe + 1);
    for (int c = tid; c < R; c += blockDim.x) {
        const int64_t idx = (int64_t)q * R + c;
        const int32_t pos = rsel_slots[idx];
        int64_t slot = -1;
        if (pos >= 0 && rsel_dists[idx] != FLT_MAX) {
            int lo = 0, hi = nprobe - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (offs[mid] <= pos) lo = mid; else hi = mid - 1;
            }
            const int32_t list = probe_lists[(int64_t)q * nprobe + lo];
            slot = list_slot_base[list] + (pos - offs[lo]);
        }
        slots[c] = slot;
    }
    for (int c = R + tid; c < P; c += blockDim.x) keys[c] = ~0ULL;
    __syncthreads();

    /* 2. exact distances, four candidates per wave step */
    for (int c0 = wave * 4; c0 < R; c0 += 16) {
        const float* row[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t slot = c0 + j < R ? slots[c0 + j] : -1;
            row[j] = slot < 0 ? nullptr : rows_f32 + slot * (int64_t)dim;
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, rn[4] = {0.f, 0.f, 0.f, 0.f};
        /* four 64-dim steps of four rows: 16 loads issued, then summed */
        for (int t0 = lane; t0 < dim; t0 += 256) {
            float x[4][4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    x[s][j] = (t0 + 64 * s < dim && row[j])
                                  ? row[j][t0 + 64 * s] : 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int t = t0 + 64 * s;
                if (t < dim) {
                    const float qq = ldsq[t];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xv = x[s][j];
                        if (METRIC == KM_L2SQ) {
                            const float e = xv - qq;
                            acc[j] = fmaf(e, e, acc[j]);
                        } else if (METRIC == KM_IP || METRIC == KM_COS) {
                            acc[j] = fmaf(xv, qq, acc[j]);
                            if (METRIC == KM_COS)
                                rn[j] = fmaf(xv, xv, rn[j]);
                        } else {
                            acc[j] += fabsf(xv - qq);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = acc[j], r = rn[j];
            for (int off = 32; off; off >>= 1) {
                a += __shfl_down(a, off, 64);
                if (METRIC == KM_COS) r += __shfl_down(r, off, 64);
            }
            if (lane == 0 && c0 + j < R) { /* qnorms is null unless cos */
                float dist = FLT_MAX;
                if (row[j]) {
                    if (METRIC == KM_IP) dist = -a;
                    else if (METRIC == KM_COS)
                        dist = mo_cos_distance(a, r, qnorms[q]);
                    else dist = a;
                }
                keys[c0 + j] = ((uint64_t)f2u(dist) << 32) | (uint32_t)(c0 + j);
            }
        }
    }
    __syncthreads();

    /* 3. sort, 4. write */
    for (int ks = 2; ks <= P; ks <<= 1) {
        for (int jj = ks >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P; i += blockDim.x) {
                const int l = i ^ jj;
                if (l > i) {
                    const uint64_t a = keys[i], b = keys[l];
                    const bool up = (i & ks) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += blockDim.x) {
        const int64_t o = (int64_t)q * k + i;
        int64_t slot = -1;
        float dist = FLT_MAX;
        if (i < R) {
            const uint64_t kv = keys[i];
            slot = slots[(uint32_t)kv];
            dist = u2f((uint32_t)(kv >> 32));
        }
        /* FLT_MAX marks padding AND membership-filtered rows */
        if (slot < 0 || dist == FLT_MAX) {
            out_ids[o] = -1; out_dists[o] = FLT_MAX;
        } else {
            out_ids[o] = id_by_slot[slot];
            out_dists[o] = transform_score_dev(dist, do_sqrt, inv_mul2);
        }
    }
}

static size_t refine_finish_lds(int R, int dpad) {
    int P = 1;
    while (P < R) P <<= 1;
    return (size_t)P * 8 + (size_t)R * 8 + (size_t)dpad * 4;
}

bool refine_finish_applies(int R, int dpad) {
    return R <= REFINE_FINISH_RMAX && refine_finish_lds(R, dpad) <= 64 * 1024;
}

void launch_refine_finish(int metric, const float* rows_f32,
                          const float* queries, const float* qnorms, int dim,
                          int dpad, int R, int nq, const int32_t* rsel_slots,
                          const float* rsel_dists, const int32_t* probe_lists,
                          const int64_t* probe_offs,
                          const int64_t* list_slot_base,
                          const int64_t* id_by_slot, int nprobe, int k,
                          int do_sqrt, double inv_mul2, int64_t* out_ids,
                          float* out_dists, hipStream_t stream) {
    if (!nq) return;
    if (!refine_finish_applies(R, dpad) || k > R)
        throw std::logic_error("launch_refine_finish: R " + std::to_string(R) +
                               " k " + std::to_string(k) + " dpad " +
                               std::to_string(dpad));
    int P = 1;
    while (P < R) P <<= 1;
    const size_t shmem = refine_finish_lds(R, dpad);
    with_metric(metric, [&](auto m) {
        hipLaunchKernelGGL(refine_finish_kernel<decltype(m)::value>, dim3(nq),
                           dim3(256), shmem, stream, rows_f32, queries, qnorms,
                           dim, dpad, R, P, rsel_slots, rsel_dists,
                           probe_lists, probe_offs, list_slot_base,
                           id_by_slot, nprobe, k, do_sqrt, inv_mul2, out_ids,
                           out_dists);
    });
}

/* -------------------------- quantized (int8/uint8) scan ------------------
 * Narrow-storage variant of the list scan (reference: int8/uint8 entries
 * quantized by q(x)=round(x*mul+add), distance computed IN THE QUANTIZED
 * DOMAIN with exact integer accumulation — distance_func_narrow.go:330-450;
 * the /mul^2 rescale happens at gather, ivfflat/search.go:1062-1077).
 * Data layout: bytes [g][dpad/4][64][4] (same interleave as f32, byte
 * elements — one coalesced 256 B read per wave step). Query tile: quantized
 * bytes in LDS. int32 accumulators are exact for dpad <= 33024 (l2sq term
 * <= 65025/elem). */
template <int METRIC, bool UNSIGNED>
__global__ __launch_bounds__(256) void scan_i8_kernel(
    const uint8_t* __restrict__ packed, const uint8_t* __restrict__ queries_q,
    const int32_t* __restrict__ qnorms_i /* [nq] sum sq, cos only */,
    int dpad, const ScanJobs jobs,
    const uint32_t* __restrict__ filter_bitset,
    float* __restrict__ dists_out) {
    constexpr int QT = 8;
    extern __shared__ float ldsf[];
    uint8_t* ldsq = (uint8_t*)ldsf;            /* [QT][dpad] bytes */
    int32_t* ldsn = (int32_t*)(ldsq + QT * dpad);

    const JobView jv = load_job(jobs);
    stage_query_tile<QT, METRIC == KM_COS>(jv, jobs.qslot_query, queries_q,
                                           qnorms_i, dpad, ldsq, ldsn);

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gend = jv.gstart + jv.gcount;
    const int d4 = dpad >> 2;

    const auto sx = [](uint8_t b) -> int {
        return UNSIGNED ? (int)b : (int)(int8_t)b;
    };

    for (int g0 = jv.gstart + 2 * wave; g0 < gend; g0 += 8) {
        const bool has1 = (g0 + 1) < gend;
        const int g1 = has1 ? g0 + 1 : g0;
        const uchar4* __restrict__ d0 =
            (const uchar4*)(packed + (jv.baseg + g0) * (int64_t)64 * dpad) + lane;
        const uchar4* __restrict__ d1 =
            (const uchar4*)(packed + (jv.baseg + g1) * (int64_t)64 * dpad) + lane;
        int32_t acc0[QT], acc1[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) acc0[t] = acc1[t] = 0;
        int32_t rn0 = 0, rn1 = 0;
#pragma unroll 2
        for (int q4 = 0; q4 < d4; ++q4) {
            const uchar4 x0 = d0[q4 * 64];
            const uchar4 x1 = d1[q4 * 64];
            if (METRIC == KM_COS) {
                rn0 += sx(x0.x) * sx(x0.x) + sx(x0.y) * sx(x0.y) +
                       sx(x0.z) * sx(x0.z) + sx(x0.w) * sx(x0.w);
                rn1 += sx(x1.x) * sx(x1.x) + sx(x1.y) * sx(x1.y) +
                       sx(x1.z) * sx(x1.z) + sx(x1.w) * sx(x1.w);
            }
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const uchar4 qv = ((const uchar4*)(ldsq + t * dpad))[q4];
                if (METRIC == KM_L2SQ) {
                    int e;
                    e = sx(x0.x) - sx(qv.x); acc0[t] += e * e;
                    e = sx(x0.y) - sx(qv.y); acc0[t] += e * e;
                    e = sx(x0.z) - sx(qv.z); acc0[t] += e * e;
                    e = sx(x0.w) - sx(qv.w); acc0[t] += e * e;
                    e = sx(x1.x) - sx(qv.x); acc1[t] += e * e;
                    e = sx(x1.y) - sx(qv.y); acc1[t] += e * e;
                    e = sx(x1.z) - sx(qv.z); acc1[t] += e * e;
                    e = sx(x1.w) - sx(qv.w); acc1[t] += e * e;
                } else if (METRIC == KM_IP || METRIC == KM_COS) {
                    acc0[t] += sx(x0.x) * sx(qv.x) + sx(x0.y) * sx(qv.y) +
                               sx(x0.z) * sx(qv.z) + sx(x0.w) * sx(qv.w);
                    acc1[t] += sx(x1.x) * sx(qv.x) + sx(x1.y) * sx(qv.y) +
                               sx(x1.z) * sx(qv.z) + sx(x1.w) * sx(qv.w);
                } else { /* KM_L1 */
                    acc0[t] += abs(sx(x0.x) - sx(qv.x)) +
                               abs(sx(x0.y) - sx(qv.y)) +
                               abs(sx(x0.z) - sx(qv.z)) +
                               abs(sx(x0.w) - sx(qv.w));
                    acc1[t] += abs(sx(x1.x) - sx(qv.x)) +
                               abs(sx(x1.y) - sx(qv.y)) +
                               abs(sx(x1.z) - sx(qv.z)) +
                               abs(sx(x1.w) - sx(qv.w));
                }
            }
        }
        store_group_pair<QT, METRIC == KM_COS>(
            jobs, jv, lane, g0, g1, has1, acc0, acc1, rn0, rn1, ldsn,
            filter_bitset, dists_out, [](int32_t acc, int32_t rn, int32_t qn) {
                return finish_i32<METRIC, false>(acc, rn, qn);
            });
    }
}

/* Dot-form byte scan (dpad % 16 == 0): one dwordx4 load = 16 dims of the
 * row per lane (1 KiB per wave step, same stream shape as the f32 kernel
 * — the uchar4 kernel's 256 B loads were MLP-starved at ~1 TB/s), and the
 * arithmetic uses the CDNA dot/sad byte ops:
 *   L2sq:  |x-q|^2 = rn + qn - 2*dot(x,q)  (exact in int32: bounds
 *          255^2*dpad <= 5.1e7 at dpad<=768; v_dot4_{i32_i8,u32_u8})
 *   IP/cos: dot(x,q) directly (cos norms precomputed, same ints)
 *   L1:    v_sad_u8 (signed values biased by XOR 0x80 per byte — two's
 *          complement int8 + 128 == x ^ 0x80, |x-q| unchanged)
 * Row norms rn come from launch_rownorms_i8 at build time; query norms qn
 * from launch_qnorms_i8. Results are bit-identical to scan_i8_kernel
 * (exact integer arithmetic both ways); that kernel stays the path for
 * dpad % 16 != 0. */
template <int METRIC, bool UNSIGNED, int QT = 8>
__global__ __launch_bounds__(256) void scan_i8_dot_kernel(
    const uint8_t* __restrict__ packed, const uint8_t* __restrict__ queries_q,
    const int32_t* __restrict__ qnorms_i, /* [nq] sum sq (l2/cos) */
    const int32_t* __restrict__ rownorms, /* [ngroups*64] sum sq (l2/cos) */
    int dpad, const ScanJobs jobs,
    const uint32_t* __restrict__ filter_bitset,
    float* __restrict__ dists_out) {
    constexpr bool NEED_N = METRIC == KM_L2SQ || METRIC == KM_COS;
    extern __shared__ float ldsf[];
    uint8_t* ldsq = (uint8_t*)ldsf;            /* [QT][dpad] bytes */
    int32_t* ldsn = (int32_t*)(ldsq + QT * dpad);

    const JobView jv = load_job(jobs);
    stage_query_tile<QT, NEED_N>(jv, jobs.qslot_query, queries_q, qnorms_i,
                                 dpad, ldsq, ldsn);

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gend = jv.gstart + jv.gcount;
    const int d16 = dpad >> 4;

    for (int g0 = jv.gstart + 2 * wave; g0 < gend; g0 += 8) {
        const bool has1 = (g0 + 1) < gend;
        const int g1 = has1 ? g0 + 1 : g0;
        const uint4* __restrict__ d0 =
            (const uint4*)(packed + (jv.baseg + g0) * (int64_t)64 * dpad) + lane;
        const uint4* __restrict__ d1 =
            (const uint4*)(packed + (jv.baseg + g1) * (int64_t)64 * dpad) + lane;

        int32_t acc0[QT], acc1[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) acc0[t] = acc1[t] = 0;

#pragma unroll 2
        for (int j16 = 0; j16 < d16; ++j16) {
            uint4 x0 = d0[j16 * 64];
            uint4 x1 = d1[j16 * 64];
            if (METRIC == KM_L1 && !UNSIGNED) {
                /* bias int8 -> u8 so v_sad_u8 applies */
                x0.x ^= 0x80808080u; x0.y ^= 0x80808080u;
                x0.z ^= 0x80808080u; x0.w ^= 0x80808080u;
                x1.x ^= 0x80808080u; x1.y ^= 0x80808080u;
                x1.z ^= 0x80808080u; x1.w ^= 0x80808080u;
            }
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                uint4 qv = *(const uint4*)(ldsq + t * dpad + j16 * 16);
                if (METRIC == KM_L1) {
                    if (!UNSIGNED) {
                        qv.x ^= 0x80808080u; qv.y ^= 0x80808080u;
                        qv.z ^= 0x80808080u; qv.w ^= 0x80808080u;
                    }
                    acc0[t] = (int32_t)__builtin_amdgcn_sad_u8(x0.x, qv.x, (uint32_t)acc0[t]);
                    acc0[t] = (int32_t)__builtin_amdgcn_sad_u8(x0.y, qv.y, (uint32_t)acc0[t]);
                    acc0[t] = (int32_t)__builtin_amdgcn_sad_u8(x0.z, qv.z, (uint32_t)acc0[t]);
                    acc0[t] = (int32_t)__builtin_amdgcn_sad_u8(x0.w, qv.w, (uint32_t)acc0[t]);
                    acc1[t] = (int32_t)__builtin_amdgcn_sad_u8(x1.x, qv.x, (uint32_t)acc1[t]);
                    acc1[t] = (int32_t)__builtin_amdgcn_sad_u8(x1.y, qv.y, (uint32_t)acc1[t]);
                    acc1[t] = (int32_t)__builtin_amdgcn_sad_u8(x1.z, qv.z, (uint32_t)acc1[t]);
                    acc1[t] = (int32_t)__builtin_amdgcn_sad_u8(x1.w, qv.w, (uint32_t)acc1[t]);
                } else if (UNSIGNED) {
                    acc0[t] = (int32_t)__builtin_amdgcn_udot4(x0.x, qv.x, (uint32_t)acc0[t], false);
                    acc0[t] = (int32_t)__builtin_amdgcn_udot4(x0.y, qv.y, (uint32_t)acc0[t], false);
                    acc0[t] = (int32_t)__builtin_amdgcn_udot4(x0.z, qv.z, (uint32_t)acc0[t], false);
                    acc0[t] = (int32_t)__builtin_amdgcn_udot4(x0.w, qv.w, (uint32_t)acc0[t], false);
                    acc1[t] = (int32_t)__builtin_amdgcn_udot4(x1.x, qv.x, (uint32_t)acc1[t], false);
                    acc1[t] = (int32_t)__builtin_amdgcn_udot4(x1.y, qv.y, (uint32_t)acc1[t], false);
                    acc1[t] = (int32_t)__builtin_amdgcn_udot4(x1.z, qv.z, (uint32_t)acc1[t], false);
                    acc1[t] = (int32_t)__builtin_amdgcn_udot4(x1.w, qv.w, (uint32_t)acc1[t], false);
                } else {
                    acc0[t] = __builtin_amdgcn_sdot4((int32_t)x0.x, (int32_t)qv.x, acc0[t], false);
                    acc0[t] = __builtin_amdgcn_sdot4((int32_t)x0.y, (int32_t)qv.y, acc0[t], false);
                    acc0[t] = __builtin_amdgcn_sdot4((int32_t)x0.z, (int32_t)qv.z, acc0[t], false);
                    acc0[t] = __builtin_amdgcn_sdot4((int32_t)x0.w, (int32_t)qv.w, acc0[t], false);
                    acc1[t] = __builtin_amdgcn_sdot4((int32_t)x1.x, (int32_t)qv.x, acc1[t], false);
                    acc1[t] = __builtin_amdgcn_sdot4((int32_t)x1.y, (int32_t)qv.y, acc1[t], false);
                    acc1[t] = __builtin_amdgcn_sdot4((int32_t)x1.z, (int32_t)qv.z, acc1[t], false);
                    acc1[t] = __builtin_amdgcn_sdot4((int32_t)x1.w, (int32_t)qv.w, acc1[t], false);
                }
            }
        }

        const int32_t rn0 = NEED_N ? rownorms[(jv.baseg + g0) * 64 + lane] : 0;
        const int32_t rn1 = NEED_N ? rownorms[(jv.baseg + g1) * 64 + lane] : 0;
        store_group_pair<QT, NEED_N>(
            jobs, jv, lane, g0, g1, has1, acc0, acc1, rn0, rn1, ldsn,
            filter_bitset, dists_out, [](int32_t acc, int32_t rn, int32_t qn) {
                return finish_i32<METRIC, true>(acc, rn, qn);
            });
    }
}

/* MFMA byte scan (dpad % 64 == 0, signed bytes, QT = 16): the dot-form scan
 * as the 16-column int8 GEMM it is, on v_mfma_i32_16x16x64_i8. Reads the
 * image in ByteImageLayout::MFMA64 — per group of 64 rows and 64-dim step J,
 * four 1 KiB units (16-row sub-blocks s); in a unit lane l's 16 bytes are row
 * 16s + (l & 15), dims 64J + 16(l >> 4) .. +15 — so one coalesced wave load
 * is one B operand as it stands. The A operand is the query tile: lane l
 * reads query (l & 15), the same 16 dims, from LDS (row stride dpad + 16:
 * the sixteen rows of one read fall on distinct banks). Both operands hold
 * the same k positions in the same lane, so the product is the row-by-query
 * dot whatever the k order inside the instruction. Accumulator: column
 * (lane & 15) = image row, row 4(lane >> 4) + reg = query; one store
 * instruction writes 4 queries x 16 consecutive rows.
 *
 * A wave streams a CONTIGUOUS run of the job's groups (a quarter of the
 * chunk) as one sequence of 4 KiB steps through a register ring RING steps
 * deep: the steady-state loop reloads each ring slot unconditionally right
 * after consuming it, so RING * 4 KiB stay in flight across steps and group
 * boundaries; the last steps are peeled. Exact int32 accumulation: results
 * are bit-identical to scan_i8_dot_kernel. */
typedef int mfma_v4i __attribute__((ext_vector_type(4)));

/* One 4 KiB step of the MFMA scan's stream into a ring slot: four 1 KiB wave
 * loads. Written as asm so that hipcc does not track them: with plain loads
 * it drained the whole ring (s_waitcnt vmcnt(0)) before every step, because
 * the group epilogue inside the loop leaves its wait state unknown. The
 * slot's registers hold nothing until ring_wait has passed over them. */
__device__ __forceinline__ void ring_load(mfma_v4i (&x)[4], const uint4* p) {
    asm volatile(
        "global_load_dwordx4 %0, %4, off\n\t"
        "global_load_dwordx4 %1, %4, off offset:1024\n\t"
        "global_load_dwordx4 %2, %4, off offset:2048\n\t"
        "global_load_dwordx4 %3, %4, off offset:3072"
        : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3])
        : "v"(p));
}

/* Wait until at most NEWER vector-memory operations issued after this slot's
 * ring_load are outstanding (they complete in issue order, so the slot has
 * landed; anything else issued since only makes the wait stricter). The slot
 * is an in-out operand so that no use of it moves above the wait. */
template <int NEWER>
__device__ __forceinline__ void ring_wait(mfma_v4i (&x)[4]) {
    asm volatile("s_waitcnt vmcnt(%4)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3])
                 : "n"(NEWER));
}

template <int METRIC>
__global__ __launch_bounds__(256) void scan_i8_mfma_kernel(
    const uint8_t* __restrict__ packed, const uint8_t* __restrict__ queries_q,
    const int32_t* __restrict__ qnorms_i, /* [nq] sum sq (l2/cos) */
    const int32_t* __restrict__ rownorms, /* [ngroups*64] sum sq (l2/cos) */
    int dpad, const ScanJobs jobs,
    const uint32_t* __restrict__ filter_bitset,
    float* __restrict__ dists_out) {
    constexpr int QT = 16, RING = 3;
    constexpr bool NEED_N = METRIC == KM_L2SQ || METRIC == KM_COS;
    extern __shared__ float ldsf[];
    uint8_t* ldsq = (uint8_t*)ldsf; /* [QT][dpad + 16] bytes */
    const int qstride = dpad + 16;
    int32_t* ldsn = (int32_t*)(ldsq + QT * qstride);

    const JobView jv = load_job(jobs);

    /* query tile -> LDS, 16 bytes per thread and step; slots t >= nq zero */
    {
        const int d16 = dpad >> 4;
        for (int e = threadIdx.x; e < QT * d16; e += 256) {
            const int t = e / d16, c = e - t * d16;
            uint4 v = {0, 0, 0, 0};
            if (t < jv.nq) {
                const int q = jobs.qslot_query[jv.qbase + t];
                v = ((const uint4*)(queries_q + (int64_t)q * dpad))[c];
            }
            *(uint4*)(ldsq + t * qstride + 16 * c) = v;
        }
        if (NEED_N && threadIdx.x < QT)
            ldsn[threadIdx.x] =
                (int)threadIdx.x < jv.nq
                    ? qnorms_i[jobs.qslot_query[jv.qbase + threadIdx.x]]
                    : 0;
        __syncthreads();
    }

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r16 = lane & 15, quad = lane >> 4;
    const int nJ = dpad >> 6;

    /* this wave's contiguous groups of the chunk */
    const int per = (jv.gcount + 3) >> 2;
    const int gw0 = jv.gstart + wave * per;
    const int ngw = min(per, jv.gstart + jv.gcount - gw0);
    if (ngw <= 0) return;
    const int nsteps = ngw * nJ;

    /* the 4 queries this lane finishes: output bases and norms */
    int64_t ob[4];
    int32_t qn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = 4 * quad + i;
        ob[i] = t < jv.nq ? jobs.qslot_outbase[jv.qbase + t] : 0;
        qn[i] = NEED_N ? ldsn[t] : 0;
    }
    const int64_t sb = filter_bitset ? jobs.slot_base[jv.j] : 0;

    /* step k of the wave: 4 uint4 per lane at base + k*256 + s*64 */
    const uint4* __restrict__ base =
        (const uint4*)(packed + (jv.baseg + gw0) * (int64_t)64 * dpad) + lane;
    const uint8_t* qlane = ldsq + r16 * qstride + 16 * quad;

    mfma_v4i acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = mfma_v4i{0, 0, 0, 0};
    int J = 0, g = gw0;

    const auto consume = [&](const mfma_v4i (&x)[4]) {
        const uint4 qv = *(const uint4*)(qlane + 64 * J);
        const mfma_v4i a = {(int)qv.x, (int)qv.y, (int)qv.z, (int)qv.w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, x[s], acc[s], 0,
                                                           0, 0);
        }
        if (++J < nJ) return;
        /* group done. First everything the epilogue reads from memory, and
         * an explicit wait for it: a load the compiler still counts as
         * pending when control rejoins the stream (a row whose queries are
         * all skipped never uses its norm) made it drain the ring before
         * every ring_load. Stores may stay in flight. */
        int32_t rn[4];
        bool live[4], pass[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = g * 64 + 16 * s + r16;
            live[s] = row < jv.rows;
            rn[s] = NEED_N && live[s]
                        ? rownorms[(jv.baseg + g) * 64 + 16 * s + r16]
                        : 0;
            pass[s] = !filter_bitset || !live[s] ||
                      slot_passes(filter_bitset, sb + row);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0) only */
        /* finish and store, filter per row */
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = g * 64 + 16 * s + r16;
            if (live[s]) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * quad + i < jv.nq)
                        dists_out[ob[i] + row] =
                            pass[s] ? finish_i32<METRIC, true>(acc[s][i],
                                                               rn[s], qn[i])
                                    : FLT_MAX;
            }
            acc[s] = mfma_v4i{0, 0, 0, 0};
        }
        J = 0;
        ++g;
    };

    mfma_v4i ring[RING][4];
#pragma unroll
    for (int d = 0; d < RING; ++d) {
#pragma unroll
        for (int s = 0; s < 4; ++s) ring[d][s] = mfma_v4i{0, 0, 0, 0};
        if (d < nsteps) ring_load(ring[d], base + d * 256);
    }

    /* steady state: a slot is consumed once only the RING - 1 younger slots'
     * loads may still be out, then reloaded RING steps ahead */
    const int nmain = nsteps > RING ? (nsteps - RING) / RING * RING : 0;
    int k = 0;
    for (; k < nmain; k += RING) {
#pragma unroll
        for (int d = 0; d < RING; ++d) {
            ring_wait<4 * (RING - 1)>(ring[d]);
            consume(ring[d]);
            ring_load(ring[d], base + (int64_t)(k + d + RING) * 256);
        }
    }
    /* peeled tail, at most 2*RING - 1 steps: drain the ring once, then
     * rotate it; the first RING - 1 of these steps still load */
#pragma unroll
    for (int d = 0; d < RING; ++d) ring_wait<0>(ring[d]);
    for (; k < nsteps; ++k) {
        consume(ring[0]);
#pragma unroll
        for (int d = 0; d + 1 < RING; ++d)
#pragma unroll
            for (int s = 0; s < 4; ++s) ring[d][s] = ring[d + 1][s];
        if (k + RING < nsteps) {
            const uint4* nx = base + (int64_t)(k + RING) * 256;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint4 v = nx[s * 64];
                ring[RING - 1][s] =
                    mfma_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
            }
        }
    }
}

/* pack quantized byte rows into 16-byte units: [g][dpad/16][64][16] — the
 * layout the dot-form scan streams with 16 B/lane dwordx4 loads (the
 * uchar4 [g][dpad/4][64][4] layout only gives 4 B/lane per 256 B block).
 * Used when dpad % 16 == 0; thread per output uint4. */
__global__ void bytes_pack16_kernel(const uint8_t* __restrict__ rows_q,
                                    int dpad,
                                    const int64_t* __restrict__ group_rowbase,
                                    const int32_t* __restrict__ group_valid,
                                    const int64_t* __restrict__ slot_rows,
                                    int64_t ngroups,
                                    uint8_t* __restrict__ packed) {
    const int d16 = dpad >> 4;
    const int64_t nunits = ngroups * (int64_t)d16 * 64;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < nunits; idx += stride) {
        const int lane = (int)(idx & 63);
        const int64_t rest = idx >> 6;
        const int m16 = (int)(rest % d16);
        const int64_t g = rest / d16;
        uint4 v = {0, 0, 0, 0};
        if (lane < group_valid[g]) {
            const int64_t row = slot_rows[group_rowbase[g] + lane];
            v = *(const uint4*)(rows_q + row * (int64_t)dpad + 16 * m16);
        }
        ((uint4*)packed)[idx] = v;
    }
}

void launch_bytes_pack16(const uint8_t* rows_q, int dpad,
                         const int64_t* group_rowbase,
                         const int32_t* group_valid,
                         const int64_t* slot_rows, int64_t ngroups,
                         uint8_t* packed, hipStream_t stream) {
    const int64_t nunits = ngroups * (int64_t)(dpad >> 4) * 64;
    if (!nunits) return;
    const int block = 256;
    const int64_t grid = std::min<int64_t>((nunits + block - 1) / block,
                                           1 << 22);
    hipLaunchKernelGGL(bytes_pack16_kernel, dim3((uint32_t)grid), dim3(block),
                       0, stream, rows_q, dpad, group_rowbase, group_valid,
                       slot_rows, ngroups, packed);
}

/* pack quantized byte rows in MFMA order (ByteImageLayout::MFMA64, dpad % 64
 * == 0): [g][dpad/64][4][64][16] — unit (g, J, s), lane l holds row
 * 16s + (l & 15), dims 64J + 16(l >> 4) .. +15; what scan_i8_mfma_kernel
 * loads as its B operand. Same group stride (64*dpad bytes) as pack16;
 * thread per output uint4. */
__global__ void bytes_pack_mfma_kernel(const uint8_t* __restrict__ rows_q,
                                       int dpad,
                                       const int64_t* __restrict__ group_rowbase,
                                       const int32_t* __restrict__ group_valid,
                                       const int64_t* __restrict__ slot_rows,
                                       int64_t ngroups,
                                       uint8_t* __restrict__ packed) {
    const int nJ = dpad >> 6;
    const int64_t nunits = ngroups * (int64_t)nJ * 256;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < nunits; idx += stride) {
        const int lane = (int)(idx & 63);
        const int s = (int)((idx >> 6) & 3);
        const int64_t rest = idx >> 8;
        const int J = (int)(rest % nJ);
        const int64_t g = rest / nJ;
        const int rg = 16 * s + (lane & 15);
        uint4 v = {0, 0, 0, 0};
        if (rg < group_valid[g]) {
            const int64_t row = slot_rows[group_rowbase[g] + rg];
            v = *(const uint4*)(rows_q + row * (int64_t)dpad + 64 * J +
                                16 * (lane >> 4));
        }
        ((uint4*)packed)[idx] = v;
    }
}

void launch_bytes_pack_mfma(const uint8_t* rows_q, int dpad,
                            const int64_t* group_rowbase,
                            const int32_t* group_valid,
                            const int64_t* slot_rows, int64_t ngroups,
                            uint8_t* packed, hipStream_t stream) {
    const int64_t nunits = ngroups * (int64_t)(dpad >> 6) * 256;
    if (!nunits) return;
    const int block = 256;
    const int64_t grid = std::min<int64_t>((nunits + block - 1) / block,
                                           1 << 22);
    hipLaunchKernelGGL(bytes_pack_mfma_kernel, dim3((uint32_t)grid),
                       dim3(block), 0, stream, rows_q, dpad, group_rowbase,
                       group_valid, slot_rows, ngroups, packed);
}

/* per-(group,lane) byte-row sum of squares; lane = row of the group in both
 * layouts, so the output is [g*64 + row] either way */
template <bool UNSIGNED, bool MFMA64>
__global__ __launch_bounds__(256) void rownorms_i8_kernel(
    const uint8_t* __restrict__ packed, int64_t ngroups, int dpad,
    int32_t* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + wave;
    if (g >= ngroups) return;
    /* ROWS16: [g][dpad/16][64][16] (bytes_pack16_kernel): 16-dim unit m of
     * row `lane` is uint4 m*64 + lane. MFMA64 (bytes_pack_mfma_kernel): it
     * is uint4 ((m>>2)*4 + (lane>>4))*64 + (m&3)*16 + (lane&15). */
    const uint4* __restrict__ d =
        (const uint4*)(packed + g * (int64_t)64 * dpad) +
        (MFMA64 ? (lane >> 4) * 64 + (lane & 15) : lane);
    int32_t acc = 0;
    const int d16 = dpad >> 4;
    for (int m = 0; m < d16; ++m) {
        const uint4 v = MFMA64 ? d[(m >> 2) * 256 + (m & 3) * 16] : d[m * 64];
        if (UNSIGNED) {
            acc = (int32_t)__builtin_amdgcn_udot4(v.x, v.x, (uint32_t)acc, false);
            acc = (int32_t)__builtin_amdgcn_udot4(v.y, v.y, (uint32_t)acc, false);
            acc = (int32_t)__builtin_amdgcn_udot4(v.z, v.z, (uint32_t)acc, false);
            acc = (int32_t)__builtin_amdgcn_udot4(v.w, v.w, (uint32_t)acc, false);
        } else {
            acc = __builtin_amdgcn_sdot4((int32_t)v.x, (int32_t)v.x, acc, false);
            acc = __builtin_amdgcn_sdot4((int32_t)v.y, (int32_t)v.y, acc, false);
            acc = __builtin_amdgcn_sdot4((int32_t)v.z, (int32_t)v.z, acc, false);
            acc = __builtin_amdgcn_sdot4((int32_t)v.w, (int32_t)v.w, acc, false);
        }
    }
    out[g * 64 + lane] = acc;
}

void launch_rownorms_i8(bool uns, ByteImageLayout layout,
                        const uint8_t* packed, int64_t ngroups, int dpad,
                        int32_t* out, hipStream_t stream) {
    const dim3 grid((uint32_t)((ngroups + 3) / 4)), block(256);
    if (layout == ByteImageLayout::MFMA64) {
        if (uns || dpad % 64)
            throw std::logic_error("launch_rownorms_i8: MFMA64 image is "
                                   "signed with dpad % 64 == 0");
        hipLaunchKernelGGL((rownorms_i8_kernel<false, true>), grid, block, 0,
                           stream, packed, ngroups, dpad, out);
    } else if (uns)
        hipLaunchKernelGGL((rownorms_i8_kernel<true, false>), grid, block, 0,
                           stream, packed, ngroups, dpad, out);
    else
        hipLaunchKernelGGL((rownorms_i8_kernel<false, false>), grid, block, 0,
                           stream, packed, ngroups, dpad, out);
}

void launch_scan_i8(int metric, ScanVariant v, bool uns,
                    ByteImageLayout layout, const uint8_t* packed,
                    const uint8_t* queries_q, const int32_t* qnorms,
                    const int32_t* rownorms, int dpad, const ScanJobs& jb,
                    float* dists_out, hipStream_t stream,
                    const uint32_t* filter_bitset) {
    /* the byte kernels' only tile widths: dot form 16 and 8, uchar4 form 8 */
    const bool dot_ok = v.kind == ScanKind::BYTE_DOT &&
                        (v.qt == 16 || v.qt == 8);
    const bool u4_ok = v.kind == ScanKind::BYTE_U4 && v.qt == 8;
    if (!dot_ok && !u4_ok) bad_variant("launch_scan_i8", v);
    if (dot_ok && !rownorms)
        throw std::logic_error("launch_scan_i8: BYTE_DOT without row norms");
    if (layout == ByteImageLayout::MFMA64) {
        /* the image was packed for scan_i8_mfma_kernel alone: a variant or
         * metric that kernel does not cover must never read it */
        if (!byte_mfma_applies(metric, v, dpad) || uns)
            throw std::logic_error("launch_scan_i8: MFMA64 image with a "
                                   "variant the MFMA scan does not cover");
        if (!jb.njobs) return;
        with_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if constexpr (M != KM_L1) {
                const size_t shmem = (size_t)16 * (dpad + 16) + 16 * 4;
                hipLaunchKernelGGL(scan_i8_mfma_kernel<M>, dim3(jb.njobs),
                                   dim3(256), shmem, stream, packed,
                                   queries_q, qnorms, rownorms, dpad, jb,
                                   filter_bitset, dists_out);
            }
        });
        return;
    }
    if (!jb.njobs) return;
    with_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const dim3 grid(jb.njobs), block(256);
        const int qt = v.qt;
        const size_t shmem = (size_t)qt * dpad + (size_t)qt * 4 + 16;
        /* dot form (16-dim-aligned rows + row norms) or the uchar4 kernel */
        const auto dot = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, packed,
                               queries_q, qnorms, rownorms, dpad, jb,
                               filter_bitset, dists_out);
        };
        const auto u4 = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, packed,
                               queries_q, qnorms, dpad, jb, filter_bitset,
                               dists_out);
        };
        if (dot_ok && qt == 16)
            uns ? dot(scan_i8_dot_kernel<M, true, 16>)
                : dot(scan_i8_dot_kernel<M, false, 16>);
        else if (dot_ok)
            uns ? dot(scan_i8_dot_kernel<M, true, 8>)
                : dot(scan_i8_dot_kernel<M, false, 8>);
        else
            uns ? u4(scan_i8_kernel<M, true>) : u4(scan_i8_kernel<M, false>);
    });
}

/* quantize f32 rows -> int8/uint8 with the reference's exact semantics:
 * two separate f32 roundings (product, then sum — quantizer.go:165-176),
 * round half away from zero, clamp, NaN -> 0 (float16.go:227-239).
 * Pad columns (dim <= c < dpad) emit 0 so padded dims stay identity for
 * every metric (q(0) is generally nonzero — quantizing pads would poison
 * IP/cosine). in: [rows][in_stride] f32; out: [rows][dpad] bytes. */
template <bool UNSIGNED>
__global__ void quantize_rows_kernel(const float* __restrict__ in,
                                     int64_t nrows, int in_stride, int dim,
                                     int dpad, float fmul, float fadd,
                                     uint8_t* __restrict__ out) {
    /* GRID-STRIDE: the AQL packet's grid size counts WORK-ITEMS in 32
     * bits, so a flat launch of >= 2^32 threads silently wraps (measured:
     * exactly total mod 2^32 elements written at 6M x 768 halves). Every
     * elementwise kernel over rows x dpad strides instead. */
    const int64_t total = nrows * (int64_t)dpad;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < total; i += stride) {
        const int64_t r = i / dpad;
        const int c = (int)(i % dpad);
        if (c >= dim) {
            out[i] = 0;
            continue;
        }
        const float x = in[r * (int64_t)in_stride + c];
        float m = x * fmul;
        asm volatile("" : "+v"(m)); /* block FMA fusion of the two f32 ops */
        const float sum = m + fadd;
        float v;
        if (sum != sum) v = 0.f;
        else v = (float)round((double)sum);
        const float lo = UNSIGNED ? 0.f : -128.f;
        const float hi = UNSIGNED ? 255.f : 127.f;
        v = v < lo ? lo : (v > hi ? hi : v);
        out[i] = UNSIGNED ? (uint8_t)v : (uint8_t)(int8_t)v;
    }
}

void launch_quantize_rows(bool uns, const float* in, int64_t nrows,
                          int in_stride, int dim, int dpad, float fmul,
                          float fadd, uint8_t* out, hipStream_t stream) {
    const int64_t total = nrows * (int64_t)dpad;
    if (!total) return;
    const int block = 256;
    /* cap work-items below 2^31: the AQL grid is 32-bit in WORK-ITEMS */
    const int64_t grid = std::min<int64_t>((total + block - 1) / block,
                                           1 << 22);
    if (uns)
        hipLaunchKernelGGL((quantize_rows_kernel<true>), dim3((uint32_t)grid),
                           dim3(block), 0, stream, in, nrows, in_stride, dim,
                           dpad, fmul, fadd, out);
    else
        hipLaunchKernelGGL((quantize_rows_kernel<false>), dim3((uint32_t)grid),
                           dim3(block), 0, stream, in, nrows, in_stride, dim,
                           dpad, fmul, fadd, out);
}

/* int32 sum-of-squares per quantized query (cos, narrow path) */
template <bool UNSIGNED>
__global__ void qnorm_i8_kernel(const uint8_t* __restrict__ q, int nq,
                                int dpad, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint8_t* row = q + (int64_t)i * dpad;
    int32_t s = 0;
    for (int e = 0; e < dpad; ++e) {
        const int v = UNSIGNED ? (int)row[e] : (int)(int8_t)row[e];
        s += v * v;
    }
    out[i] = s;
}

void launch_qnorms_i8(bool uns, const uint8_t* q, int nq, int dpad,
                      int32_t* out, hipStream_t stream) {
    if (!nq) return;
    const int grid = (nq + 255) / 256;
    if (uns)
        hipLaunchKernelGGL((qnorm_i8_kernel<true>), dim3(grid), dim3(256), 0,
                           stream, q, nq, dpad, out);
    else
        hipLaunchKernelGGL((qnorm_i8_kernel<false>), dim3(grid), dim3(256), 0,
                           stream, q, nq, dpad, out);
}

/* --------------------------- pairwise 1xN --------------------------------
 * The SQL distance-builtin batch (metric.PairwiseDistanceLaunch,
 * pkg/sql/plan/function/func_binary.go:9127 const-query 1xN) and the legacy
 * cgo/cuda/mocl.cu l2distance kernels, subsumed: one wave per row over
 * row-major data, MO distance conventions. */
template <int METRIC>
__global__ __launch_bounds__(256) void pairwise_kernel(
    const float* __restrict__ rows, const float* __restrict__ query,
    float qnorm /* |q|^2, cos only */, int64_t n, int dim,
    float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) +
                      (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const float* row = rows + r * (int64_t)dim;
    float acc = 0.f, nrm = 0.f;
    for (int e = lane; e < dim; e += 64) {
        const float x = row[e], qv = query[e];
        if (METRIC == KM_L2SQ) {
            const float d = x - qv;
            acc = fmaf(d, d, acc);
        } else if (METRIC == KM_L1) {
            acc += fabsf(x - qv);
        } else {
            acc = fmaf(x, qv, acc);
            if (METRIC == KM_COS) nrm += x * x;
        }
    }
#pragma unroll
    for (int w = 32; w; w >>= 1) {
        acc += __shfl_down(acc, w, 64);
        if (METRIC == KM_COS) nrm += __shfl_down(nrm, w, 64);
    }
    if (lane) return;
    out[r] = finish_f32<METRIC>(acc, nrm, qnorm);
}

void launch_pairwise(int metric, const float* rows, const float* query,
                     float qnorm, int64_t n, int dim, float* out,
                     hipStream_t stream) {
    if (!n) return;
    const int wpb = 4;
    const int64_t grid = (n + wpb - 1) / wpb;
    with_metric(metric, [&](auto m) {
        hipLaunchKernelGGL((pairwise_kernel<decltype(m)::value>),
                           dim3((uint32_t)grid), dim3(wpb * 64), 0, stream,
                           rows, query, qnorm, n, dim, out);
    });
}

/* --------------------------- query norms ---------------------------------
 * one wave per query; f32 accumulate (matches distance_func.go cosine's f32
 * norm accumulation within the 1e-5 parity tolerance). */
__global__ void qnorm_kernel(const float* __restrict__ queries, int nq,
                             int dpad, float* __restrict__ qnorms) {
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const float* src = queries + (int64_t)q * dpad;
    float s = 0.f;
    for (int e = lane; e < dpad; e += 64) s += src[e] * src[e];
#pragma unroll
    for (int w = 32; w; w >>= 1) s += __shfl_down(s, w, 64);
    if (lane == 0) qnorms[q] = s;
}

void launch_qnorms(const float* queries, int nq, int dpad, float* qnorms,
                   hipStream_t stream) {
    if (!nq) return;
    const int wpb = 4;
    const int grid = (nq + wpb - 1) / wpb;
    hipLaunchKernelGGL(qnorm_kernel, dim3(grid), dim3(wpb * 64), 0, stream,
                       queries, nq, dpad, qnorms);
}

}  // namespace moann
