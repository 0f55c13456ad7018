/* Resident brute-force index on gfx950: the fused exact
 * distance + top-k kernel, and the small kernels around the two search modes
 * (moann_bf_lib.cpp, moann_bf_plan.h).
 *
 * bf_fused_topk_kernel is assign_argmin_kernel (kmeans_kernels.hip) with the
 * running argmin generalised to a sorted list of k entries per query. The
 * GEMM part is that kernel's, operand roles swapped: one 256-thread block
 * owns 128 queries (A) and walks the 128-row tiles (B) of its row slice; wave
 * w owns queries [32w, 32w+32) against all 128 rows of a tile (2 x 8 MFMA
 * tiles of `v_mfma_f32_16x16x4_f32`, 16 accumulators). K is walked in 32-dim
 * slabs through one LDS stage with a 36-float pitch, the next slab's global
 * loads held in registers while the MFMAs consume the current one. Both
 * operands are [.][dpad] with dpad % 4 == 0 and zero padding, so every
 * stage-in is an aligned 16-byte load and a slab past dpad is zeros.
 * Fragments: lane l reads 4 consecutive floats at k = 16s + 4(l>>4) of row
 * l&15 and feeds element e to MFMA e of the chunk — a permutation of k applied
 * to both operands alike. C/D: lane l, reg r -> query (l>>4)*4 + r, row l&15.
 *
 * Epilogue. The distances are rank_gemm_kernel's (qn + xn - 2 dot clamped at
 * 0, -dot, mo_cos_distance) from the norms the host computed with
 * launch_qnorms. Each query's list lives in LDS, [k] distances and [k] rows
 * sorted ascending by (distance, row) and padded with (FLT_MAX, -1); only the
 * wave that owns the query touches it, so no barrier guards it. Its k-th
 * distance is mirrored in a register of the 16 lanes that hold the query's
 * columns. A value enters only by strict < against that k-th distance; a dead,
 * excluded or out-of-range row carries FLT_MAX and never does. Survivors are
 * inserted one at a time by the whole wave, in ascending row order per query
 * (j ascends, then the lane): lane e holds entry e, the insert position is
 * the count of entries <= the new distance (the new row is larger than every
 * row already listed, so it goes behind its equals), entry e-1 arrives by a
 * lane shift, and lane e writes entry e. Every lane reads and writes its own
 * address only, reads before writes, so the update needs no ordering beyond
 * program order. No atomic is involved: the lists are a pure function of the
 * inputs. Once the lists are warm almost no tile has a survivor, and one
 * ballot skips the insert code altogether.
 *
 * KCAP (16, 32 or 64) is the list capacity the launch picks for k: the LDS
 * lists take 128 * KCAP * 8 bytes beside the 36.5 KB of the stage, so
 * KCAP <= 32 keeps two blocks per CU (69 KB each of 160 KB) and KCAP = 64
 * (101 KB) runs one. */

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <stdexcept>

#include "moann_bf_plan.h"
#include "moann_internal.h"
#include "moann_scan_device.h" /* mo_cos_distance, scan_job_index */

namespace moann {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int BF_KS = 32;    /* K slab (dims per LDS stage)       */
constexpr int BF_PITCH = 36; /* LDS row pitch, floats (see above) */
constexpr int BQ = (int)BF_QTILE, BR = (int)BF_TILE;

template <int METRIC, int KCAP>
__global__ __launch_bounds__(256, KCAP <= 32 ? 2 : 1) void bf_fused_topk_kernel(
    const float* __restrict__ rows,    /* [n][dpad], zero-padded            */
    const float* __restrict__ xnorms,  /* [n] |x|^2                         */
    const uint32_t* __restrict__ mask, /* bit per row, cleared = excluded;
                                          null = every row passes           */
    int64_t n,
    const float* __restrict__ queries, /* [nq][dpad], zero-padded           */
    const float* __restrict__ qnorms,  /* [nq] |q|^2 (null for KM_IP)       */
    int nq, int dpad, int k, int nqb /* query blocks */,
    int64_t tiles, int64_t tiles_per_slice, int64_t nslices,
    float* __restrict__ cand_d,   /* [nq][nslices][k] */
    int32_t* __restrict__ cand_r /* [nq][nslices][k] */) {
    __shared__ __attribute__((aligned(16))) float ldsq[BQ * BF_PITCH];
    __shared__ __attribute__((aligned(16))) float ldsx[BR * BF_PITCH];
    __shared__ float ldsn[BQ];        /* |q|^2 of the block's queries */
    __shared__ float lstd[BQ * KCAP]; /* per-query list: distances    */
    __shared__ int32_t lstr[BQ * KCAP]; /*               and rows     */

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    /* consecutive jobs share a row slice: the XCD remap lets the query
     * blocks of one slice stream it through one L2 */
    const int job = scan_job_index();
    const int64_t slice = job / nqb;
    const int qbase = (job % nqb) * BQ;
    const int64_t t0 = slice * tiles_per_slice;
    const int64_t t1 = t0 + tiles_per_slice < tiles ? t0 + tiles_per_slice
                                                    : tiles;

    /* stage-in indexing: thread t moves quad (t&7) of rows (t>>3) + 32i */
    const int srow = tid >> 3, squad = (tid & 7) * 4;
    const float* qp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int q = qbase + srow + 32 * i;
        q = q < nq ? q : nq - 1; /* clamped queries are computed, not stored */
        qp[i] = queries + (int64_t)q * dpad;
    }
    if (METRIC != KM_IP && tid < BQ) {
        const int q = qbase + tid;
        ldsn[tid] = qnorms[q < nq ? q : nq - 1];
    }
    /* the wave's 32 lists start as padding */
    for (int e = lane; e < 32 * KCAP; e += 64) {
        lstd[wave * 32 * KCAP + e] = FLT_MAX;
        lstr[wave * 32 * KCAP + e] = -1;
    }

    const int nks = (dpad + BF_KS - 1) / BF_KS;

    float4 pq[4], px[4];
    auto gload = [&](int64_t tile, int ks) {
        const int kk = ks * BF_KS + squad;
        const bool in = kk < dpad; /* dpad % 4 == 0: the whole quad is */
#pragma unroll
        for (int i = 0; i < 4; ++i)
            pq[i] = in ? *(const float4*)(qp[i] + kk)
                       : float4 {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int64_t r = tile * BR + srow + 32 * i;
            r = r < n ? r : n - 1; /* clamped rows never enter (epilogue) */
            px[i] = in ? *(const float4*)(rows + r * dpad + kk)
                       : float4 {0.f, 0.f, 0.f, 0.f};
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(float4*)&ldsq[(srow + 32 * i) * BF_PITCH + squad] = pq[i];
            *(float4*)&ldsx[(srow + 32 * i) * BF_PITCH + squad] = px[i];
        }
    };

    const int frow = lane & 15, fq = (lane >> 4) * 4;
    const float* qa = &ldsq[(wave * 32 + frow) * BF_PITCH + fq];
    const float* xb = &ldsx[frow * BF_PITCH + fq];

    f32x4 acc[2][8];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[t][j] = f32x4 {0.f, 0.f, 0.f, 0.f};
    float kth[2][4]; /* k-th distance of query wave*32 + t*16 + fq + r */
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) kth[t][r] = FLT_MAX;

    gload(t0, 0);
    lstore();
    __syncthreads();
    for (int64_t tile = t0; tile < t1; ++tile) {
        for (int ks = 0; ks < nks; ++ks) {
            const bool last_ks = ks + 1 == nks;
            const bool more = !last_ks || tile + 1 < t1;
            if (more) gload(last_ks ? tile + 1 : tile, last_ks ? 0 : ks + 1);
#pragma unroll
            for (int s = 0; s < BF_KS / 16; ++s) {
                const float4 a0 = *(const float4*)(qa + 16 * s);
                const float4 a1 =
                    *(const float4*)(qa + 16 * BF_PITCH + 16 * s);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float4 b =
                        *(const float4*)(xb + j * 16 * BF_PITCH + 16 * s);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a0.x, b.x, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a1.x, b.x, acc[1][j], 0, 0, 0);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a0.y, b.y, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a1.y, b.y, acc[1][j], 0, 0, 0);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a0.z, b.z, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a1.z, b.z, acc[1][j], 0, 0, 0);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a0.w, b.w, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a1.w, b.w, acc[1][j], 0, 0, 0);
                }
            }
            if (last_ks) {
                /* dots -> distances in place; FLT_MAX for a row that may not
                 * enter. `any`: some value beats its query's k-th distance */
                bool any = false;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int64_t row = tile * BR + j * 16 + frow;
                    bool live = row < n;
                    if (live && mask)
                        live = (mask[row >> 5] >> (row & 31)) & 1u;
                    const float xn =
                        (METRIC != KM_IP && row < n) ? xnorms[row] : 0.f;
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float dot = acc[t][j][r];
                            float dist;
                            if (METRIC == KM_IP) {
                                dist = -dot;
                            } else {
                                const float qn =
                                    ldsn[wave * 32 + t * 16 + fq + r];
                                if (METRIC == KM_COS) {
                                    dist = mo_cos_distance(dot, xn, qn);
                                } else {
                                    dist = qn + xn - 2.0f * dot;
                                    if (dist < 0.f) dist = 0.f;
                                }
                            }
                            if (!live) dist = FLT_MAX;
                            acc[t][j][r] = dist;
                            any |= dist < kth[t][r];
                        }
                }
                if (__ballot(any)) { /* wave-uniform */
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                float d = acc[t][j][r];
                                const int32_t rowi =
                                    (int32_t)(tile * BR + j * 16 + frow);
                                unsigned long long m;
                                /* re-tested against the k-th distance each
                                 * round: an insert may have lowered it */
                                while ((m = __ballot(d < kth[t][r])) != 0) {
                                    const int L = __ffsll(m) - 1;
                                    const float cd = __shfl(d, L);
                                    const int32_t cr = __shfl(rowi, L);
                                    const int ql = wave * 32 + t * 16 +
                                                   (L >> 4) * 4 + r;
                                    float* ld = &lstd[ql * KCAP];
                                    int32_t* lr = &lstr[ql * KCAP];
                                    const bool mine = lane < k;
                                    const float ed = mine ? ld[lane] : FLT_MAX;
                                    const int32_t er = mine ? lr[lane] : -1;
                                    const int pos =
                                        __popcll(__ballot(mine && ed <= cd));
                                    const float pd = __shfl_up(ed, 1);
                                    const int32_t pr = __shfl_up(er, 1);
                                    const float nd = lane < pos ? ed
                                                     : lane == pos ? cd : pd;
                                    const int32_t nr = lane < pos ? er
                                                       : lane == pos ? cr : pr;
                                    if (mine && lane >= pos) {
                                        ld[lane] = nd;
                                        lr[lane] = nr;
                                    }
                                    const float nk = __shfl(nd, k - 1);
                                    if ((lane >> 4) == (L >> 4)) kth[t][r] = nk;
                                    if (lane == L) d = FLT_MAX; /* consumed */
                                }
                            }
                }
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        acc[t][j] = f32x4 {0.f, 0.f, 0.f, 0.f};
            }
            __syncthreads(); /* every wave is done reading this stage */
            if (more) lstore();
            __syncthreads();
        }
    }

    /* the wave's lists -> this slice's segment of the candidate buffer */
    for (int ql = 0; ql < 32; ++ql) {
        const int q = qbase + wave * 32 + ql;
        if (q < nq && lane < k) {
            const int64_t o = ((int64_t)q * nslices + slice) * k + lane;
            cand_d[o] = lstd[(wave * 32 + ql) * KCAP + lane];
            cand_r[o] = lstr[(wave * 32 + ql) * KCAP + lane];
        }
    }
}

/* gemm mode: excluded rows of a [nq][len] distance tile -> FLT_MAX */
__global__ __launch_bounds__(256) void bf_mask_kernel(
    float* __restrict__ dmat, int nq, int64_t len, int64_t row0,
    const uint32_t* __restrict__ mask) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nq * len) return;
    const int64_t row = row0 + idx % len;
    if (!((mask[row >> 5] >> (row & 31)) & 1u)) dmat[idx] = FLT_MAX;
}

/* gemm mode: one chunk's launch_topk output -> its candidate segment as
 * (distance, row) pairs. A slot launch_topk padded, or one whose key is not
 * below FLT_MAX (an excluded row), becomes the padding (FLT_MAX, -1). */
__global__ __launch_bounds__(256) void bf_stash_kernel(
    const int32_t* __restrict__ sel_slots, const float* __restrict__ sel_dists,
    int nq, int k, int64_t row0, int64_t slice, int64_t nslices,
    float* __restrict__ cand_d, int32_t* __restrict__ cand_r) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nq * k) return;
    const int64_t q = idx / k, e = idx % k;
    const int32_t slot = sel_slots[idx];
    const float d = sel_dists[idx];
    const bool real = slot >= 0 && d < FLT_MAX;
    const int64_t o = (q * nslices + slice) * k + e;
    cand_d[o] = real ? d : FLT_MAX;
    cand_r[o] = real ? (int32_t)(row0 + slot) : -1;
}

/* Final selection's slots -> ids and distances: slot -> candidate row -> id.
 * Padding (-1, FLT_MAX) for a padded slot, a candidate without a row, or a
 * key that is not below FLT_MAX. L2sqrt takes its square root here, in f64
 * as transform_score_dev does. */
__global__ __launch_bounds__(256) void bf_gather_kernel(
    const int32_t* __restrict__ sel_slots, const float* __restrict__ sel_dists,
    const int32_t* __restrict__ cand_r, int64_t cand_per_q,
    const int64_t* __restrict__ ids, int nq, int k, int do_sqrt,
    int64_t* __restrict__ out_ids, float* __restrict__ out_dists) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nq * k) return;
    const int64_t q = idx / k;
    const int32_t slot = sel_slots[idx];
    const float d = sel_dists[idx];
    const int32_t row = slot >= 0 ? cand_r[q * cand_per_q + slot] : -1;
    if (row < 0 || !(d < FLT_MAX)) {
        out_ids[idx] = -1;
        out_dists[idx] = FLT_MAX;
        return;
    }
    out_ids[idx] = ids[row];
    out_dists[idx] = do_sqrt ? (float)sqrt((double)d) : d;
}

template <int METRIC, int KCAP>
void launch_fused(const float* rows, const float* xnorms,
                  const uint32_t* mask, int64_t n, const float* queries,
                  const float* qnorms, int nq, int dpad, int k,
                  const BfPlan& p, float* cand_d, int32_t* cand_r,
                  hipStream_t stream) {
    const int nqb = (nq + BQ - 1) / BQ;
    const dim3 grid((unsigned)(p.slices * nqb)), block(256);
    hipLaunchKernelGGL((bf_fused_topk_kernel<METRIC, KCAP>), grid, block, 0,
                       stream, rows, xnorms, mask, n, queries, qnorms, nq,
                       dpad, k, nqb, p.tiles, p.tiles_per_slice, p.slices,
                       cand_d, cand_r);
}

template <int METRIC>
void launch_fused_k(const float* rows, const float* xnorms,
                    const uint32_t* mask, int64_t n, const float* queries,
                    const float* qnorms, int nq, int dpad, int k,
                    const BfPlan& p, float* cand_d, int32_t* cand_r,
                    hipStream_t stream) {
    if (k <= 16)
        launch_fused<METRIC, 16>(rows, xnorms, mask, n, queries, qnorms, nq,
                                 dpad, k, p, cand_d, cand_r, stream);
    else if (k <= 32)
        launch_fused<METRIC, 32>(rows, xnorms, mask, n, queries, qnorms, nq,
                                 dpad, k, p, cand_d, cand_r, stream);
    else
        launch_fused<METRIC, 64>(rows, xnorms, mask, n, queries, qnorms, nq,
                                 dpad, k, p, cand_d, cand_r, stream);
}

}  // namespace

void launch_bf_fused_topk(int metric, const float* rows, const float* xnorms,
                          const uint32_t* mask, int64_t n,
                          const float* queries, const float* qnorms, int nq,
                          int dpad, int k, const BfPlan& plan, float* cand_d,
                          int32_t* cand_r, hipStream_t stream) {
    if (nq <= 0 || n <= 0) return;
    if (k < 1 || k > (int)BF_FUSED_KMAX)
        throw std::logic_error("launch_bf_fused_topk: k beyond the fused limit");
    switch (metric) {
    case KM_L2SQ:
        launch_fused_k<KM_L2SQ>(rows, xnorms, mask, n, queries, qnorms, nq,
                                dpad, k, plan, cand_d, cand_r, stream);
        break;
    case KM_IP:
        launch_fused_k<KM_IP>(rows, xnorms, mask, n, queries, qnorms, nq, dpad,
                              k, plan, cand_d, cand_r, stream);
        break;
    case KM_COS:
        launch_fused_k<KM_COS>(rows, xnorms, mask, n, queries, qnorms, nq,
                               dpad, k, plan, cand_d, cand_r, stream);
        break;
    default:
        throw std::logic_error("launch_bf_fused_topk: metric has no MFMA form");
    }
}

void launch_bf_mask(float* dmat, int nq, int64_t len, int64_t row0,
                    const uint32_t* mask, hipStream_t stream) {
    const int64_t total = (int64_t)nq * len;
    if (!total || !mask) return;
    hipLaunchKernelGGL(bf_mask_kernel, dim3((unsigned)((total + 255) / 256)),
                       dim3(256), 0, stream, dmat, nq, len, row0, mask);
}

void launch_bf_stash(const int32_t* sel_slots, const float* sel_dists, int nq,
                     int k, int64_t row0, int64_t slice, int64_t nslices,
                     float* cand_d, int32_t* cand_r, hipStream_t stream) {
    const int64_t total = (int64_t)nq * k;
    if (!total) return;
    hipLaunchKernelGGL(bf_stash_kernel, dim3((unsigned)((total + 255) / 256)),
                       dim3(256), 0, stream, sel_slots, sel_dists, nq, k, row0,
                       slice, nslices, cand_d, cand_r);
}

void launch_bf_gather(const int32_t* sel_slots, const float* sel_dists,
                      const int32_t* cand_r, int64_t cand_per_q,
                      const int64_t* ids, int nq, int k, int do_sqrt,
                      int64_t* out_ids, float* out_dists, hipStream_t stream) {
    const int64_t total = (int64_t)nq * k;
    if (!total) return;
    hipLaunchKernelGGL(bf_gather_kernel, dim3((unsigned)((total + 255) / 256)),
                       dim3(256), 0, stream, sel_slots, sel_dists, cand_r,
                       cand_per_q, ids, nq, k, do_sqrt, out_ids, out_dists);
}

}  // namespace moann
