/* Resident brute-force index, f16 row store (DESIGN.md §3d "f16 store"): the
 * fused exact distance + top-k kernel on `v_mfma_f32_16x16x32_f16`, and the
 * f16 -> f32 widening the gemm mode runs over a slice before the rank GEMM.
 *
 * bf_fused_topk_h_kernel is bf_fused_topk_kernel (bf_kernels.hip) with the
 * GEMM moved to the f16 MFMA: same 256 threads, one block per 128 queries
 * walking the 128-row tiles of its slice, wave w owning queries [32w, 32w+32)
 * against the whole tile (2 x 8 accumulator tiles), same job map, same
 * epilogue, lists and candidate-buffer format. Both operands are binary16
 * [.][dpad] with dpad % 8 == 0 and zero padding, so every stage-in is an
 * aligned 16-byte load of one 8-half unit and a unit or slab past dpad is
 * zeros. f16 products are exact in f32 and the accumulation is f32.
 *
 * K is walked in slabs of 64 halfs (8 units, 128 bytes per row: the stage
 * geometry of the f32 kernel's 32 floats) and a slab in two K=32 steps, 32
 * MFMAs per wave and slab. Fragments: in step s lane l reads unit 4s + (l>>4)
 * of row l&15 with one ds_read_b128 and supplies A[row l&15][k = 8(l>>4)+j]
 * resp. B[k = 8(l>>4)+j][col l&15], j = 0..7. C/D: lane l, reg r -> query
 * 4(l>>4) + r, row l&15, as in the f32 kernel.
 *
 * LDS image: rows of 128 bytes without padding, unit u of row r stored at
 * 16-byte slot u ^ ((r>>1) & 7) of its row. ds_read_b128 is served in four
 * 16-lane groups, each holding 8 lanes of one k-group and 8 of the next:
 * rows {0-3, 12-15} at unit u and rows {4-11} at unit u^1. A padded pitch
 * cannot separate them: with a pitch of p slots two such lanes meet when
 * (a-b) p = 1 mod 16, and a-b takes every non-zero residue (the 72-half pitch
 * is 2-way on 7 of a group's 16 lanes). With the XOR, the first set lands on
 * slots {u, u^1, u^6, u^7} and the second on {u^2, u^3, u^4, u^5} of the two
 * 128-byte halves of the bank row (r&1): 16 distinct slots, conflict-free.
 * The stores are ds_write_b128, served in groups of 8 contiguous lanes = the
 * 8 units of one row = one whole 128-byte half, in any permutation.
 *
 * KCAP as in the f32 kernel; the stage takes 32.5 KB, so KCAP <= 32 (65 KB)
 * keeps two blocks per CU and KCAP = 64 (97 KB) runs one. */

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cfloat>
#include <cstdint>
#include <stdexcept>

#include "moann_bf_plan.h"
#include "moann_internal.h"
#include "moann_scan_device.h" /* mo_cos_distance, scan_job_index */

namespace moann {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

constexpr int BFH_KS = 64;     /* K slab (halfs per LDS stage)  */
constexpr int BFH_ROWB = 128;  /* LDS bytes per row of a slab   */
constexpr int BQ = (int)BF_QTILE, BR = (int)BF_TILE;

template <int METRIC, int KCAP>
__global__ __launch_bounds__(256, KCAP <= 32 ? 2 : 1) void
bf_fused_topk_h_kernel(
    const uint16_t* __restrict__ rows, /* [n][dpad] binary16, zero-padded   */
    const float* __restrict__ xnorms,  /* [n] |x|^2                         */
    const uint32_t* __restrict__ mask, /* bit per row, cleared = excluded;
                                          null = every row passes           */
    int64_t n,
    const uint16_t* __restrict__ queries, /* [nq][dpad] binary16            */
    const float* __restrict__ qnorms,  /* [nq] |q|^2 (null for KM_IP)       */
    int nq, int dpad, int k, int nqb /* query blocks */,
    int64_t tiles, int64_t tiles_per_slice, int64_t nslices,
    float* __restrict__ cand_d,   /* [nq][nslices][k] */
    int32_t* __restrict__ cand_r /* [nq][nslices][k] */) {
    __shared__ __attribute__((aligned(16))) unsigned char ldsq[BQ * BFH_ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char ldsx[BR * BFH_ROWB];
    __shared__ float ldsn[BQ];        /* |q|^2 of the block's queries */
    __shared__ float lstd[BQ * KCAP]; /* per-query list: distances    */
    __shared__ int32_t lstr[BQ * KCAP]; /*               and rows     */

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int job = scan_job_index();
    const int64_t slice = job / nqb;
    const int qbase = (job % nqb) * BQ;
    const int64_t t0 = slice * tiles_per_slice;
    const int64_t t1 = t0 + tiles_per_slice < tiles ? t0 + tiles_per_slice
                                                    : tiles;

    /* stage-in indexing: thread t moves unit (t&7) of rows (t>>3) + 32i; the
     * swizzle term of those rows is that of (t>>3) */
    const int srow = tid >> 3, sunit = tid & 7;
    const int sslot = (sunit ^ ((srow >> 1) & 7)) * 16;
    const uint16_t* qp[4];
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

    const int nks = (dpad + BFH_KS - 1) / BFH_KS;

    uint4 pq[4], px[4];
    auto gload = [&](int64_t tile, int ks) {
        const int kk = ks * BFH_KS + sunit * 8;
        const bool in = kk < dpad; /* dpad % 8 == 0: the whole unit is */
#pragma unroll
        for (int i = 0; i < 4; ++i)
            pq[i] = in ? *(const uint4*)(qp[i] + kk) : uint4 {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int64_t r = tile * BR + srow + 32 * i;
            r = r < n ? r : n - 1; /* clamped rows never enter (epilogue) */
            px[i] = in ? *(const uint4*)(rows + r * dpad + kk)
                       : uint4 {0u, 0u, 0u, 0u};
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(uint4*)&ldsq[(srow + 32 * i) * BFH_ROWB + sslot] = pq[i];
            *(uint4*)&ldsx[(srow + 32 * i) * BFH_ROWB + sslot] = px[i];
        }
    };

    const int frow = lane & 15, fq = (lane >> 4) * 4;
    /* byte offset of the lane's unit in its row, for the two K=32 steps */
    const int fsw = (frow >> 1) & 7;
    const int foff[2] = {(((lane >> 4)) ^ fsw) * 16,
                         ((4 + (lane >> 4)) ^ fsw) * 16};
    const unsigned char* qa = &ldsq[(wave * 32 + frow) * BFH_ROWB];
    const unsigned char* xb = &ldsx[frow * BFH_ROWB];

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
            for (int s = 0; s < 2; ++s) {
                const f16x8 a0 = *(const f16x8*)(qa + foff[s]);
                const f16x8 a1 =
                    *(const f16x8*)(qa + 16 * BFH_ROWB + foff[s]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f16x8 b =
                        *(const f16x8*)(xb + j * 16 * BFH_ROWB + foff[s]);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        a0, b, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        a1, b, acc[1][j], 0, 0, 0);
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

/* gemm mode: binary16 [nrows][dpad_h] -> f32 [nrows][dpad_w], exact;
 * dpad_w <= dpad_h, the columns past dim are zeros in both */
__global__ __launch_bounds__(256) void bf_widen_half_kernel(
    const uint16_t* __restrict__ in, int64_t nrows, int dpad_h, int dpad_w,
    float* __restrict__ out) {
    const int64_t total = nrows * (int64_t)dpad_w;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int64_t r = idx / dpad_w;
        const int c = (int)(idx % dpad_w);
        __half_raw h;
        h.x = in[r * dpad_h + c];
        out[idx] = __half2float((__half)h);
    }
}

template <int METRIC, int KCAP>
void launch_fused_h(const uint16_t* rows, const float* xnorms,
                    const uint32_t* mask, int64_t n, const uint16_t* queries,
                    const float* qnorms, int nq, int dpad, int k,
                    const BfPlan& p, float* cand_d, int32_t* cand_r,
                    hipStream_t stream) {
    const int nqb = (nq + BQ - 1) / BQ;
    const dim3 grid((unsigned)(p.slices * nqb)), block(256);
    hipLaunchKernelGGL((bf_fused_topk_h_kernel<METRIC, KCAP>), grid, block, 0,
                       stream, rows, xnorms, mask, n, queries, qnorms, nq,
                       dpad, k, nqb, p.tiles, p.tiles_per_slice, p.slices,
                       cand_d, cand_r);
}

template <int METRIC>
void launch_fused_h_k(const uint16_t* rows, const float* xnorms,
                      const uint32_t* mask, int64_t n,
                      const uint16_t* queries, const float* qnorms, int nq,
                      int dpad, int k, const BfPlan& p, float* cand_d,
                      int32_t* cand_r, hipStream_t stream) {
    if (k <= 16)
        launch_fused_h<METRIC, 16>(rows, xnorms, mask, n, queries, qnorms, nq,
                                   dpad, k, p, cand_d, cand_r, stream);
    else if (k <= 32)
        launch_fused_h<METRIC, 32>(rows, xnorms, mask, n, queries, qnorms, nq,
                                   dpad, k, p, cand_d, cand_r, stream);
    else
        launch_fused_h<METRIC, 64>(rows, xnorms, mask, n, queries, qnorms, nq,
                                   dpad, k, p, cand_d, cand_r, stream);
}

}  // namespace

void launch_bf_fused_topk_h(int metric, const uint16_t* rows,
                            const float* xnorms, const uint32_t* mask,
                            int64_t n, const uint16_t* queries,
                            const float* qnorms, int nq, int dpad, int k,
                            const BfPlan& plan, float* cand_d, int32_t* cand_r,
                            hipStream_t stream) {
    if (nq <= 0 || n <= 0) return;
    if (k < 1 || k > (int)BF_FUSED_KMAX)
        throw std::logic_error(
            "launch_bf_fused_topk_h: k beyond the fused limit");
    if (dpad % 8 != 0)
        throw std::logic_error(
            "launch_bf_fused_topk_h: dpad must be a multiple of 8 halfs");
    switch (metric) {
    case KM_L2SQ:
        launch_fused_h_k<KM_L2SQ>(rows, xnorms, mask, n, queries, qnorms, nq,
                                  dpad, k, plan, cand_d, cand_r, stream);
        break;
    case KM_IP:
        launch_fused_h_k<KM_IP>(rows, xnorms, mask, n, queries, qnorms, nq,
                                dpad, k, plan, cand_d, cand_r, stream);
        break;
    case KM_COS:
        launch_fused_h_k<KM_COS>(rows, xnorms, mask, n, queries, qnorms, nq,
                                 dpad, k, plan, cand_d, cand_r, stream);
        break;
    default:
        throw std::logic_error(
            "launch_bf_fused_topk_h: metric has no MFMA form");
    }
}

void launch_bf_widen_half(const uint16_t* in, int64_t nrows, int dpad_h,
                          int dpad_w, float* out, hipStream_t stream) {
    const int64_t total = nrows * (int64_t)dpad_w;
    if (!total) return;
    const int64_t grid = (total + 255) / 256 < ((int64_t)1 << 22)
                             ? (total + 255) / 256
                             : (int64_t)1 << 22;
    hipLaunchKernelGGL(bf_widen_half_kernel, dim3((unsigned)grid), dim3(256),
                       0, stream, in, nrows, dpad_h, dpad_w, out);
}

}  // namespace moann
