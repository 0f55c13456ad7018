/* Native k-means build on gfx950: the fused assignment (distance GEMM +
 * running argmin, no [n][k] matrix), the deterministic centroid update and
 * the small helpers of the training loop (DESIGN.md "Native k-means build").
 *
 * assign_argmin_kernel computes the distances of rank_gemm_kernel
 * (mfma_rank.hip) — expanded L2 clamped at 0, -x.c, mo_cos_distance — with
 * `v_mfma_f32_16x16x4_f32`, exact f32 fmaf-chain numerics. One 256-thread
 * block owns 128 rows and walks every 128-centroid tile; wave w owns rows
 * [32w, 32w+32) of the block against all 128 centroids of the tile (2 x 8
 * MFMA tiles, 16 accumulators), so a row never spans two waves and its
 * running (min, argmin) stays in the registers of the 16 lanes that hold its
 * C/D columns until the single cross-lane reduction at the end.
 *
 * K is walked in 32-dim slabs through one LDS stage, the next slab's global
 * loads held in registers while the MFMAs consume the current one. LDS rows
 * have a 36-float pitch: a multiple of 4, so the 16-byte stage-in stores and
 * the 16-byte fragment reads are aligned, and 36r mod 64 puts the 16 rows of
 * a fragment read on 16 distinct 16-byte slots.
 * Fragments: lane l reads 4 consecutive floats at k = 16s + 4(l>>4) of row
 * l&15 and feeds element e to MFMA e of the chunk, so MFMA e sums
 * k = 16s + 4q + e over q = 0..3 — a permutation of k applied to both
 * operands alike. C/D: lane l, reg r -> row (l>>4)*4 + r, col l&15. */

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "moann_internal.h"
#include "moann_scan_device.h" /* mo_cos_distance */

namespace moann {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int KA_ROWS = 128;  /* rows per block                    */
constexpr int KA_CENTS = 128; /* centroids per tile                */
constexpr int KA_KS = 32;     /* K slab (dims per LDS stage)       */
constexpr int KA_PITCH = 36;  /* LDS row pitch, floats (see above) */

/* i*num stays inside int64: the host checks n * n_train < 2^63 before it
 * builds a map (kmeans_train) */
__device__ __forceinline__ int64_t km_src_row(const KmRowMap& m, int64_t i) {
    return m.num == m.den ? i : (i * m.num) / m.den;
}

/* 4 dims of a staged row at kk, zero past dim. Rows have stride `dim`, so
 * they are 16-byte aligned only when vec (stride % 4 == 0). */
__device__ __forceinline__ float4 km_load_row4(const float* __restrict__ rp,
                                               int kk, int dim, bool vec) {
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && kk + 3 < dim) {
        v = *(const float4*)(rp + kk);
    } else {
        if (kk < dim) v.x = rp[kk];
        if (kk + 1 < dim) v.y = rp[kk + 1];
        if (kk + 2 < dim) v.z = rp[kk + 2];
        if (kk + 3 < dim) v.w = rp[kk + 3];
    }
    return v;
}

template <int METRIC>
__global__ __launch_bounds__(256, 2) void assign_argmin_kernel(
    const float* __restrict__ rows, /* [.][row_stride] staged f32 rows     */
    int64_t row_stride, KmRowMap map, int64_t n,
    const float* __restrict__ cents,  /* [k][dpad], zero-padded            */
    const float* __restrict__ cnorms, /* [k] |c|^2                         */
    int k, int dim, int dpad,
    int32_t* __restrict__ assign, float* __restrict__ best /* [n] each */) {
    __shared__ __attribute__((aligned(16))) float ldsx[KA_ROWS * KA_PITCH];
    __shared__ __attribute__((aligned(16))) float ldsc[KA_CENTS * KA_PITCH];
    __shared__ float ldsn[KA_ROWS]; /* |x|^2 of the block's rows */

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t rbase = (int64_t)blockIdx.x * KA_ROWS;
    const bool vec = (row_stride & 3) == 0;

    /* stage-in indexing: thread t moves quad (t&7) of rows (t>>3) + 32i */
    const int srow = tid >> 3, squad = (tid & 7) * 4;
    const float* rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int64_t r = rbase + srow + 32 * i;
        if (r >= n) r = n - 1; /* clamped rows are computed, never stored */
        rp[i] = rows + km_src_row(map, r) * row_stride;
    }

    if (METRIC != KM_IP) {
        /* |x|^2: 8 threads per row, fixed order, fixed shuffle tree */
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = 0.f;
            for (int kk = squad; kk < dim; kk += 32) {
                const float4 v = km_load_row4(rp[i], kk, dim, vec);
                s = fmaf(v.x, v.x, s);
                s = fmaf(v.y, v.y, s);
                s = fmaf(v.z, v.z, s);
                s = fmaf(v.w, v.w, s);
            }
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            if ((tid & 7) == 0) ldsn[srow + 32 * i] = s;
        }
    }

    const int nks = (dpad + KA_KS - 1) / KA_KS;
    const int nct = (k + KA_CENTS - 1) / KA_CENTS;

    float4 px[4], pc[4];
    auto gload = [&](int ct, int ks) {
        const int kk = ks * KA_KS + squad;
#pragma unroll
        for (int i = 0; i < 4; ++i) px[i] = km_load_row4(rp[i], kk, dim, vec);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int c = ct * KA_CENTS + srow + 32 * i;
            c = c < k ? c : k - 1; /* clamped tiles never win (epilogue) */
            pc[i] = kk < dpad ? *(const float4*)(cents + (int64_t)c * dpad + kk)
                              : float4 {0.f, 0.f, 0.f, 0.f};
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(float4*)&ldsx[(srow + 32 * i) * KA_PITCH + squad] = px[i];
            *(float4*)&ldsc[(srow + 32 * i) * KA_PITCH + squad] = pc[i];
        }
    };

    const int frow = lane & 15, fq = (lane >> 4) * 4;
    const float* xa = &ldsx[(wave * 32 + frow) * KA_PITCH + fq];
    const float* cb = &ldsc[frow * KA_PITCH + fq];

    f32x4 acc[2][8];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[t][j] = f32x4 {0.f, 0.f, 0.f, 0.f};
    float bmin[2][4];
    int bidx[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bmin[t][r] = INFINITY;
            bidx[t][r] = 0;
        }

    gload(0, 0);
    lstore();
    __syncthreads();
    for (int ct = 0; ct < nct; ++ct) {
        for (int ks = 0; ks < nks; ++ks) {
            const bool last_ks = ks + 1 == nks;
            const bool more = !last_ks || ct + 1 < nct;
            if (more) gload(last_ks ? ct + 1 : ct, last_ks ? 0 : ks + 1);
#pragma unroll
            for (int s = 0; s < KA_KS / 16; ++s) {
                const float4 a0 = *(const float4*)(xa + 16 * s);
                const float4 a1 =
                    *(const float4*)(xa + 16 * KA_PITCH + 16 * s);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float4 b =
                        *(const float4*)(cb + j * 16 * KA_PITCH + 16 * s);
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
                /* tile epilogue, registers only: columns ascend with j and
                 * with ct, so the strict < keeps the lowest index per lane */
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int col = ct * KA_CENTS + j * 16 + frow;
                    const bool live = col < k;
                    const float cn =
                        (METRIC != KM_IP && live) ? cnorms[col] : 0.f;
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float dot = acc[t][j][r];
                            float dist;
                            if (METRIC == KM_IP) {
                                dist = -dot;
                            } else {
                                const float xn =
                                    ldsn[wave * 32 + t * 16 + fq + r];
                                if (METRIC == KM_COS) {
                                    dist = mo_cos_distance(dot, cn, xn);
                                } else {
                                    dist = xn + cn - 2.0f * dot;
                                    if (dist < 0.f) dist = 0.f;
                                }
                            }
                            if (live && dist < bmin[t][r]) {
                                bmin[t][r] = dist;
                                bidx[t][r] = col;
                            }
                            acc[t][j][r] = 0.f;
                        }
                }
            }
            __syncthreads(); /* every wave is done reading this stage */
            if (more) lstore();
            __syncthreads();
        }
    }

    /* the 16 lanes that share (l>>4) hold one row's columns: lexicographic
     * (distance, index) min across them, so equal distances resolve to the
     * lowest centroid index */
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float d = bmin[t][r];
            int ix = bidx[t][r];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                const float od = __shfl_xor(d, m);
                const int oi = __shfl_xor(ix, m);
                if (od < d || (od == d && oi < ix)) {
                    d = od;
                    ix = oi;
                }
            }
            const int64_t row = rbase + wave * 32 + t * 16 + fq + r;
            if (frow == 0 && row < n) {
                assign[row] = ix;
                best[row] = d;
            }
        }
}

/* Per-row sum of squares (INV: 1/|x|, 0 for a zero row), f64 accumulation in
 * a fixed order: 8 threads per row, fixed shuffle tree. */
template <bool INV>
__global__ __launch_bounds__(256) void km_row_sumsq_kernel(
    const float* __restrict__ rows, int64_t row_stride, KmRowMap map,
    int64_t n, int dim, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const int64_t rc = r < n ? r : n - 1;
    const float* rp = rows + km_src_row(map, rc) * row_stride;
    double s = 0.0;
    for (int e = threadIdx.x & 7; e < dim; e += 8)
        s += (double)rp[e] * (double)rp[e];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if ((threadIdx.x & 7) == 0 && r < n)
        out[r] = INV ? (s > 0.0 ? (float)(1.0 / sqrt(s)) : 0.f) : (float)s;
}

/* One block per (centroid, 32-dim slab): thread (dl, rl) sums the members
 * rl, rl+8, ... of its dim in CSR order (f64), the 8 partials meet in a
 * fixed tree, the sum is divided by the count. No atomics: the same input
 * gives the same bits. An empty centroid is left as it was. */
__global__ __launch_bounds__(256) void km_update_kernel(
    const float* __restrict__ rows, int64_t row_stride, KmRowMap map,
    const int64_t* __restrict__ offs,   /* [k+1] CSR offsets               */
    const int32_t* __restrict__ members, /* training rows, grouped, ascending */
    const float* __restrict__ inv_norm, /* [n_train] or null (spherical)   */
    int dim, int dpad, float* __restrict__ cents) {
    __shared__ double part[8][32];
    const int c = blockIdx.x, dl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int d = blockIdx.y * 32 + dl;
    const int64_t beg = offs[c], end = offs[c + 1];
    if (beg == end) return; /* block-uniform */
    double s = 0.0;
    if (d < dim)
        for (int64_t m = beg + rl; m < end; m += 8) {
            const int64_t i = members[m];
            double v = rows[km_src_row(map, i) * row_stride + d];
            if (inv_norm) v *= (double)inv_norm[i];
            s += v;
        }
    part[rl][dl] = s;
    __syncthreads();
    if (rl == 0 && d < dim) {
        const double tot =
            ((part[0][dl] + part[1][dl]) + (part[2][dl] + part[3][dl])) +
            ((part[4][dl] + part[5][dl]) + (part[6][dl] + part[7][dl]));
        cents[(int64_t)c * dpad + d] = (float)(tot / (double)(end - beg));
    }
}

/* cents[cidx[b]] = training row trow[b] (init and reseed); pad stays zero */
__global__ __launch_bounds__(256) void km_set_centroids_kernel(
    const float* __restrict__ rows, int64_t row_stride, KmRowMap map,
    const int32_t* __restrict__ cidx, const int64_t* __restrict__ trow,
    int dim, int dpad, float* __restrict__ cents) {
    const float* rp =
        rows + km_src_row(map, trow[blockIdx.x]) * row_stride;
    float* cp = cents + (int64_t)cidx[blockIdx.x] * dpad;
    for (int e = threadIdx.x; e < dim; e += blockDim.x) cp[e] = rp[e];
}

/* rows [i0, i0+cnt) of the mapped row set -> [cnt][dpad], zero-padded (the
 * operand of the MOANN_KMEANS_ASSIGN=gemm composition) */
__global__ __launch_bounds__(256) void km_gather_pad_kernel(
    const float* __restrict__ rows, int64_t row_stride, KmRowMap map,
    int64_t i0, int dim, int dpad, float* __restrict__ out) {
    const float* rp =
        rows + km_src_row(map, i0 + blockIdx.x) * row_stride;
    float* op = out + (int64_t)blockIdx.x * dpad;
    for (int e = threadIdx.x; e < dpad; e += blockDim.x)
        op[e] = e < dim ? rp[e] : 0.f;
}

}  // namespace

void launch_km_assign(int metric, const float* rows, int64_t row_stride,
                      KmRowMap map, int64_t n, const float* cents,
                      const float* cnorms, int k, int dim, int dpad,
                      int32_t* assign, float* best, hipStream_t stream) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + KA_ROWS - 1) / KA_ROWS)), block(256);
    switch (metric) {
    case KM_L2SQ:
        hipLaunchKernelGGL((assign_argmin_kernel<KM_L2SQ>), grid, block, 0,
                           stream, rows, row_stride, map, n, cents, cnorms, k,
                           dim, dpad, assign, best);
        break;
    case KM_IP:
        hipLaunchKernelGGL((assign_argmin_kernel<KM_IP>), grid, block, 0,
                           stream, rows, row_stride, map, n, cents, cnorms, k,
                           dim, dpad, assign, best);
        break;
    case KM_COS:
        hipLaunchKernelGGL((assign_argmin_kernel<KM_COS>), grid, block, 0,
                           stream, rows, row_stride, map, n, cents, cnorms, k,
                           dim, dpad, assign, best);
        break;
    default:
        throw std::logic_error("launch_km_assign: metric has no MFMA form");
    }
}

void launch_km_row_sumsq(bool inverse_norm, const float* rows,
                         int64_t row_stride, KmRowMap map, int64_t n, int dim,
                         float* out, hipStream_t stream) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 31) / 32)), block(256);
    if (inverse_norm)
        hipLaunchKernelGGL((km_row_sumsq_kernel<true>), grid, block, 0, stream,
                           rows, row_stride, map, n, dim, out);
    else
        hipLaunchKernelGGL((km_row_sumsq_kernel<false>), grid, block, 0,
                           stream, rows, row_stride, map, n, dim, out);
}

void launch_km_update(const float* rows, int64_t row_stride, KmRowMap map,
                      const int64_t* offs, const int32_t* members,
                      const float* inv_norm, int k, int dim, int dpad,
                      float* cents, hipStream_t stream) {
    hipLaunchKernelGGL(km_update_kernel, dim3(k, (dim + 31) / 32), dim3(256),
                       0, stream, rows, row_stride, map, offs, members,
                       inv_norm, dim, dpad, cents);
}

void launch_km_set_centroids(const float* rows, int64_t row_stride,
                             KmRowMap map, const int32_t* cidx,
                             const int64_t* trow, int count, int dim, int dpad,
                             float* cents, hipStream_t stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(km_set_centroids_kernel, dim3(count), dim3(256), 0,
                       stream, rows, row_stride, map, cidx, trow, dim, dpad,
                       cents);
}

void launch_km_gather_pad(const float* rows, int64_t row_stride, KmRowMap map,
                          int64_t i0, int64_t count, int dim, int dpad,
                          float* out, hipStream_t stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(km_gather_pad_kernel, dim3((unsigned)count), dim3(256),
                       0, stream, rows, row_stride, map, i0, dim, dpad, out);
}

}  // namespace moann
