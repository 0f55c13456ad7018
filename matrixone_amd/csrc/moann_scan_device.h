/* Device pieces shared by the list-scan kernels (scan_kernel, scan_h_kernel,
 * scan_i8_kernel, scan_i8_dot_kernel, scan_asm768_kernel; scan_i8_mfma_kernel
 * takes load_job, slot_passes and finish_i32 and has a tile stage and store
 * of its own shape): everything around their inner dimension loops, plus the two conventions other kernels share
 * (the membership-filter bit test and MO's cosine distance). Each is stated
 * once, here. `__device__ __forceinline__` functions only. */

#ifndef MOANN_SCAN_DEVICE_H
#define MOANN_SCAN_DEVICE_H

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>

#include "moann_internal.h"

namespace moann {

/* XCD-aware bijective blockIdx remap (T1): the dispatcher places block
 * b on XCD b%8; this permutation gives each XCD a CONTIGUOUS job range,
 * so the query tiles of one list (consecutive jobs) stream through one
 * XCD's L2 instead of re-fetching from HBM on every XCD. */
__device__ __forceinline__ int scan_job_index() {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int j =
        (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    return j < nwg ? j : bid; /* safety: cannot happen for bijective map */
}

/* This workgroup's row of the job table. */
struct JobView {
    int j;         /* job index (after the XCD remap)                        */
    int nq, qbase; /* queries in the tile, offset into the qslot arrays      */
    int gstart, gcount, rows;
    int64_t baseg;
};

__device__ __forceinline__ JobView load_job(const ScanJobs& jobs) {
    JobView v;
    v.j = scan_job_index();
    v.nq = jobs.nq[v.j];
    v.qbase = jobs.qbase[v.j];
    v.gstart = jobs.gstart[v.j];
    v.gcount = jobs.gcount[v.j];
    v.rows = jobs.rows[v.j];
    v.baseg = jobs.databaseg[v.j];
    return v;
}

/* Stage the job's query tile into LDS: ldsq[QT][dpad] elements, and
 * ldsn[QT] norms when NEED_NORM; tile slots t >= nq are zero-filled so the
 * inner loops need no tile bound. Ends in the barrier. */
template <int QT, bool NEED_NORM, typename QE, typename NE>
__device__ __forceinline__ void stage_query_tile(
    const JobView& jv, const int32_t* __restrict__ qslot_query,
    const QE* __restrict__ queries, const NE* __restrict__ qnorms, int dpad,
    QE* ldsq, NE* ldsn) {
    /* Code generation, not semantics: the five hand-written copies read
     * blockDim.x inside the copy loops and compiled to a scalar load. From
     * this shared function the same text made hipcc keep the
     * partial-workgroup select in the t < nq branch and fetch the size with
     * one global_load_ushort per tile slot. Reading it once here brings the
     * scalar load back; the loop vectorizer then versions the strided copies
     * for a stride of 1 (twice the code, 3x the vector-memory instructions),
     * hence vectorize(disable). With both, each kernel's count of
     * vector-memory instructions equals the hand-written copy's. */
    const int nthreads = blockDim.x;
    for (int t = 0; t < QT; ++t) {
        if (t < jv.nq) {
            const int q = qslot_query[jv.qbase + t];
            const QE* src = queries + (int64_t)q * dpad;
#pragma clang loop vectorize(disable)
            for (int e = threadIdx.x; e < dpad; e += nthreads)
                ldsq[t * dpad + e] = src[e];
            if (NEED_NORM && threadIdx.x == 0) ldsn[t] = qnorms[q];
        } else {
#pragma clang loop vectorize(disable)
            for (int e = threadIdx.x; e < dpad; e += nthreads)
                ldsq[t * dpad + e] = QE(0);
            if (NEED_NORM && threadIdx.x == 0) ldsn[t] = NE(0);
        }
    }
    __syncthreads();
}

/* Membership filter: one bit per GLOBAL slot; a cleared bit excludes the
 * entry (cuVS bitset_filter precedent, cgo/cuvs/ivf_flat.hpp:908-924). The
 * caller handles the null (unfiltered) bitset. */
__device__ __forceinline__ bool slot_passes(
    const uint32_t* __restrict__ filter_bitset, int64_t global_slot) {
    return (filter_bitset[global_slot >> 5] >> (global_slot & 31)) & 1u;
}

/* MO's cosine distance (metric/distance_func.go:211-286; integer sums ->
 * double per distance_func_narrow.go:444-449): norms are sums of squares,
 * the denominator is a double product of square roots, the similarity is
 * clamped to [-1, 1], and a zero denominator gives distance 1. */
__device__ __forceinline__ float mo_cos_distance(double dot, double rn,
                                                 double qn) {
    const double denom = sqrt(rn) * sqrt(qn);
    if (denom == 0.0) return 1.0f;
    double sim = dot / denom;
    sim = sim > 1.0 ? 1.0 : (sim < -1.0 ? -1.0 : sim);
    return (float)(1.0 - sim);
}

/* Accumulator -> MO distance. IP is negated (distance_func.go:207). */
template <int METRIC>
__device__ __forceinline__ float finish_f32(float acc, float rn, float qn) {
    if (METRIC == KM_IP) return -acc;
    if (METRIC == KM_COS) return mo_cos_distance(acc, rn, qn);
    return acc;
}

/* Integer accumulators; DOT_FORM L2sq is rn + qn - 2*dot (exact in int32). */
template <int METRIC, bool DOT_FORM>
__device__ __forceinline__ float finish_i32(int32_t acc, int32_t rn,
                                            int32_t qn) {
    if (METRIC == KM_IP) return (float)(-(int64_t)acc);
    if (METRIC == KM_COS) return mo_cos_distance(acc, rn, qn);
    if (METRIC == KM_L2SQ && DOT_FORM) return (float)(rn + qn - 2 * acc);
    return (float)acc;
}

/* Epilogue of one group pair (g0, g1): each lane owns row g*64+lane of both
 * groups. Filter test once per row, then for every query of the tile
 * dists_out[outbase + row] = finish(acc, row norm, query norm), FLT_MAX for
 * a filtered-out row. has1 == false is the single-row form (g1's arguments
 * are ignored). ldsn is read only when NEED_NORM. */
template <int QT, bool NEED_NORM, typename ACC, typename NE, typename FIN>
__device__ __forceinline__ void store_group_pair(
    const ScanJobs& jobs, const JobView& jv, int lane, int g0, int g1,
    bool has1, const ACC (&acc0)[QT], const ACC (&acc1)[QT], NE rn0, NE rn1,
    const NE* ldsn, const uint32_t* __restrict__ filter_bitset,
    float* __restrict__ dists_out, FIN finish) {
    const int row0 = g0 * 64 + lane;
    const int row1 = g1 * 64 + lane;
    const bool live0 = row0 < jv.rows;
    const bool live1 = has1 && row1 < jv.rows;
    bool pass0 = true, pass1 = true;
    if (filter_bitset) {
        const int64_t sb = jobs.slot_base[jv.j];
        if (live0) pass0 = slot_passes(filter_bitset, sb + row0);
        if (live1) pass1 = slot_passes(filter_bitset, sb + row1);
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        if (t >= jv.nq) break;
        const int64_t ob = jobs.qslot_outbase[jv.qbase + t];
        const NE qn = NEED_NORM ? ldsn[t] : NE(0);
        if (live0)
            dists_out[ob + row0] = pass0 ? finish(acc0[t], rn0, qn) : FLT_MAX;
        if (live1)
            dists_out[ob + row1] = pass1 ? finish(acc1[t], rn1, qn) : FLT_MAX;
    }
}

}  // namespace moann

#endif
