/* Shared host-side helpers for the moann C-ABI libraries (IVF-Flat, HNSW,
 * IVF-PQ). Internal — not part of the public ABI. */

#ifndef MOANN_HOST_COMMON_H
#define MOANN_HOST_COMMON_H

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "moann_internal.h"  /* ScanJobs */
#include "moann_scan_plan.h" /* HostScanJobs */

namespace moann {

#define MOANN_HIP_CHECK(expr)                                               \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess)                                               \
            throw std::runtime_error(std::string("HIP error: ") +           \
                                     hipGetErrorString(_e) + " at " #expr); \
    } while (0)

#define MOANN_KCHECK(tag)                                                    \
    do {                                                                     \
        hipError_t _e = hipGetLastError();                                   \
        if (_e != hipSuccess)                                                \
            throw std::runtime_error(std::string("HIP launch error [") +     \
                                     tag + "]: " + hipGetErrorString(_e));   \
    } while (0)

/* errmsg convention: cgo/cuvs/helper.h:59 — errmsg is a char** as void*. */
inline void moann_set_errmsg(void* errmsg, const char* context,
                             const char* message) {
    if (!errmsg) return;
    std::string full = std::string(context) + ": " + message;
    *(char**)errmsg = strdup(full.c_str());
}

/* The result object behind gpu_ivf_flat_result_c — ALL index families
 * return this type so the gpu_ivf_flat_get_neighbors/get_distances/
 * free_result readout (ivf_flat_c.h:139-141) works for every search. */
struct MoannResult {
    std::vector<int64_t> neighbors;
    std::vector<float> distances;
    /* async pipeline (moann_ivf_flat_search_submit): while !collected the
     * payload lives in the owning SearchCtx's pinned bounce buffer and
     * done_ev marks the D2H completion on that ctx's stream. */
    void* owner = nullptr;        /* SearchCtx* (IVF lib) or null          */
    hipEvent_t done_ev = nullptr; /* owned by the result; null => sync    */
    bool collected = true;
    /* extend support: the tail sub-index's (already collected) result,
     * top-k merged into this one at collect (gpu_ivf_flat_extend) */
    std::unique_ptr<MoannResult> tail_res;
    int merge_kmetric = 0;   /* KM_* of the owning index (IP merge order) */
    uint32_t merge_limit = 0; /* row stride (limit) for the tail merge */
    bool tail_merged = false;
};

/* grow-only device buffer (cuvs_worker.hpp:50-150 shape, minus RMM) */
struct MoannDevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    void ensure(size_t need) {
        if (need <= bytes) return;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        MOANN_HIP_CHECK(hipMalloc(&ptr, need));
        bytes = need;
    }
    ~MoannDevBuf() {
        if (ptr) (void)hipFree(ptr);
    }
    template <typename T>
    T* as() { return (T*)ptr; }
};

/* Grow `buf` to fit a host vector and enqueue its H2D copy; the vector must
 * stay untouched until the copy has run. */
template <typename T>
inline void upload_vector(MoannDevBuf& buf, const std::vector<T>& v,
                          hipStream_t s) {
    buf.ensure(v.size() * sizeof(T));
    MOANN_HIP_CHECK(hipMemcpyAsync(buf.ptr, v.data(), v.size() * sizeof(T),
                                   hipMemcpyHostToDevice, s));
}

/* Queries to the device as [nq][dpad] f32 rows, zero-padded past dim. */
inline const float* stage_padded_queries(MoannDevBuf& buf, const float* src,
                                         bool src_on_device, uint64_t nq,
                                         uint32_t dim, uint32_t dpad,
                                         hipStream_t s) {
    buf.ensure((size_t)nq * dpad * 4);
    if (dim != dpad)
        MOANN_HIP_CHECK(hipMemsetAsync(buf.ptr, 0, (size_t)nq * dpad * 4, s));
    MOANN_HIP_CHECK(hipMemcpy2DAsync(
        buf.ptr, (size_t)dpad * 4, src, (size_t)dim * 4, (size_t)dim * 4, nq,
        src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    return buf.as<float>();
}

/* Bump-allocate a host job table's SoA arrays (8-byte aligned) in `buf` and
 * enqueue their H2D copies on `stream`. `h` must stay untouched until those
 * copies have run. An empty slot_base (rank scan) uploads as null. */
inline ScanJobs upload_scan_jobs(const HostScanJobs& h, MoannDevBuf& buf,
                                 hipStream_t stream) {
    auto al8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
    const size_t nj = (size_t)h.njobs, ns = (size_t)h.nqslots;
    buf.ensure(2 * al8(nj * 8) + 5 * al8(nj * 4) + al8(ns * 4) +
               al8(ns * 8) + 64);
    uint8_t* p = buf.as<uint8_t>();
    auto up = [&](const auto& v) {
        using T = typename std::decay_t<decltype(v)>::value_type;
        const size_t bytes = v.size() * sizeof(T);
        if (!bytes) return (const T*)nullptr;
        MOANN_HIP_CHECK(hipMemcpyAsync(p, v.data(), bytes,
                                       hipMemcpyHostToDevice, stream));
        const T* r = (const T*)p;
        p += al8(bytes);
        return r;
    };
    /* ScanJobs member order (and the copy order the libraries always used) */
    return ScanJobs {up(h.databaseg), up(h.gstart), up(h.gcount), up(h.rows),
                     up(h.nq), up(h.qbase), up(h.qslot_query),
                     up(h.qslot_outbase), up(h.slot_base), h.njobs};
}

}  // namespace moann

#endif
