/* libmoann_hip — host side of the MI355X-native MatrixOne ANN search backend.
 *
 * Implements the C ABI of include/moann.h (mirroring cgo/cuvs/ivf_flat_c.h,
 * the interface MatrixOne's Go cgo layer binds for this path). Index state
 * management follows the contract of cgo/cuvs/index_base.hpp:104-251 (shared
 * mutex on host state, kernels run unlocked on the index's stream, caller-
 * allocated result buffers, errmsg out-params per cgo/cuvs/helper.h:59) —
 * re-designed for one device per process (multi-GPU distribution lives in the
 * host layer as one process per GPU + RCCL), HIP streams and
 * grow-only hipMalloc workspaces instead of RAFT/RMM pools.
 */

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <unordered_map>
#include <memory>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <chrono>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/moann.h"
#include "moann_host_common.h"
#include "moann_kmeans_plan.h"
#include "moann_select_plan.h"

namespace {

using namespace moann;

/* local short names for the shared helpers (moann_host_common.h) */
#define HIP_CHECK MOANN_HIP_CHECK
#define KCHECK MOANN_KCHECK
using DevBuf = MoannDevBuf;
constexpr auto set_errmsg = moann_set_errmsg;

using Result = MoannResult;  /* shared with the PQ/HNSW libs so the
    gpu_ivf_flat_get_* readout works on every family's results */

struct PerfState {
    moann_perf_t c {};
    hipEvent_t ev[8] {};  /* rank0, rank1, scan0, scan1, sel0, sel1, all0, all1 */
    bool made = false;
    void ensure() {
        if (made) return;
        for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
        made = true;
    }
    ~PerfState() {
        if (made)
            for (auto& e : ev) (void)hipEventDestroy(e);
    }
};

/* One in-flight search pipeline: its own stream, perf events, grow-only
 * workspaces and a pinned result bounce buffer. IvfIndex keeps two, so
 * consecutive moann_ivf_flat_search_submit calls overlap: batch B's rank +
 * host job build run while batch A's list scan still owns the other stream
 * (the GPU otherwise idles ~0.8 ms per step; dynamic_batching.hpp's
 * overlapping-worker precedent, redesigned around two HIP streams). */
struct SearchCtx {
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] {}; /* rank0,rank1, scan0,scan1, sel0,sel1 */
    bool made = false;
    DevBuf w_queries, w_qnorms, w_cdists, w_csel_slots, w_csel_dists;
    DevBuf w_jobs, w_qslots, w_cand, w_sel_slots, w_sel_dists;
    DevBuf w_probe_lists, w_probe_offs, w_qoffs, w_out_ids, w_out_dists;
    DevBuf w_filter, w_queries_q, w_qnorms_i;
    DevBuf w_rsel_slots, w_rsel_dists, w_refined, w_sel2; /* refine stage */
    void* h_out = nullptr;   /* pinned [ids int64][dists f32] bounce */
    size_t h_out_bytes = 0;
    std::vector<uint32_t> h_filter; /* staged filter words: must outlive the
        async H2D when the submit path returns before the copy runs */
    /* host side of the scan plan, reused across searches (same lifetime
     * rule: their async H2D copies complete before this ctx is reused) */
    std::vector<int32_t> h_probe; /* [nq][probe] probed lists, rank order */
    HostScanJobs rank_jobs;
    ProbeOffsets offs;
    ListScanPlan lists;
    struct Call { /* the search in flight through the stages below */
        uint64_t nq = 0;
        uint32_t limit = 0, probe = 0;
        ScanChoice scan {};
        bool refine = false;            /* two-stage scan active            */
        bool outputs_written = false;   /* fused refine tail filled w_out_* */
        const float* d_q = nullptr;     /* [nq][dpad] padded queries        */
        const float* d_qn = nullptr;    /* [nq] |q|^2, when a stage needs it */
    } call;
    MoannResult* pending = nullptr; /* submitted, not yet collected */
    void* parent = nullptr;         /* IvfIndex*, for perf accumulation */
    void ensure(void* ix) {
        parent = ix;
        if (made) return;
        HIP_CHECK(hipStreamCreate(&stream));
        for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
        made = true;
    }
    void ensure_hout(size_t need) {
        if (need <= h_out_bytes) return;
        if (h_out) (void)hipHostFree(h_out);
        h_out = nullptr;
        h_out_bytes = 0;
        HIP_CHECK(hipHostMalloc(&h_out, need));
        h_out_bytes = need;
    }
    ~SearchCtx() {
        if (made) {
            (void)hipStreamDestroy(stream);
            for (auto& e : ev) (void)hipEventDestroy(e);
        }
        if (h_out) (void)hipHostFree(h_out);
    }
};

const ScanOverrides& scan_overrides(); /* below */

struct IvfIndex {
    /* config */
    int device = 0;
    uint32_t dim = 0, dpad = 0, nlist = 0;
    distance_type_t metric = DistanceType_L2Expanded;
    int kmetric = KM_L2SQ;
    uint64_t cap = 0, count = 0;
    quantization_t btype = Quantization_F32; /* base/query element type    */
    quantization_t qtype = Quantization_F32;
    double quant_mul = 1.0, quant_add = 0.0; /* identity until trained */
    double quant_min = 0.0, quant_max = 0.0;
    uint8_t* d_packed_q = nullptr;  /* quantized interleaved entries */
    int32_t* d_rownorm_q = nullptr; /* [total_groups*64] byte-row |x|^2 */
    /* two-stage scan (moann_ivf_flat_enable_refine): byte first pass over
     * an INTERNAL clip-quantized image, exact f32 re-rank of the top-R */
    int refine_depth = 0;
    float* d_rows_f32 = nullptr;    /* [count][dim] slot-major (refine) */
    uint8_t* d_packed_rq = nullptr; /* clip-quantized interleaved image */
    ByteImageLayout rq_layout = ByteImageLayout::ROWS16; /* its byte order */
    int32_t* d_rownorm_rq = nullptr;
    double rq_mul = 1.0, rq_add = 0.0;
    /* selection and refine tail (moann_ivf_flat_set_refine_tail): legacy =
     * radix select for every selection and the four-kernel refine tail */
    bool refine_tail_legacy = scan_overrides().refine_tail_legacy;
    unsigned long long* d_select_stats = nullptr; /* [2] filtered, fallback */
    bool built = false, started = false;

    hipStream_t stream = nullptr;

    /* staging (host mirrors + device raw rows, dropped after build) */
    std::vector<int64_t> h_ids;
    std::vector<int32_t> h_assign;
    std::vector<float> h_centroids;
    float* d_staging = nullptr;
    /* native k-means build (moann_kmeans_plan.h): build_params fraction,
     * moann_ivf_flat_set_kmeans_params knobs (0 = default / no cap), and
     * what the last build spent (moann_ivf_flat_kmeans_stats) */
    double km_fraction = KMEANS_DEFAULT_FRACTION;
    uint32_t km_iters = 0;
    uint64_t km_max_train = 0;
    double km_train_ms = 0.0, km_assign_ms = 0.0;
    uint32_t km_iters_run = 0;
    uint64_t km_n_train = 0;

    /* built state */
    float* d_packed = nullptr;           /* interleaved entry data            */
    float* d_cent_packed = nullptr;      /* interleaved centroid matrix       */
    float* d_cent_rows = nullptr;        /* [nlist][dpad] row-major (MFMA)    */
    float* d_cnorms = nullptr;           /* [nlist] |c|^2 (MFMA rank)         */
    bool rank_mfma = false;              /* MOANN_RANK=mfma opt-in            */
    int64_t* d_id_by_slot = nullptr;     /* [total_slots]                     */
    int64_t* d_list_slot_base = nullptr; /* [nlist]                           */
    std::vector<int64_t> list_gbase;     /* group base per list               */
    std::vector<int64_t> group_slotbase; /* per group: global slot of lane 0  */
    std::vector<int32_t> group_valid;    /* per group: valid rows             */
    std::vector<int32_t> list_rows;      /* rows per list                     */
    std::vector<int64_t> list_slot_base; /* slot base per list                */
    int64_t total_groups = 0;
    int64_t cent_groups = 0;

    /* per-call workspaces: two pipeline contexts (submit/wait overlap) */
    SearchCtx sctx[2];
    uint64_t sparity = 0;
    std::vector<int64_t> h_id_by_slot;  /* kept for the membership filter */
    std::vector<int64_t> h_slot_rows;   /* slot -> add-order row (pred filter) */
    std::unordered_map<int64_t, int64_t> id_to_slot; /* lazy */

    std::mutex mu;
    PerfState perf;

    std::map<uint64_t, std::unique_ptr<Result>> jobs;
    uint64_t next_job = 1;

    /* dynamic request batching (cgo/cuvs/dynamic_batching.hpp:19-60 shape:
     * coalesce concurrent small search_async calls inside a µs window) */
    std::atomic<int64_t> batch_window_us {0};
    struct PendingReq {
        std::vector<float> queries;
        uint64_t nq;
        uint32_t limit, nprobe;
        uint64_t job_id;
    };
    std::mutex bmu;
    std::condition_variable bcv;       /* worker wakeup */
    std::condition_variable bdone_cv;  /* waiters */
    std::vector<PendingReq> pending;
    std::map<uint64_t, std::unique_ptr<Result>> done_jobs;
    std::thread batcher;
    bool batcher_stop = false;
    bool batcher_started = false;
    bool dynb_conservative = false; /* ivf_flat_c.h:92 knob (recorded) */

    /* post-build extends (gpu_ivf_flat_extend/_float): a per-list TAIL
     * sub-index over the extended rows, same centroids/metric/quantizer,
     * rebuilt from host staging on each extend (O(tail) per call) and
     * searched alongside the main lists with a top-k merge at collect —
     * result-identical to the reference's in-list insertion
     * (cuvs::ivf_flat::extend): a row participates exactly when its
     * assigned list is probed. */
    std::shared_ptr<IvfIndex> tail; /* shared: searches snapshot it under
        mu so a concurrent extend's rebuild cannot free it mid-search */
    std::vector<float> tail_staging;   /* f32 rows, extend order */
    std::vector<int64_t> tail_ids;
    std::vector<int32_t> tail_assign;
    std::vector<int64_t> tail_deleted; /* deletes re-applied on rebuild */

    /* soft-delete bitset (index_base.hpp:183-209): bit per SLOT, 1 = alive,
     * lazily allocated on first delete. Applied to every search by ANDing
     * into the membership filter. */
    std::vector<uint32_t> alive;
    uint64_t deleted_count = 0;

    /* pre-filter INCLUDE columns (ivf_flat_c.h:165-177): raw column bytes
     * in ADD order + null bitmaps, registered before build */
    std::string filter_cols_json;
    std::vector<int> filter_col_types;
    std::vector<std::vector<uint8_t>> filter_col_data;
    std::vector<std::vector<uint32_t>> filter_col_nulls;
    std::vector<uint64_t> filter_col_rows;
    std::vector<bool> filter_col_has_nulls;

    ~IvfIndex() {
        if (batcher_started) {
            {
                std::lock_guard<std::mutex> lk(bmu);
                batcher_stop = true;
            }
            bcv.notify_all();
            batcher.join();
        }
        (void)hipSetDevice(device);
        for (auto p : {(void*)d_staging, (void*)d_packed, (void*)d_cent_packed,
                       (void*)d_cent_rows, (void*)d_cnorms, (void*)d_packed_q,
                       (void*)d_rownorm_q, (void*)d_rows_f32,
                       (void*)d_packed_rq, (void*)d_rownorm_rq,
                       (void*)d_id_by_slot, (void*)d_list_slot_base,
                       (void*)d_select_stats})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

/* Build the interleaved layout for an arbitrary row set (used for both the
 * entry lists and the centroid matrix-as-one-list). */
void pack_lists(IvfIndex* ix, const float* d_rows, int64_t nrows,
                const std::vector<int64_t>& slot_rows,
                const std::vector<int64_t>& loffsets, /* [nlists+1] slots */
                float** d_packed_out, std::vector<int64_t>* gbase_out,
                int64_t* ngroups_out) {
    (void)nrows; /* implicit in loffsets */
    const int64_t nlists = (int64_t)loffsets.size() - 1;
    std::vector<int64_t> gbase(nlists + 1, 0);
    for (int64_t l = 0; l < nlists; ++l) {
        const int64_t rows = loffsets[l + 1] - loffsets[l];
        gbase[l + 1] = gbase[l] + (rows + 63) / 64;
    }
    const int64_t ngroups = gbase[nlists];
    std::vector<int64_t> group_rowbase(ngroups);
    std::vector<int32_t> group_valid(ngroups);
    for (int64_t l = 0; l < nlists; ++l) {
        const int64_t rows = loffsets[l + 1] - loffsets[l];
        for (int64_t g = gbase[l]; g < gbase[l + 1]; ++g) {
            const int64_t gi = g - gbase[l];
            group_rowbase[g] = loffsets[l] + gi * 64;
            const int64_t rem = rows - gi * 64;
            group_valid[g] = (int32_t)std::min<int64_t>(64, rem);
        }
    }
    float* d_packed = nullptr;
    HIP_CHECK(hipMalloc(&d_packed,
                        (size_t)ngroups * 64 * ix->dpad * sizeof(float)));
    DevBuf tmp_rb, tmp_gv, tmp_sr;
    tmp_rb.ensure(ngroups * sizeof(int64_t));
    tmp_gv.ensure(ngroups * sizeof(int32_t));
    tmp_sr.ensure(std::max<size_t>(1, slot_rows.size() * sizeof(int64_t)));
    HIP_CHECK(hipMemcpyAsync(tmp_rb.ptr, group_rowbase.data(),
                             ngroups * sizeof(int64_t), hipMemcpyHostToDevice,
                             ix->stream));
    HIP_CHECK(hipMemcpyAsync(tmp_gv.ptr, group_valid.data(),
                             ngroups * sizeof(int32_t), hipMemcpyHostToDevice,
                             ix->stream));
    if (!slot_rows.empty())
        HIP_CHECK(hipMemcpyAsync(tmp_sr.ptr, slot_rows.data(),
                                 slot_rows.size() * sizeof(int64_t),
                                 hipMemcpyHostToDevice, ix->stream));
    launch_pack(d_rows, (int)ix->dim, (int)ix->dpad, tmp_rb.as<int64_t>(),
                tmp_gv.as<int32_t>(), tmp_sr.as<int64_t>(), ngroups, d_packed,
                ix->stream);
    KCHECK("pack");
    HIP_CHECK(hipStreamSynchronize(ix->stream));
    HIP_CHECK(hipGetLastError());
    *d_packed_out = d_packed;
    if (gbase_out) *gbase_out = std::move(gbase);
    *ngroups_out = ngroups;
}

/* ---------------- host-side element conversions (ABI edges) -------------- */

float half_to_f32(uint16_t b) {
    const uint32_t s = (uint32_t)(b >> 15) << 31;
    uint32_t e = (b >> 10) & 0x1f, m = b & 0x3ff;
    uint32_t out;
    if (e == 0) {
        if (m == 0) out = s;
        else { /* subnormal */
            e = 127 - 14;
            while (!(m & 0x400)) { m <<= 1; --e; }
            m &= 0x3ff;
            out = s | (e << 23) | (m << 13);
        }
    } else if (e == 31) {
        out = s | 0x7f800000u | (m << 13);
    } else {
        out = s | ((e + 112) << 23) | (m << 13);
    }
    float f;
    memcpy(&f, &out, 4);
    return f;
}

float bf16_to_f32(uint16_t b) {
    const uint32_t out = (uint32_t)b << 16;
    float f;
    memcpy(&f, &out, 4);
    return f;
}

/* storage-typed rows -> f32 staging rows. The affine byte map round-trips
 * exactly (|code| <= 255: dequant->requant errors are ~1e-5 code steps, far
 * inside the round-to-nearest window), halves are exact casts — so staging
 * narrow input as f32 and re-quantizing at build reproduces the caller's
 * bytes bit-for-bit. */
void storage_to_f32(quantization_t st, const void* src, size_t n,
                    double mul, double add, float* dst) {
    switch (st) {
    case Quantization_F32:
        memcpy(dst, src, n * 4);
        break;
    case Quantization_INT8: {
        const int8_t* p = (const int8_t*)src;
        const double m = mul == 0.0 ? 1.0 : mul;
        for (size_t i = 0; i < n; ++i)
            dst[i] = (float)(((double)p[i] - add) / m);
        break;
    }
    case Quantization_UINT8: {
        const uint8_t* p = (const uint8_t*)src;
        const double m = mul == 0.0 ? 1.0 : mul;
        for (size_t i = 0; i < n; ++i)
            dst[i] = (float)(((double)p[i] - add) / m);
        break;
    }
    case Quantization_F16: {
        const uint16_t* p = (const uint16_t*)src;
        for (size_t i = 0; i < n; ++i) dst[i] = half_to_f32(p[i]);
        break;
    }
    case Quantization_BF16: {
        const uint16_t* p = (const uint16_t*)src;
        for (size_t i = 0; i < n; ++i) dst[i] = bf16_to_f32(p[i]);
        break;
    }
    default:
        throw std::runtime_error("unsupported storage type");
    }
}

size_t storage_elem_bytes(quantization_t st) {
    return st == Quantization_F32 ? 4
           : (st == Quantization_F16 || st == Quantization_BF16) ? 2 : 1;
}

/* base-typed queries (B = f32 or f16, ivf_flat_c.h:33-35) -> f32 */
std::vector<float> base_to_f32(quantization_t btype, const void* src,
                               size_t n) {
    std::vector<float> out(n);
    if (btype == Quantization_F32) memcpy(out.data(), src, n * 4);
    else if (btype == Quantization_F16) {
        const uint16_t* p = (const uint16_t*)src;
        for (size_t i = 0; i < n; ++i) out[i] = half_to_f32(p[i]);
    } else throw std::runtime_error("base type must be F32 or F16");
    return out;
}

/* ------------------------- the search pipeline -------------------------- */

double collect_result(MoannResult* res); /* below; returns kernel-window ms */

/* The A/B tuning environment of the scan path, read once per process: the
 * only getenv on it (MOANN_RANK is read where the build picks the rank). */
const ScanOverrides& scan_overrides() {
    static const ScanOverrides ov = [] {
        const char *sc = getenv("MOANN_SCAN"), *bq = getenv("MOANN_BYTE_QT"),
                   *cg = getenv("MOANN_CHUNKG"),
                   *bm = getenv("MOANN_BYTE_MFMA"),
                   *rt = getenv("MOANN_REFINE_TAIL");
        ScanOverrides o;
        o.refine_tail_legacy = rt && strcmp(rt, "legacy") == 0;
        o.generic_f32 = sc && strcmp(sc, "generic") == 0;
        o.byte_qt8 = bq && atoi(bq) == 8;
        o.chunk_g = cg ? atoi(cg) : 0;
        o.byte_mfma_off = bm && strcmp(bm, "0") == 0;
        return o;
    }();
    return ov;
}

/* run_search is the stages below in order, all enqueued on cx->stream; the
 * per-call state they share is cx->call.
 * 1. queries to device, padded to dpad (+ |q|^2 where a stage needs it) */
void stage_queries(IvfIndex* ix, SearchCtx* cx, const float* queries,
                   bool queries_on_device) {
    SearchCtx::Call& c = cx->call;
    const int dpad = (int)ix->dpad;
    const hipStream_t s = cx->stream;
    c.d_q = stage_padded_queries(cx->w_queries, queries, queries_on_device,
                                 c.nq, ix->dim, ix->dpad, s);
    c.d_qn = nullptr;
    const bool use_mfma_rank = ix->rank_mfma && ix->kmetric != KM_L1;
    if (ix->kmetric == KM_COS || use_mfma_rank) {
        cx->w_qnorms.ensure(c.nq * 4);
        launch_qnorms(c.d_q, (int)c.nq, dpad, cx->w_qnorms.as<float>(), s);
        KCHECK("qnorms");
        c.d_qn = cx->w_qnorms.as<float>();
    }
}

/* 2. centroid rank: scan the centroid matrix as one "list" of nlist rows (or
 * the MFMA GEMM), then top-probe per query (search.go:265-308 rankCentroids) */
void rank_centroids(IvfIndex* ix, SearchCtx* cx) {
    const SearchCtx::Call& c = cx->call;
    const int dpad = (int)ix->dpad, nq = (int)c.nq;
    const hipStream_t s = cx->stream;
    cx->w_cdists.ensure((size_t)c.nq * ix->nlist * 4);
    if (ix->rank_mfma && ix->kmetric != KM_L1) {
        HIP_CHECK(hipEventRecord(cx->ev[0], s));
        launch_rank_gemm(ix->kmetric, c.d_q, ix->d_cent_rows, c.d_qn,
                         ix->d_cnorms, nq, (int)ix->nlist, dpad,
                         cx->w_cdists.as<float>(), s);
        KCHECK("rank-gemm");
    } else {
        plan_rank_scan(c.nq, c.scan.rank.qt, ix->nlist, ix->cent_groups,
                       cx->rank_jobs);
        const ScanJobs jb = upload_scan_jobs(cx->rank_jobs, cx->w_jobs, s);
        HIP_CHECK(hipEventRecord(cx->ev[0], s));
        launch_scan(ix->kmetric, c.scan.rank, ix->d_cent_packed, c.d_q,
                    c.d_qn, dpad, jb, cx->w_cdists.as<float>(), s);
        KCHECK("rank-scan");
    }
    HIP_CHECK(hipEventRecord(cx->ev[1], s));
    cx->w_csel_slots.ensure((size_t)c.nq * c.probe * 4);
    cx->w_csel_dists.ensure((size_t)c.nq * c.probe * 4);
    launch_topk(cx->w_cdists.as<float>(), nullptr, ix->nlist, nq,
                (int)c.probe, cx->w_csel_slots.as<int32_t>(),
                cx->w_csel_dists.as<float>(), s);
    KCHECK("rank-topk");
}

/* 3. D2H the probe selection — the pipeline's one host sync — and plan the
 * list scan (findCentroids -> scanEntries shape, search.go:917-1005) */
void fetch_probe_and_plan(IvfIndex* ix, SearchCtx* cx) {
    const SearchCtx::Call& c = cx->call;
    const hipStream_t s = cx->stream;
    cx->h_probe.resize((size_t)c.nq * c.probe);
    HIP_CHECK(hipMemcpyAsync(cx->h_probe.data(), cx->w_csel_slots.ptr,
                             cx->h_probe.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    plan_probe_offsets(cx->h_probe.data(), c.nq, c.probe, ix->list_rows,
                       cx->offs);
    plan_list_scan(cx->h_probe.data(), c.nq, c.probe, c.scan.list.qt,
                   list_chunk_groups(ix->qtype, scan_overrides()),
                   ix->list_rows, ix->list_gbase, ix->list_slot_base,
                   cx->offs, cx->lists);
}

/* 4. list scan into the ragged candidate buffer: prepare the queries the
 * way the variant's kernel reads them, then one launch. */
void scan_lists(IvfIndex* ix, SearchCtx* cx, const uint32_t* filter_words) {
    const SearchCtx::Call& c = cx->call;
    const int dpad = (int)ix->dpad, nq = (int)c.nq;
    const hipStream_t s = cx->stream;
    const ScanVariant v = c.scan.list;
    const uint32_t* d_filter = nullptr;
    if (filter_words) {
        const size_t fw = (size_t)((ix->count + 31) / 32);
        cx->h_filter.assign(filter_words, filter_words + fw);
        cx->w_filter.ensure(fw * 4);
        HIP_CHECK(hipMemcpyAsync(cx->w_filter.ptr, cx->h_filter.data(),
                                 fw * 4, hipMemcpyHostToDevice, s));
        d_filter = cx->w_filter.as<uint32_t>();
    }
    cx->w_cand.ensure(std::max<int64_t>(1, cx->offs.total_cand) * 4);
    float* d_cand = cx->w_cand.as<float>();
    const ScanJobs jb = upload_scan_jobs(cx->lists.jobs, cx->w_qslots, s);
    HIP_CHECK(hipEventRecord(cx->ev[2], s));
    switch (v.kind) {
    case ScanKind::BYTE_DOT:
    case ScanKind::BYTE_U4: {
        /* the byte image — the internal clip-quantized one for the refine
         * first pass, else the int8/uint8 storage — and the map that narrows
         * the queries like its entries (quantizer.go ApplyInt8/entry SQL) */
        const bool uns = !c.refine && ix->qtype == Quantization_UINT8;
        const uint8_t* image = c.refine ? ix->d_packed_rq : ix->d_packed_q;
        const ByteImageLayout layout =
            c.refine ? ix->rq_layout : ByteImageLayout::ROWS16;
        const int32_t* rownorms =
            c.refine ? ix->d_rownorm_rq : ix->d_rownorm_q;
        const double mul = c.refine ? ix->rq_mul : ix->quant_mul;
        const double add = c.refine ? ix->rq_add : ix->quant_add;
        cx->w_queries_q.ensure((size_t)c.nq * dpad);
        uint8_t* d_qq = cx->w_queries_q.as<uint8_t>();
        launch_quantize_rows(uns, c.d_q, (int64_t)c.nq, dpad, (int)ix->dim,
                             dpad, (float)mul, (float)add, d_qq, s);
        KCHECK("query-quantize");
        const int32_t* d_qni = nullptr;
        if (ix->kmetric == KM_COS || ix->kmetric == KM_L2SQ) {
            /* cos denominators; also qn of the dot-form L2 */
            cx->w_qnorms_i.ensure(c.nq * 4);
            launch_qnorms_i8(uns, d_qq, nq, dpad,
                             cx->w_qnorms_i.as<int32_t>(), s);
            d_qni = cx->w_qnorms_i.as<int32_t>();
        }
        launch_scan_i8(ix->kmetric, v, uns, layout, image, d_qq, d_qni,
                       rownorms, dpad, jb, d_cand, s, d_filter);
        break;
    }
    case ScanKind::HALF: {
        /* plain-cast narrow search: query cast RTNE like the entries
         * (relation_search.go:56-63), decoded-f32 distance */
        const bool bf = ix->qtype == Quantization_BF16;
        cx->w_queries_q.ensure((size_t)c.nq * dpad * 2);
        uint16_t* d_qh = cx->w_queries_q.as<uint16_t>();
        launch_quantize_half_rows(bf, c.d_q, (int64_t)c.nq, dpad,
                                  (int)ix->dim, dpad, d_qh, s);
        KCHECK("query-half-cast");
        const float* d_qnh = nullptr;
        if (ix->kmetric == KM_COS) {
            cx->w_qnorms_i.ensure(c.nq * 4);
            launch_qnorms_h(bf, d_qh, nq, dpad, cx->w_qnorms_i.as<float>(),
                            s);
            d_qnh = cx->w_qnorms_i.as<float>();
        }
        launch_scan_h(ix->kmetric, v, bf, (const uint16_t*)ix->d_packed_q,
                      d_qh, d_qnh, dpad, jb, d_cand, s, d_filter);
        break;
    }
    case ScanKind::F32:
    case ScanKind::F32_ASM768:
        launch_scan(ix->kmetric, v, ix->d_packed, c.d_q, c.d_qn, dpad, jb,
                    d_cand, s, d_filter);
        break;
    }
    KCHECK("list-scan");
    HIP_CHECK(hipEventRecord(cx->ev[3], s));
}

/* 5. per-query top-limit over the candidates; for the two-stage scan: top-R
 * by byte distance -> exact f32 re-rank -> top-limit -> candidate slots */
int score_sqrt(const IvfIndex* ix) {
    return ix->metric == DistanceType_L2SqrtExpanded;
}
double score_inv_mul2(const IvfIndex* ix) {
    return (ix->quant_mul != 0.0 && ix->quant_mul != 1.0)
               ? 1.0 / (ix->quant_mul * ix->quant_mul) : 1.0;
}

void select_candidates(IvfIndex* ix, SearchCtx* cx) {
    SearchCtx::Call& c = cx->call;
    const int dpad = (int)ix->dpad, nq = (int)c.nq, limit = (int)c.limit;
    const hipStream_t s = cx->stream;
    upload_vector(cx->w_qoffs, cx->offs.qoffs, s);
    upload_vector(cx->w_probe_lists, cx->h_probe, s);
    upload_vector(cx->w_probe_offs, cx->offs.probe_offs, s);
    cx->w_sel_slots.ensure((size_t)c.nq * limit * 4);
    cx->w_sel_dists.ensure((size_t)c.nq * limit * 4);
    const bool legacy = ix->refine_tail_legacy;
    if (!legacy && !ix->d_select_stats) {
        HIP_CHECK(hipMalloc(&ix->d_select_stats, 16));
        HIP_CHECK(hipMemset(ix->d_select_stats, 0, 16)); /* once */
    }
    /* the ragged selection: one read against a sampled threshold, or the
     * radix select under the legacy switch */
    const auto select_ragged = [&](int k, int32_t* slots, float* dists) {
        if (legacy)
            launch_topk(cx->w_cand.as<float>(), cx->w_qoffs.as<int64_t>(), 0,
                        nq, k, slots, dists, s);
        else
            launch_select(cx->w_cand.as<float>(), cx->w_qoffs.as<int64_t>(),
                          nq, k, slots, dists, ix->d_select_stats, s);
    };
    c.outputs_written = false;
    HIP_CHECK(hipEventRecord(cx->ev[4], s));
    if (c.refine) {
        const int R = std::max<int>(limit, ix->refine_depth);
        cx->w_rsel_slots.ensure((size_t)c.nq * R * 4);
        cx->w_rsel_dists.ensure((size_t)c.nq * R * 4);
        select_ragged(R, cx->w_rsel_slots.as<int32_t>(),
                      cx->w_rsel_dists.as<float>());
        KCHECK("refine-topR");
        if (!legacy && refine_finish_applies(R, dpad)) {
            /* exact re-rank, top-limit, ids and score transform in one
             * kernel: gather_results only copies */
            const size_t n = (size_t)c.nq * limit;
            cx->w_out_ids.ensure(n * 8);
            cx->w_out_dists.ensure(n * 4);
            launch_refine_finish(
                ix->kmetric, ix->d_rows_f32, c.d_q, c.d_qn, (int)ix->dim,
                dpad, R, nq, cx->w_rsel_slots.as<int32_t>(),
                cx->w_rsel_dists.as<float>(),
                cx->w_probe_lists.as<int32_t>(),
                cx->w_probe_offs.as<int64_t>(), ix->d_list_slot_base,
                ix->d_id_by_slot, (int)c.probe, limit, score_sqrt(ix),
                score_inv_mul2(ix), cx->w_out_ids.as<int64_t>(),
                cx->w_out_dists.as<float>(), s);
            KCHECK("refine-finish");
            c.outputs_written = true;
            HIP_CHECK(hipEventRecord(cx->ev[5], s));
            return;
        }
        cx->w_refined.ensure((size_t)c.nq * R * 4);
        launch_refine(ix->kmetric, ix->d_rows_f32, c.d_q, c.d_qn,
                      (int)ix->dim, dpad, R, nq,
                      cx->w_rsel_slots.as<int32_t>(),
                      cx->w_rsel_dists.as<float>(),
                      cx->w_probe_lists.as<int32_t>(),
                      cx->w_probe_offs.as<int64_t>(), ix->d_list_slot_base,
                      (int)c.probe, cx->w_refined.as<float>(), s);
        KCHECK("refine");
        cx->w_sel2.ensure((size_t)c.nq * limit * 4);
        launch_topk(cx->w_refined.as<float>(), nullptr, R, nq, limit,
                    cx->w_sel2.as<int32_t>(), cx->w_sel_dists.as<float>(), s);
        KCHECK("refine-topk");
        launch_compose_select(cx->w_sel2.as<int32_t>(),
                              cx->w_rsel_slots.as<int32_t>(), R, limit, nq,
                              cx->w_sel_slots.as<int32_t>(), s);
        KCHECK("refine-compose");
    } else {
        select_ragged(limit, cx->w_sel_slots.as<int32_t>(),
                      cx->w_sel_dists.as<float>());
        KCHECK("cand-topk");
    }
    HIP_CHECK(hipEventRecord(cx->ev[5], s));
}

/* 6. id gather + score transform (unless the fused refine tail has written
 * them), then D2H through the ctx's pinned bounce (pageable-async degrades
 * to a host-blocking copy on ROCm, which would serialize the pipeline) */
void gather_results(IvfIndex* ix, SearchCtx* cx) {
    const SearchCtx::Call& c = cx->call;
    const size_t n = (size_t)c.nq * c.limit;
    const hipStream_t s = cx->stream;
    if (!c.outputs_written) {
        cx->w_out_ids.ensure(n * 8);
        cx->w_out_dists.ensure(n * 4);
        launch_gather(cx->w_sel_slots.as<int32_t>(),
                      cx->w_sel_dists.as<float>(),
                      cx->w_probe_lists.as<int32_t>(),
                      cx->w_probe_offs.as<int64_t>(), ix->d_list_slot_base,
                      ix->d_id_by_slot, (int)c.probe, (int)c.nq, (int)c.limit,
                      score_sqrt(ix), score_inv_mul2(ix),
                      cx->w_out_ids.as<int64_t>(),
                      cx->w_out_dists.as<float>(), s);
        KCHECK("gather");
    }
    cx->ensure_hout(n * 12);
    int64_t* ho_ids = (int64_t*)cx->h_out;
    float* ho_dists = (float*)(ho_ids + n);
    HIP_CHECK(hipMemcpyAsync(ho_ids, cx->w_out_ids.ptr, n * 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ho_dists, cx->w_out_dists.ptr, n * 4,
                             hipMemcpyDeviceToHost, s));
}

std::unique_ptr<Result> run_search(IvfIndex* ix, const float* queries,
                                   bool queries_on_device, uint64_t nq,
                                   uint32_t limit, uint32_t n_probes,
                                   const uint32_t* filter_words = nullptr,
                                   bool sync_end = true) {
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_CHECK(hipSetDevice(ix->device));
    SearchCtx* cx = &ix->sctx[ix->sparity++ & 1];
    cx->ensure(ix);
    if (cx->pending) collect_result(cx->pending); /* FIFO reuse guard */
    auto res = std::make_unique<Result>();
    res->neighbors.assign((size_t)nq * limit, -1);
    res->distances.assign((size_t)nq * limit, FLT_MAX);
    if (nq == 0) return res;
    if (!ix->built) throw std::runtime_error("index not built");
    if (ix->count == 0) return res;
    if (limit > 4096) throw std::runtime_error("limit > 4096 unsupported");
    const uint32_t probe =
        std::min<uint32_t>(n_probes ? n_probes : 1, ix->nlist);
    if (probe > 4096) throw std::runtime_error("n_probes > 4096 unsupported");
    ix->perf.ensure();

    SearchCtx::Call& c = cx->call;
    c.nq = nq;
    c.limit = limit;
    c.probe = probe;
    c.refine = ix->qtype == Quantization_F32 && ix->refine_depth > 0 &&
               ix->d_packed_rq != nullptr;
    /* the one scan decision: job tables are planned at, and launchers
     * switch on, these variants (moann_scan_plan.h) */
    c.scan = pick_scan(ix->kmetric, (int)ix->dpad, ix->qtype, c.refine,
                       (c.refine ? ix->d_rownorm_rq : ix->d_rownorm_q) !=
                           nullptr,
                       scan_overrides());

    const auto t_all0 = std::chrono::steady_clock::now();
    stage_queries(ix, cx, queries, queries_on_device);
    rank_centroids(ix, cx);
    fetch_probe_and_plan(ix, cx);
    scan_lists(ix, cx, filter_words);
    select_candidates(ix, cx);
    gather_results(ix, cx);

    /* host-known perf counters (kernel window times land at collect) */
    ix->perf.c.rank_launches++;
    ix->perf.c.rank_flops += 2ull * nq * ix->nlist * ix->dim;
    uint64_t unique_rows = 0;
    for (uint32_t l = 0; l < ix->nlist; ++l)
        if (cx->lists.lcount[l]) unique_rows += (uint64_t)ix->list_rows[l];
    ix->perf.c.scan_launches++;
    ix->perf.c.scan_bytes += unique_rows * ix->dim * 4;
    ix->perf.c.scan_rows += (uint64_t)cx->offs.total_cand;

    res->owner = cx;
    res->collected = false;
    HIP_CHECK(hipEventCreate(&res->done_ev));
    HIP_CHECK(hipEventRecord(res->done_ev, cx->stream));
    cx->pending = res.get();
    /* submit-side wall: under pipelining this is the NON-overlapped host
     * cost (H2D, probe sync, job build); kernel windows come from cx->ev */
    const double kms = sync_end ? collect_result(res.get()) : 0.0;
    const double wall = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - t_all0).count();
    ix->perf.c.other_ms += wall - kms;
    return res;
}

/* Wait for a submitted search, copy the pinned payload into the result
 * vectors and fold the kernel event windows into the perf counters.
 * Serialized by the submit/wait discipline (the submit path collects a
 * ctx's pending result before reusing it). */
/* Top-k merge of an extend tail's (collected) result into the main result.
 * Both rows are ordered by closeness (cpu_topk_merge_sharded semantics,
 * cgo/cuvs/helper.h:137-167): ascending distance, except post-flip IP where
 * the C-ABI value is +a.b and closeness is DESCENDING value. Pads (-1,
 * FLT_MAX) sort last. */
void merge_tail_into(MoannResult* res) {
    if (!res->tail_res || res->tail_merged) return;
    MoannResult* t = res->tail_res.get();
    const size_t total = res->neighbors.size();
    if (t->neighbors.size() != total || total == 0) { res->tail_merged = true; return; }
    /* limit is carried implicitly: both results are [nq][limit]; recover
     * nq from the merge caller's perspective via the stored stride */
    const uint32_t limit = res->merge_limit;
    const size_t nq = limit ? total / limit : 0;
    const bool ip = res->merge_kmetric == KM_IP;
    auto closer = [&](float a, float b) { return ip ? a > b : a < b; };
    std::vector<int64_t> mi(limit);
    std::vector<float> md(limit);
    for (size_t q = 0; q < nq; ++q) {
        const int64_t* an = res->neighbors.data() + q * limit;
        const float* ad = res->distances.data() + q * limit;
        const int64_t* bn = t->neighbors.data() + q * limit;
        const float* bd = t->distances.data() + q * limit;
        uint32_t i = 0, j = 0, o = 0;
        while (o < limit) {
            const bool av = i < limit && an[i] != -1;
            const bool bv = j < limit && bn[j] != -1;
            if (!av && !bv) break;
            if (av && (!bv || closer(ad[i], bd[j]) ||
                       (ad[i] == bd[j] && true /* main-first tie order,
                           matching helper.h's stable shard order */))) {
                mi[o] = an[i]; md[o] = ad[i]; ++i;
            } else {
                mi[o] = bn[j]; md[o] = bd[j]; ++j;
            }
            ++o;
        }
        for (; o < limit; ++o) { mi[o] = -1; md[o] = FLT_MAX; }
        memcpy(res->neighbors.data() + q * limit, mi.data(), limit * 8);
        memcpy(res->distances.data() + q * limit, md.data(), limit * 4);
    }
    res->tail_merged = true;
    res->tail_res.reset();
}

double collect_result(MoannResult* res) {
    if (res->collected) return 0.0;
    auto cx = (SearchCtx*)res->owner;
    auto ix = (IvfIndex*)cx->parent;
    HIP_CHECK(hipEventSynchronize(res->done_ev));
    HIP_CHECK(hipGetLastError());
    const size_t n = res->neighbors.size();
    const int64_t* ho_ids = (const int64_t*)cx->h_out;
    const float* ho_dists = (const float*)(ho_ids + n);
    memcpy(res->neighbors.data(), ho_ids, n * 8);
    memcpy(res->distances.data(), ho_dists, n * 4);
    /* Reference C-ABI contract (cgo/cuvs/index_base.hpp:355-375
     * transform_distance): InnerProduct distances cross the C ABI as the
     * TRUE +a.b (the internal/MO-convention -a.b is flipped at readout;
     * ±FLT_MAX pad/filter sentinels preserved). The host mirror negates
     * back to MO's -a.b convention, matching the reference's division of
     * labor between cgo and Go. */
    if (ix->kmetric == KM_IP) {
        float* d = res->distances.data();
        for (size_t i = 0; i < n; ++i)
            if (d[i] != FLT_MAX && d[i] != -FLT_MAX) d[i] = -d[i];
    }
    float r_ms = 0, sc_ms = 0, sel_ms = 0;
    (void)hipEventElapsedTime(&r_ms, cx->ev[0], cx->ev[1]);
    (void)hipEventElapsedTime(&sc_ms, cx->ev[2], cx->ev[3]);
    (void)hipEventElapsedTime(&sel_ms, cx->ev[4], cx->ev[5]);
    ix->perf.c.rank_ms += r_ms;
    ix->perf.c.scan_ms += sc_ms;
    ix->perf.c.select_ms += sel_ms;
    res->collected = true;
    if (cx->pending == res) cx->pending = nullptr;
    merge_tail_into(res);
    return (double)r_ms + sc_ms + sel_ms;
}

uint64_t total_len(IvfIndex* ix) {
    return ix->count + (ix->tail ? ix->tail->count : 0);
}

/* AND the caller's slot bitset (over [0, nbits) slots) with the alive
 * bitset of `ix` over its own slot range starting at `slot0` in the global
 * numbering; returns words covering ix->count bits (bit extraction handles
 * the unaligned tail region). nullptr user = all-pass. */
std::vector<uint32_t> combined_filter(IvfIndex* ix, uint64_t slot0,
                                      const uint32_t* user, uint64_t nbits) {
    const uint64_t n = ix->count;
    std::vector<uint32_t> out((size_t)((n + 31) / 32), ~0u);
    if (user) {
        if (slot0 % 32 == 0 && slot0 + n <= nbits) {
            /* word-aligned range (the main index at slot0 = 0): straight
             * word copy — no per-bit work on the 10M-slot hot path */
            memcpy(out.data(), user + slot0 / 32, out.size() * 4);
            if (n % 32) /* mask stray bits beyond count in the last word */
                out.back() |= ~((1u << (n % 32)) - 1u);
        } else {
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t g = slot0 + i;
                const bool bit =
                    g < nbits && ((user[g / 32] >> (g % 32)) & 1u);
                if (!bit) out[i / 32] &= ~(1u << (i % 32));
            }
        }
    }
    if (ix->deleted_count) {
        const size_t aw = ix->alive.size();
        for (size_t w = 0; w < out.size() && w < aw; ++w)
            out[w] &= ix->alive[w];
    }
    return out;
}

/* Search main + (if extends happened) the tail sub-index, with the soft-
 * delete bitset and any caller filter folded in; tail top-k is merged at
 * collect (or immediately for the synchronous path). This is the single
 * funnel every C search entry routes through. */
std::unique_ptr<Result> run_search_full(IvfIndex* ix, const float* queries,
                                        bool queries_on_device, uint64_t nq,
                                        uint32_t limit, uint32_t n_probes,
                                        const uint32_t* user_filter = nullptr,
                                        uint64_t user_nbits = 0,
                                        bool sync_end = true) {
    /* snapshot mutable host state under the index mutex: ix->tail and the
     * alive bitsets are written by extend/delete_id (which hold mu); the
     * shared_ptr copy keeps a replaced tail alive through this search */
    std::shared_ptr<IvfIndex> tl;
    std::vector<uint32_t> mf, tf;
    bool need_main_filter = false, need_tf = false;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        tl = ix->tail;
        need_main_filter = user_filter || ix->deleted_count > 0;
        if (need_main_filter)
            mf = combined_filter(ix, 0, user_filter, user_nbits);
        if (tl && tl->count > 0) {
            need_tf = user_filter || tl->deleted_count > 0;
            if (need_tf)
                tf = combined_filter(tl.get(), ix->count, user_filter,
                                     user_nbits);
        } else {
            tl.reset();
        }
    }

    /* tail first (synchronous, small), so the submit path can return after
     * enqueueing the main scan */
    std::unique_ptr<Result> tres;
    if (tl) {
        tres = run_search(tl.get(), queries, queries_on_device, nq, limit,
                          n_probes, need_tf ? tf.data() : nullptr,
                          /*sync_end=*/true);
    }
    auto res = run_search(ix, queries, queries_on_device, nq, limit, n_probes,
                          need_main_filter ? mf.data() : nullptr, sync_end);
    res->merge_kmetric = ix->kmetric;
    res->merge_limit = limit;
    if (tres) {
        res->tail_res = std::move(tres);
        if (res->collected) merge_tail_into(res.get());
    }
    return res;
}

void batcher_loop(IvfIndex* ix) {
    std::unique_lock<std::mutex> lk(ix->bmu);
    for (;;) {
        ix->bcv.wait(lk, [&] { return ix->batcher_stop || !ix->pending.empty(); });
        if (ix->batcher_stop) return;
        /* window: let more requests coalesce */
        const auto window =
            std::chrono::microseconds(ix->batch_window_us.load());
        ix->bcv.wait_for(lk, window, [&] { return ix->batcher_stop; });
        if (ix->batcher_stop) return;
        auto batch = std::move(ix->pending);
        ix->pending.clear();
        lk.unlock();
        /* group by (limit, nprobe); one fused search per group */
        using PReq = IvfIndex::PendingReq;
    std::map<std::pair<uint32_t, uint32_t>, std::vector<PReq*>> gs;
        for (auto& r : batch) gs[{r.limit, r.nprobe}].push_back(&r);
        for (auto& [key, reqs] : gs) {
            const auto [limit, nprobe] = key;
            uint64_t total = 0;
            for (auto* r : reqs) total += r->nq;
            std::vector<float> qcat((size_t)total * ix->dim);
            uint64_t off = 0;
            for (auto* r : reqs) {
                memcpy(qcat.data() + off * ix->dim, r->queries.data(),
                       r->queries.size() * 4);
                off += r->nq;
            }
            std::unique_ptr<Result> merged;
            std::string err;
            try {
                merged = run_search_full(ix, qcat.data(), false, total,
                                         limit, nprobe);
            } catch (const std::exception& e) {
                err = e.what();
            }
            std::lock_guard<std::mutex> g(ix->bmu);
            off = 0;
            for (auto* r : reqs) {
                auto part = std::make_unique<Result>();
                if (merged) {
                    part->neighbors.assign(
                        merged->neighbors.begin() + off * limit,
                        merged->neighbors.begin() + (off + r->nq) * limit);
                    part->distances.assign(
                        merged->distances.begin() + off * limit,
                        merged->distances.begin() + (off + r->nq) * limit);
                } /* on error: empty result — search_wait reports it */
                ix->done_jobs[r->job_id] = std::move(part);
                off += r->nq;
            }
        }
        lk.lock();
        ix->bdone_cv.notify_all();
    }
}

/* ------------------------- native k-means build -------------------------
 * gpu_ivf_flat_build fills h_centroids / h_assign itself when the caller
 * did not (DESIGN.md "Native k-means build"). The rules — sample, init,
 * reseed, stop — are moann_kmeans_plan.h; the kernels kmeans_kernels.hip. */

/* MOANN_KMEANS_ASSIGN=gemm, read once: assignment through the chunked
 * rank GEMM + top-1 select instead of the fused kernel (A/B + fallback). */
bool kmeans_assign_gemm() {
    static const bool v = [] {
        const char* e = getenv("MOANN_KMEANS_ASSIGN");
        return e && strcmp(e, "gemm") == 0;
    }();
    return v;
}

struct KmeansWork { /* workspaces of the gemm composition */
    DevBuf q, qn, dmat;
};

/* assign[i], best[i] for the n rows of the set `map` over d_staging */
void kmeans_assign(IvfIndex* ix, int metric, KmRowMap map, int64_t n,
                   const float* d_cents, const float* d_cnorms,
                   int32_t* d_assign, float* d_best, KmeansWork& w) {
    const int k = (int)ix->nlist, dim = (int)ix->dim, dpad = (int)ix->dpad;
    if (!kmeans_assign_gemm()) {
        launch_km_assign(metric, ix->d_staging, dim, map, n, d_cents,
                         d_cnorms, k, dim, dpad, d_assign, d_best, ix->stream);
        KCHECK("kmeans-assign");
        return;
    }
    /* the composition the tree could already do: padded row chunk ->
     * [chunk][k] distance matrix -> top-1. The matrix is bounded at 256 MiB
     * by chunking the rows. */
    int64_t chunk = std::max<int64_t>(
        32, ((int64_t)256 << 20) / ((int64_t)k * 4) / 32 * 32);
    chunk = std::min(chunk, n);
    w.q.ensure((size_t)chunk * dpad * 4);
    w.qn.ensure((size_t)chunk * 4);
    w.dmat.ensure((size_t)chunk * k * 4);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t cnt = std::min(chunk, n - i0);
        launch_km_gather_pad(ix->d_staging, dim, map, i0, cnt, dim, dpad,
                             w.q.as<float>(), ix->stream);
        launch_qnorms(w.q.as<float>(), (int)cnt, dpad, w.qn.as<float>(),
                      ix->stream);
        if (!launch_rank_gemm(metric, w.q.as<float>(), d_cents,
                              w.qn.as<float>(), d_cnorms, (int)cnt, k, dpad,
                              w.dmat.as<float>(), ix->stream))
            throw std::logic_error("kmeans: metric has no GEMM form");
        launch_topk(w.dmat.as<float>(), nullptr, k, (int)cnt, 1,
                    d_assign + i0, d_best + i0, ix->stream);
        KCHECK("kmeans-assign-gemm");
    }
}

void kmeans_check_range(const std::vector<int32_t>& a, uint32_t nlist) {
    for (int32_t v : a)
        if (v < 0 || (uint32_t)v >= nlist)
            throw std::runtime_error("kmeans: assignment out of range");
}

/* [nlist][dpad] zero-padded device centroids + |c|^2 */
void kmeans_cnorms(IvfIndex* ix, const float* d_cents, float* d_cnorms) {
    launch_km_row_sumsq(false, d_cents, ix->dpad, KmRowMap {1, 1},
                        ix->nlist, (int)ix->dpad, d_cnorms, ix->stream);
    KCHECK("kmeans-cnorms");
}

/* train h_centroids from the staged rows */
void kmeans_train(IvfIndex* ix) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = (int64_t)ix->count;
    const int k = (int)ix->nlist, dim = (int)ix->dim, dpad = (int)ix->dpad;
    const int64_t n_train =
        (int64_t)kmeans_n_train(ix->count, ix->nlist, ix->km_fraction,
                                ix->km_max_train);
    /* the kernels evaluate (i*n)/n_train in int64 (moann_kmeans_plan.h
     * uses 128 bits): far beyond any staging buffer, but checked */
    if ((unsigned __int128)n * (unsigned __int128)n_train >
        (unsigned __int128)INT64_MAX)
        throw std::runtime_error("kmeans: n * n_train exceeds 2^63");
    const KmRowMap map {n, n_train};
    /* L2, L2sqrt, L1 and IP indexes train under L2SQ; COS is spherical */
    const int tmetric = ix->kmetric == KM_COS ? KM_COS : KM_L2SQ;
    const hipStream_t s = ix->stream;

    DevBuf d_cents, d_cnorms, d_assign, d_best, d_inv, d_offs, d_members,
        d_cidx, d_trow;
    KmeansWork work;
    d_cents.ensure((size_t)k * dpad * 4);
    HIP_CHECK(hipMemsetAsync(d_cents.ptr, 0, (size_t)k * dpad * 4, s));
    d_cnorms.ensure((size_t)k * 4);
    d_assign.ensure((size_t)n_train * 4);
    d_best.ensure((size_t)n_train * 4);
    d_members.ensure((size_t)n_train * 4);

    std::vector<int32_t> cidx(k);
    std::vector<int64_t> trow(k);
    for (int j = 0; j < k; ++j) {
        cidx[j] = j;
        trow[j] = (int64_t)kmeans_init_row((uint32_t)j, (uint64_t)n_train,
                                           ix->nlist);
    }
    upload_vector(d_cidx, cidx, s);
    upload_vector(d_trow, trow, s);
    launch_km_set_centroids(ix->d_staging, dim, map, d_cidx.as<int32_t>(),
                            d_trow.as<int64_t>(), k, dim, dpad,
                            d_cents.as<float>(), s);
    KCHECK("kmeans-init");
    const float* d_invp = nullptr;
    if (tmetric == KM_COS) {
        d_inv.ensure((size_t)n_train * 4);
        launch_km_row_sumsq(true, ix->d_staging, dim, map, n_train, dim,
                            d_inv.as<float>(), s);
        KCHECK("kmeans-invnorm");
        d_invp = d_inv.as<float>();
    }
    HIP_CHECK(hipStreamSynchronize(s)); /* cidx/trow are reused below */

    std::vector<int32_t> h_a(n_train), prev, members(n_train);
    std::vector<float> h_best(n_train);
    std::vector<int64_t> offs(k + 1), cur(k);
    uint32_t it = 0;
    for (;; ++it) {
        kmeans_cnorms(ix, d_cents.as<float>(), d_cnorms.as<float>());
        kmeans_assign(ix, tmetric, map, n_train, d_cents.as<float>(),
                      d_cnorms.as<float>(), d_assign.as<int32_t>(),
                      d_best.as<float>(), work);
        HIP_CHECK(hipMemcpyAsync(h_a.data(), d_assign.ptr,
                                 (size_t)n_train * 4, hipMemcpyDeviceToHost,
                                 s));
        HIP_CHECK(hipMemcpyAsync(h_best.data(), d_best.ptr,
                                 (size_t)n_train * 4, hipMemcpyDeviceToHost,
                                 s));
        HIP_CHECK(hipStreamSynchronize(s));
        kmeans_check_range(h_a, ix->nlist);

        /* CSR: rows grouped by centroid, ascending row inside a group */
        std::fill(offs.begin(), offs.end(), 0);
        for (int32_t a : h_a) offs[a + 1]++;
        for (int c = 0; c < k; ++c) offs[c + 1] += offs[c];
        std::copy(offs.begin(), offs.end() - 1, cur.begin());
        for (int64_t i = 0; i < n_train; ++i)
            members[cur[h_a[i]]++] = (int32_t)i;
        upload_vector(d_offs, offs, s);
        HIP_CHECK(hipMemcpyAsync(d_members.ptr, members.data(),
                                 (size_t)n_train * 4, hipMemcpyHostToDevice,
                                 s));
        launch_km_update(ix->d_staging, dim, map, d_offs.as<int64_t>(),
                         d_members.as<int32_t>(), d_invp, k, dim, dpad,
                         d_cents.as<float>(), s);
        KCHECK("kmeans-update");

        /* empty centroids, ascending, take the farthest training rows */
        cidx.clear();
        for (int c = 0; c < k; ++c)
            if (offs[c + 1] == offs[c]) cidx.push_back(c);
        const uint64_t n_empty = cidx.size();
        if (n_empty) {
            trow = kmeans_pick_reseeds(h_best.data(), (uint64_t)n_train,
                                       n_empty);
            upload_vector(d_cidx, cidx, s);
            upload_vector(d_trow, trow, s);
            launch_km_set_centroids(ix->d_staging, dim, map,
                                    d_cidx.as<int32_t>(),
                                    d_trow.as<int64_t>(), (int)n_empty, dim,
                                    dpad, d_cents.as<float>(), s);
            KCHECK("kmeans-reseed");
        }
        HIP_CHECK(hipStreamSynchronize(s));
        const bool same = it > 0 && h_a == prev;
        if (kmeans_should_stop(it, ix->km_iters, same, n_empty)) break;
        prev = h_a;
    }
    ix->h_centroids.resize((size_t)k * dim);
    HIP_CHECK(hipMemcpy2D(ix->h_centroids.data(), (size_t)dim * 4,
                          d_cents.ptr, (size_t)dpad * 4, (size_t)dim * 4, k,
                          hipMemcpyDeviceToHost));
    ix->km_iters_run = it + 1;
    ix->km_n_train = (uint64_t)n_train;
    ix->km_train_ms = std::chrono::duration<double, std::milli>(
                          std::chrono::steady_clock::now() - t0)
                          .count();
}

/* h_assign: every staged row to its nearest centroid under the index metric
 * (the gpu_ivf_flat_extend rule) */
void kmeans_assign_all(IvfIndex* ix) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = (int64_t)ix->count;
    const int k = (int)ix->nlist, dim = (int)ix->dim, dpad = (int)ix->dpad;
    ix->h_assign.assign((size_t)n, 0);
    if (n && ix->kmetric == KM_L1) {
        /* no MFMA form: the exact path extend uses, in bounded chunks */
        const int64_t chunk = 65536;
        std::vector<float> rows((size_t)std::min(chunk, n) * dim);
        std::vector<int64_t> nearest(std::min(chunk, n));
        std::vector<float> ndist(std::min(chunk, n));
        for (int64_t i0 = 0; i0 < n; i0 += chunk) {
            const int64_t cnt = std::min(chunk, n - i0);
            HIP_CHECK(hipMemcpy(rows.data(), ix->d_staging + i0 * dim,
                                (size_t)cnt * dim * 4,
                                hipMemcpyDeviceToHost));
            char* inner = nullptr;
            moann_brute_force_search(ix->h_centroids.data(), ix->nlist,
                                     ix->dim, ix->metric, nullptr,
                                     rows.data(), (uint64_t)cnt, 1,
                                     ix->device, nearest.data(),
                                     ndist.data(), &inner);
            if (inner) {
                std::string m = std::string("kmeans assign: ") + inner;
                free(inner);
                throw std::runtime_error(m);
            }
            HIP_CHECK(hipSetDevice(ix->device));
            for (int64_t i = 0; i < cnt; ++i)
                ix->h_assign[i0 + i] = (int32_t)nearest[i];
        }
    } else if (n) {
        DevBuf d_cents, d_cnorms, d_assign, d_best;
        KmeansWork work;
        d_cents.ensure((size_t)k * dpad * 4);
        HIP_CHECK(hipMemset(d_cents.ptr, 0, (size_t)k * dpad * 4));
        HIP_CHECK(hipMemcpy2D(d_cents.ptr, (size_t)dpad * 4,
                              ix->h_centroids.data(), (size_t)dim * 4,
                              (size_t)dim * 4, k, hipMemcpyHostToDevice));
        d_cnorms.ensure((size_t)k * 4);
        d_assign.ensure((size_t)n * 4);
        d_best.ensure((size_t)n * 4);
        kmeans_cnorms(ix, d_cents.as<float>(), d_cnorms.as<float>());
        kmeans_assign(ix, ix->kmetric, KmRowMap {1, 1}, n,
                      d_cents.as<float>(), d_cnorms.as<float>(),
                      d_assign.as<int32_t>(), d_best.as<float>(), work);
        HIP_CHECK(hipMemcpyAsync(ix->h_assign.data(), d_assign.ptr,
                                 (size_t)n * 4, hipMemcpyDeviceToHost,
                                 ix->stream));
        HIP_CHECK(hipStreamSynchronize(ix->stream));
    }
    kmeans_check_range(ix->h_assign, ix->nlist);
    ix->km_assign_ms = std::chrono::duration<double, std::milli>(
                           std::chrono::steady_clock::now() - t0)
                           .count();
}

IvfIndex* IX(gpu_ivf_flat_c h) { return (IvfIndex*)h; }

}  // namespace

/* ============================== C ABI ==================================== */

extern "C" {

gpu_ivf_flat_c gpu_ivf_flat_new_empty(uint64_t total_count, uint32_t dimension,
                                      distance_type_t metric,
                                      ivf_flat_build_params_t build_params,
                                      const int* devices, int device_count,
                                      uint32_t /*nthread*/,
                                      distribution_mode_t /*dist_mode*/,
                                      quantization_t btype, quantization_t qtype,
                                      const int64_t* /*ids*/, void* errmsg) {
    try {
        /* wired btype/qtype combos mirror ivf_flat_c.h:33-35 */
        const bool ok_f32_base =
            btype == Quantization_F32 &&
            (qtype == Quantization_F32 || qtype == Quantization_INT8 ||
             qtype == Quantization_UINT8 || qtype == Quantization_F16 ||
             qtype == Quantization_BF16);
        const bool ok_f16_base =
            btype == Quantization_F16 &&
            (qtype == Quantization_F16 || qtype == Quantization_INT8 ||
             qtype == Quantization_UINT8);
        if (!ok_f32_base && !ok_f16_base)
            throw std::runtime_error(
                "wired combos (ivf_flat_c.h:33-35): F32 base "
                "{F32,F16,BF16,INT8,UINT8}; F16 base {F16,INT8,UINT8}");
        auto ix = std::make_unique<IvfIndex>();
        ix->btype = btype;
        ix->device = (devices && device_count > 0) ? devices[0] : 0;
        HIP_CHECK(hipSetDevice(ix->device));
        HIP_CHECK(hipStreamCreate(&ix->stream));
        ix->dim = dimension;
        /* halves stream 8 elements (16 B) per lane step -> pad to 8 */
        ix->dpad = (qtype == Quantization_F16 || qtype == Quantization_BF16)
                       ? ((dimension + 7) & ~7u)
                       : ((dimension + 3) & ~3u);
        ix->metric = metric;
        ix->kmetric = metric_kind(metric);
        ix->nlist = build_params.n_lists ? build_params.n_lists : 1024;
        ix->km_fraction =
            kmeans_fraction(build_params.kmeans_trainset_fraction);
        ix->qtype = qtype;
        ix->cap = total_count;
        ix->h_ids.reserve(total_count);
        if (total_count)
            HIP_CHECK(hipMalloc(&ix->d_staging,
                                (size_t)total_count * dimension * 4));
        return (gpu_ivf_flat_c)ix.release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_new_empty", e.what());
        return nullptr;
    }
}

/* common staging path: f32 rows into d_staging (quantized at build) */
void stage_rows_f32(IvfIndex* ix, const float* rows, uint64_t chunk_count,
                    const int64_t* ids) {
    if (ix->built) throw std::runtime_error("index already built");
    if (ix->count + chunk_count > ix->cap)
        throw std::runtime_error("chunk exceeds capacity");
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipMemcpyAsync(ix->d_staging + ix->count * ix->dim, rows,
                             chunk_count * ix->dim * 4,
                             hipMemcpyHostToDevice, ix->stream));
    HIP_CHECK(hipStreamSynchronize(ix->stream));
    for (uint64_t i = 0; i < chunk_count; ++i)
        ix->h_ids.push_back(ids ? ids[i] : (int64_t)(ix->count + i));
    ix->count += chunk_count;
}

/* ivf_flat_c.h:69: chunk in the STORAGE type T (widened losslessly to the
 * f32 staging; build re-narrows to the identical codes). */
void gpu_ivf_flat_add_chunk(gpu_ivf_flat_c h, const void* chunk_data,
                            uint64_t chunk_count, const int64_t* ids,
                            void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->qtype == Quantization_F32) {
            stage_rows_f32(ix, (const float*)chunk_data, chunk_count, ids);
        } else {
            std::vector<float> conv((size_t)chunk_count * ix->dim);
            storage_to_f32(ix->qtype, chunk_data, conv.size(), ix->quant_mul,
                           ix->quant_add, conv.data());
            stage_rows_f32(ix, conv.data(), chunk_count, ids);
        }
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_add_chunk", e.what());
    }
}

/* ivf_flat_c.h:80: f32 chunk, narrowed to storage at build */
void gpu_ivf_flat_add_chunk_float(gpu_ivf_flat_c h, const float* chunk_data,
                                  uint64_t chunk_count, const int64_t* ids,
                                  void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        stage_rows_f32(ix, chunk_data, chunk_count, ids);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_add_chunk_float", e.what());
    }
}

/* ivf_flat_c.h:83: chunk in the BASE type B */
void gpu_ivf_flat_add_chunk_quantize(gpu_ivf_flat_c h, const void* base_data,
                                     uint64_t chunk_count,
                                     const int64_t* ids, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->btype == Quantization_F32) {
            stage_rows_f32(ix, (const float*)base_data, chunk_count, ids);
        } else {
            auto conv = base_to_f32(ix->btype, base_data,
                                    (size_t)chunk_count * ix->dim);
            stage_rows_f32(ix, conv.data(), chunk_count, ids);
        }
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_add_chunk_quantize", e.what());
    }
}

void moann_ivf_flat_set_centroids(gpu_ivf_flat_c h, const float* centroids,
                                  uint32_t n_lists, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        /* number of centroids must match nlist (ivfflat/search.go:146) */
        if (n_lists != ix->nlist)
            throw std::runtime_error("number of centroids != n_lists");
        ix->h_centroids.assign(centroids,
                               centroids + (size_t)n_lists * ix->dim);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_set_centroids", e.what());
    }
}

void moann_ivf_flat_set_assignments(gpu_ivf_flat_c h,
                                    const int32_t* assignments, uint64_t count,
                                    void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (count != ix->count)
            throw std::runtime_error("assignment count != vector count");
        for (uint64_t i = 0; i < count; ++i)
            if (assignments[i] < 0 || (uint32_t)assignments[i] >= ix->nlist)
                throw std::runtime_error("assignment out of range");
        ix->h_assign.assign(assignments, assignments + count);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_set_assignments", e.what());
    }
}

void gpu_ivf_flat_build(gpu_ivf_flat_c h, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->built) return;
        HIP_CHECK(hipSetDevice(ix->device));
        /* three cases (include/moann.h): neither array set -> train, then
         * assign; centroids only (LoadCentroids) -> assign; both -> as given */
        if (ix->h_centroids.empty() && !ix->h_assign.empty())
            throw std::runtime_error(
                "assignments set without centroids: set both, the centroids "
                "alone, or neither");
        if (ix->h_centroids.empty()) kmeans_train(ix);
        if (ix->h_assign.empty() && ix->count) kmeans_assign_all(ix);
        if (ix->h_assign.size() != ix->count)
            throw std::runtime_error(
                "no assignments: call moann_ivf_flat_set_assignments");
        HIP_CHECK(hipSetDevice(ix->device));

        /* CSR by list, stable insertion order (matches the entries-table scan
         * order and the oracle's np.argsort(kind='stable')) */
        std::vector<int64_t> loffsets(ix->nlist + 1, 0);
        for (auto a : ix->h_assign) loffsets[a + 1]++;
        for (uint32_t l = 0; l < ix->nlist; ++l) loffsets[l + 1] += loffsets[l];
        std::vector<int64_t> slot_rows(ix->count);
        {
            std::vector<int64_t> cur(loffsets.begin(), loffsets.end() - 1);
            for (uint64_t i = 0; i < ix->count; ++i)
                slot_rows[cur[ix->h_assign[i]]++] = (int64_t)i;
        }
        ix->list_slot_base.assign(loffsets.begin(), loffsets.end() - 1);
        ix->list_rows.resize(ix->nlist);
        for (uint32_t l = 0; l < ix->nlist; ++l)
            ix->list_rows[l] = (int32_t)(loffsets[l + 1] - loffsets[l]);

        /* pack entries */
        pack_lists(ix, ix->d_staging, ix->count, slot_rows, loffsets,
                   &ix->d_packed, &ix->list_gbase, &ix->total_groups);
        /* group -> slot metadata kept for save_dir's unpack */
        ix->group_slotbase.resize(ix->total_groups);
        ix->group_valid.resize(ix->total_groups);
        for (uint32_t l = 0; l < ix->nlist; ++l)
            for (int64_t g = ix->list_gbase[l]; g < ix->list_gbase[l + 1]; ++g) {
                const int64_t gi = g - ix->list_gbase[l];
                ix->group_slotbase[g] = loffsets[l] + gi * 64;
                ix->group_valid[g] = (int32_t)std::min<int64_t>(
                    64, (loffsets[l + 1] - loffsets[l]) - gi * 64);
            }
        if (ix->qtype != Quantization_F32) {
            /* quantize the staged rows (pad columns emit 0 so padded dims
             * stay identity), byte-pack, and drop the f32 copy — storage
             * stays narrow (search.go:1062 quantized domain). f16/bf16 are
             * MO's PLAIN-CAST narrowing (quantizer.go:50-58): u16 elements,
             * no affine scaling. */
            const bool uns = ix->qtype == Quantization_UINT8;
            const bool half = ix->qtype == Quantization_F16 ||
                              ix->qtype == Quantization_BF16;
            const size_t eb = half ? 2 : 1;
            DevBuf d_qrows, d_rb2, d_gv2, d_sr2;
            d_qrows.ensure((size_t)ix->count * ix->dpad * eb);
            if (half)
                launch_quantize_half_rows(
                    ix->qtype == Quantization_BF16, ix->d_staging,
                    (int64_t)ix->count, (int)ix->dim, (int)ix->dim,
                    (int)ix->dpad, d_qrows.as<uint16_t>(), ix->stream);
            else
                launch_quantize_rows(uns, ix->d_staging, (int64_t)ix->count,
                                     (int)ix->dim, (int)ix->dim,
                                     (int)ix->dpad, (float)ix->quant_mul,
                                     (float)ix->quant_add,
                                     d_qrows.as<uint8_t>(), ix->stream);
            KCHECK("quantize-rows");
            d_rb2.ensure(ix->total_groups * 8);
            d_gv2.ensure(ix->total_groups * 4);
            d_sr2.ensure(std::max<size_t>(8, slot_rows.size() * 8));
            HIP_CHECK(hipMemcpyAsync(d_rb2.ptr, ix->group_slotbase.data(),
                                     ix->total_groups * 8,
                                     hipMemcpyHostToDevice, ix->stream));
            HIP_CHECK(hipMemcpyAsync(d_gv2.ptr, ix->group_valid.data(),
                                     ix->total_groups * 4,
                                     hipMemcpyHostToDevice, ix->stream));
            /* pack wants slot->row; group_slotbase already holds the slot
             * base per group, slot_rows maps slot->row */
            if (!slot_rows.empty())
                HIP_CHECK(hipMemcpyAsync(d_sr2.ptr, slot_rows.data(),
                                         slot_rows.size() * 8,
                                         hipMemcpyHostToDevice, ix->stream));
            if (ix->d_rownorm_q) {
                (void)hipFree(ix->d_rownorm_q);
                ix->d_rownorm_q = nullptr;
            }
            HIP_CHECK(hipMalloc(&ix->d_packed_q,
                                (size_t)ix->total_groups * 64 * ix->dpad *
                                    eb));
            const int bpad = (int)(ix->dpad * eb); /* row bytes */
            if ((bpad & 15) == 0)
                /* 16-byte-unit layout for the dwordx4 scans */
                launch_bytes_pack16(d_qrows.as<uint8_t>(), bpad,
                                    d_rb2.as<int64_t>(), d_gv2.as<int32_t>(),
                                    d_sr2.as<int64_t>(), ix->total_groups,
                                    ix->d_packed_q, ix->stream);
            else
                launch_pq_pack(d_qrows.as<uint8_t>(), bpad,
                               d_rb2.as<int64_t>(), d_gv2.as<int32_t>(),
                               d_sr2.as<int64_t>(), ix->total_groups,
                               ix->d_packed_q, ix->stream);
            if (!half && (ix->dpad & 15) == 0) {
                /* row norms for the dot-form byte scan (rn + qn - 2*dot) */
                HIP_CHECK(hipMalloc(&ix->d_rownorm_q,
                                    (size_t)ix->total_groups * 64 * 4));
                launch_rownorms_i8(ix->qtype == Quantization_UINT8,
                                   ByteImageLayout::ROWS16, ix->d_packed_q,
                                   ix->total_groups,
                                   (int)ix->dpad, ix->d_rownorm_q,
                                   ix->stream);
            }
            HIP_CHECK(hipStreamSynchronize(ix->stream));
            KCHECK("quantize-pack");
            HIP_CHECK(hipFree(ix->d_packed));
            ix->d_packed = nullptr;
        }


        /* id map: slot -> entry id */
        std::vector<int64_t> id_by_slot(std::max<uint64_t>(1, ix->count));
        for (uint64_t sslot = 0; sslot < ix->count; ++sslot)
            id_by_slot[sslot] = ix->h_ids[slot_rows[sslot]];
        HIP_CHECK(hipMalloc(&ix->d_id_by_slot, id_by_slot.size() * 8));
        HIP_CHECK(hipMemcpy(ix->d_id_by_slot, id_by_slot.data(),
                            id_by_slot.size() * 8, hipMemcpyHostToDevice));
        ix->h_id_by_slot = std::move(id_by_slot);
        ix->h_slot_rows = slot_rows;
        HIP_CHECK(hipMalloc(&ix->d_list_slot_base, ix->nlist * 8));
        HIP_CHECK(hipMemcpy(ix->d_list_slot_base, ix->list_slot_base.data(),
                            ix->nlist * 8, hipMemcpyHostToDevice));

        /* pack the centroid matrix as one list of nlist rows */
        {
            DevBuf d_cent;
            d_cent.ensure((size_t)ix->nlist * ix->dim * 4);
            HIP_CHECK(hipMemcpy(d_cent.ptr, ix->h_centroids.data(),
                                (size_t)ix->nlist * ix->dim * 4,
                                hipMemcpyHostToDevice));
            std::vector<int64_t> cl = {0, (int64_t)ix->nlist};
            std::vector<int64_t> csr(ix->nlist);
            std::iota(csr.begin(), csr.end(), 0);
            std::vector<int64_t> cgb;
            pack_lists(ix, d_cent.as<float>(), ix->nlist, csr, cl,
                       &ix->d_cent_packed, &cgb, &ix->cent_groups);
        }

        /* MFMA rank operands: row-major zero-padded centroid matrix +
         * host-computed |c|^2 */
        {
            HIP_CHECK(hipMalloc(&ix->d_cent_rows,
                                (size_t)ix->nlist * ix->dpad * 4));
            if (ix->dim != ix->dpad)
                HIP_CHECK(hipMemset(ix->d_cent_rows, 0,
                                    (size_t)ix->nlist * ix->dpad * 4));
            HIP_CHECK(hipMemcpy2D(ix->d_cent_rows, (size_t)ix->dpad * 4,
                                  ix->h_centroids.data(), (size_t)ix->dim * 4,
                                  (size_t)ix->dim * 4, ix->nlist,
                                  hipMemcpyHostToDevice));
            std::vector<float> cn(ix->nlist);
            for (uint32_t c = 0; c < ix->nlist; ++c) {
                float ssum = 0.f;
                const float* row = ix->h_centroids.data() + (size_t)c * ix->dim;
                for (uint32_t e = 0; e < ix->dim; ++e) ssum += row[e] * row[e];
                cn[c] = ssum;
            }
            HIP_CHECK(hipMalloc(&ix->d_cnorms, ix->nlist * 4));
            HIP_CHECK(hipMemcpy(ix->d_cnorms, cn.data(), ix->nlist * 4,
                                hipMemcpyHostToDevice));
        }
        if (const char* e = getenv("MOANN_RANK"))
            ix->rank_mfma = std::string(e) == "mfma";

        /* drop staging */
        HIP_CHECK(hipFree(ix->d_staging));
        ix->d_staging = nullptr;
        ix->h_assign.clear();
        ix->h_assign.shrink_to_fit();
        ix->built = true;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_build", e.what());
    }
}

void gpu_ivf_flat_start(gpu_ivf_flat_c h, void* errmsg) {
    try {
        IX(h)->started = true;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_start", e.what());
    }
}

void gpu_ivf_flat_destroy(gpu_ivf_flat_c h, void* errmsg) {
    try {
        delete IX(h);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_destroy", e.what());
    }
}

/* ivf_flat_c.h:114-116: queries in the STORAGE type T (the reference's
 * search<T> signature); narrow input is widened host-side and re-narrowed
 * by the internal pipeline — an exact round trip, so results equal a
 * native byte-domain scan of the caller's codes. */
gpu_ivf_flat_search_res_t gpu_ivf_flat_search(gpu_ivf_flat_c h,
                                              const void* queries_data,
                                              uint64_t num_queries,
                                              uint32_t query_dimension,
                                              uint32_t limit,
                                              ivf_flat_search_params_t sp,
                                              void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        const float* q = (const float*)queries_data;
        std::vector<float> conv;
        if (ix->qtype != Quantization_F32) {
            conv.resize((size_t)num_queries * ix->dim);
            storage_to_f32(ix->qtype, queries_data, conv.size(),
                           ix->quant_mul, ix->quant_add, conv.data());
            q = conv.data();
        }
        out.result_ptr = run_search_full(ix, q, false, num_queries, limit,
                                         sp.n_probes)
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search", e.what());
    }
    return out;
}

/* ivf_flat_c.h:119-122: queries in the BASE type B. */
gpu_ivf_flat_search_res_t gpu_ivf_flat_search_quantize(
    gpu_ivf_flat_c h, const void* queries_data, uint64_t num_queries,
    uint32_t query_dimension, uint32_t limit, ivf_flat_search_params_t sp,
    void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        const float* q = (const float*)queries_data;
        std::vector<float> conv;
        if (ix->btype != Quantization_F32) {
            conv = base_to_f32(ix->btype, queries_data,
                               (size_t)num_queries * ix->dim);
            q = conv.data();
        }
        out.result_ptr = run_search_full(ix, q, false, num_queries, limit,
                                         sp.n_probes)
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_quantize", e.what());
    }
    return out;
}

gpu_ivf_flat_search_res_t moann_ivf_flat_search_device(gpu_ivf_flat_c h,
                                                       const void* queries_dev,
                                                       uint64_t num_queries,
                                                       uint32_t query_dimension,
                                                       uint32_t limit,
                                                       ivf_flat_search_params_t sp,
                                                       void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        out.result_ptr = run_search_full(ix, (const float*)queries_dev, true,
                                         num_queries, limit, sp.n_probes)
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_search_device", e.what());
    }
    return out;
}

/* Pipelined submit: phase 1 (query H2D, centroid rank, probe top-k, probe
 * D2H) and the host job build run NOW on one of two per-index pipeline
 * contexts; the list scan / select / gather / result D2H are ENQUEUED on
 * that context's stream and the call returns without waiting. Collect with
 * moann_ivf_flat_result_wait (or any get_*); at most two submits in
 * flight, collected FIFO — a third submit collects the oldest itself. */
gpu_ivf_flat_search_res_t moann_ivf_flat_search_submit(
    gpu_ivf_flat_c h, const void* queries, int queries_on_device,
    uint64_t num_queries, uint32_t query_dimension, uint32_t limit,
    ivf_flat_search_params_t sp, void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        out.result_ptr = run_search_full(ix, (const float*)queries,
                                         queries_on_device != 0, num_queries,
                                         limit, sp.n_probes, nullptr, 0,
                                         /*sync_end=*/false)
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_search_submit", e.what());
    }
    return out;
}

int moann_ivf_flat_result_wait(gpu_ivf_flat_result_c r, void* errmsg) {
    try {
        collect_result((Result*)r);
        return 0;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_result_wait", e.what());
        return -1;
    }
}

static uint64_t async_f32_impl(IvfIndex* ix, const float* queries_f32,
                               uint64_t num_queries, uint32_t limit,
                               ivf_flat_search_params_t sp) {
    {
        const void* queries_data = queries_f32;
        if (ix->batch_window_us.load() > 0) {
            /* dynamic batching: enqueue and let the batcher fuse requests
             * arriving within the window into one device search */
            std::lock_guard<std::mutex> lk(ix->bmu);
            if (!ix->batcher_started) {
                ix->batcher = std::thread(batcher_loop, ix);
                ix->batcher_started = true;
            }
            IvfIndex::PendingReq r;
            r.queries.assign((const float*)queries_data,
                             (const float*)queries_data +
                                 num_queries * ix->dim);
            r.nq = num_queries;
            r.limit = limit;
            r.nprobe = sp.n_probes;
            std::lock_guard<std::mutex> lk2(ix->mu);
            r.job_id = ix->next_job++;
            const uint64_t id = r.job_id;
            ix->pending.push_back(std::move(r));
            ix->bcv.notify_one();
            return id;
        }
        auto res = run_search_full(ix, (const float*)queries_data, false,
                                   num_queries, limit, sp.n_probes);
        std::lock_guard<std::mutex> lk(ix->mu);
        const uint64_t id = ix->next_job++;
        ix->jobs[id] = std::move(res);
        return id;
    }
}

uint64_t gpu_ivf_flat_search_async(gpu_ivf_flat_c h, const void* queries_data,
                                   uint64_t num_queries,
                                   uint32_t query_dimension, uint32_t limit,
                                   ivf_flat_search_params_t sp, void* errmsg) {
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        /* storage-typed queries like gpu_ivf_flat_search */
        std::vector<float> conv;
        const float* q = (const float*)queries_data;
        if (ix->qtype != Quantization_F32) {
            conv.resize((size_t)num_queries * ix->dim);
            storage_to_f32(ix->qtype, queries_data, conv.size(),
                           ix->quant_mul, ix->quant_add, conv.data());
            q = conv.data();
        }
        return async_f32_impl(ix, q, num_queries, limit, sp);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_async", e.what());
        return 0;
    }
}

/* ivf_flat_c.h:130-133: async pair in the BASE type B (the entry behind
 * pkg/cuvs/ivf_flat.go:772 SearchQuantizeAsync — call stack C). */
uint64_t gpu_ivf_flat_search_quantize_async(gpu_ivf_flat_c h,
                                            const void* queries_data,
                                            uint64_t num_queries,
                                            uint32_t query_dimension,
                                            uint32_t limit,
                                            ivf_flat_search_params_t sp,
                                            void* errmsg) {
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        const float* q = (const float*)queries_data;
        std::vector<float> conv;
        if (ix->btype != Quantization_F32) {
            conv = base_to_f32(ix->btype, queries_data,
                               (size_t)num_queries * ix->dim);
            q = conv.data();
        }
        return async_f32_impl(ix, q, num_queries, limit, sp);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_quantize_async", e.what());
        return 0;
    }
}

gpu_ivf_flat_search_res_t gpu_ivf_flat_search_wait(gpu_ivf_flat_c h,
                                                   uint64_t job_id,
                                                   void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        {
            std::lock_guard<std::mutex> lk(ix->mu);
            auto it = ix->jobs.find(job_id);
            if (it != ix->jobs.end()) {
                out.result_ptr = it->second.release();
                ix->jobs.erase(it);
                return out;
            }
        }
        /* batched job: block until the batcher publishes it */
        std::unique_lock<std::mutex> lk(ix->bmu);
        if (!ix->bdone_cv.wait_for(lk, std::chrono::seconds(120), [&] {
                return ix->done_jobs.count(job_id) != 0;
            }))
            throw std::runtime_error("timed out waiting for batched job");
        auto it = ix->done_jobs.find(job_id);
        auto res = std::move(it->second);
        ix->done_jobs.erase(it);
        if (res->neighbors.empty() && res->distances.empty())
            throw std::runtime_error("batched search failed");
        out.result_ptr = res.release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_wait", e.what());
    }
    return out;
}

void gpu_ivf_flat_get_neighbors(gpu_ivf_flat_result_c r, uint64_t n,
                                int64_t* neighbors) {
    auto res = (Result*)r;
    if (!res->collected) collect_result(res);
    const uint64_t m = std::min<uint64_t>(n, res->neighbors.size());
    memcpy(neighbors, res->neighbors.data(), m * 8);
}

void gpu_ivf_flat_get_distances(gpu_ivf_flat_result_c r, uint64_t n,
                                float* distances) {
    auto res = (Result*)r;
    if (!res->collected) collect_result(res);
    const uint64_t m = std::min<uint64_t>(n, res->distances.size());
    memcpy(distances, res->distances.data(), m * 4);
}

void gpu_ivf_flat_free_result(gpu_ivf_flat_result_c r) {
    auto res = (Result*)r;
    if (res && res->done_ev) {
        if (!res->collected) {
            (void)hipEventSynchronize(res->done_ev);
            auto cx = (SearchCtx*)res->owner;
            if (cx && cx->pending == res) cx->pending = nullptr;
        }
        (void)hipEventDestroy(res->done_ev);
    }
    delete res;
}

/* SQL residual-predicate filter -> slot bitset (the cuVS
 * eval_filter_bitmap_cpu shape, filter.hpp:855-960). col_data/col_nulls are
 * the caller's columnar arrays in ADD (row) order; the result is permuted
 * to GLOBAL SLOT order for moann_ivf_flat_search_filtered. */
int moann_ivf_flat_filter_from_preds(gpu_ivf_flat_c h, const char* cols_json,
                                     const char* preds_json,
                                     const void* const* col_data,
                                     const uint32_t* const* col_nulls,
                                     uint32_t* out_words, void* errmsg) {
    try {
        auto ix = IX(h);
        if (!ix->built) throw std::runtime_error("index not built");
        const uint64_t n = ix->count;
        std::vector<uint32_t> row_bits((n + 31) / 32, 0);
        /* host ids in ADD (row) order for the virtual PK column */
        std::vector<int64_t> ids_by_row(n);
        for (uint64_t s2 = 0; s2 < n; ++s2)
            ids_by_row[ix->h_slot_rows[s2]] = ix->h_id_by_slot[s2];
        const int rc = moann_preds_eval(cols_json, preds_json, col_data,
                                        col_nulls, ids_by_row.data(), n,
                                        row_bits.data(), errmsg);
        if (rc != 0) return rc;
        std::memset(out_words, 0, ((n + 31) / 32) * 4);
        for (uint64_t s2 = 0; s2 < n; ++s2) {
            const uint64_t row = (uint64_t)ix->h_slot_rows[s2];
            if ((row_bits[row >> 5] >> (row & 31)) & 1u)
                out_words[s2 >> 5] |= 1u << (s2 & 31);
        }
        return 0;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_filter_from_preds", e.what());
        return -1;
    }
}

int moann_ivf_flat_filter_from_docfilter(gpu_ivf_flat_c h, int kind,
                                         const void* payload,
                                         uint64_t payload_len,
                                         uint32_t* out_words, void* errmsg) {
    try {
        auto ix = IX(h);
        if (!ix->built) throw std::runtime_error("index not built");
        return moann_docfilter_eval(kind, payload, payload_len,
                                    ix->h_id_by_slot.data(), ix->count,
                                    out_words, errmsg);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_filter_from_docfilter", e.what());
        return -1;
    }
}

uint64_t gpu_ivf_flat_cap(gpu_ivf_flat_c h) { return IX(h)->cap; }
uint64_t gpu_ivf_flat_len(gpu_ivf_flat_c h) { return total_len(IX(h)); }
uint32_t gpu_ivf_flat_get_n_list(gpu_ivf_flat_c h) { return IX(h)->nlist; }

void gpu_ivf_flat_get_centers(gpu_ivf_flat_c h, void* centers, void* errmsg) {
    try {
        auto ix = IX(h);
        if (ix->h_centroids.empty())
            throw std::runtime_error("no centroids set");
        memcpy(centers, ix->h_centroids.data(),
               ix->h_centroids.size() * sizeof(float));
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_get_centers", e.what());
    }
}

void moann_ivf_flat_set_kmeans_params(gpu_ivf_flat_c h, uint32_t n_iters,
                                      uint64_t max_train_rows, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->built)
            throw std::runtime_error("index already built");
        ix->km_iters = n_iters;
        ix->km_max_train = max_train_rows;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_set_kmeans_params", e.what());
    }
}

void moann_ivf_flat_get_assignments(gpu_ivf_flat_c h, int32_t* out,
                                    void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built) throw std::runtime_error("index not built");
        if (ix->h_slot_rows.size() != ix->count)
            throw std::runtime_error(
                "add-order rows are not kept for a loaded index");
        /* h_assign is dropped at build: slot -> list from the slot bases,
         * slot -> add-order row from h_slot_rows */
        for (uint32_t l = 0; l < ix->nlist; ++l) {
            const int64_t b = ix->list_slot_base[l];
            for (int64_t sl = b; sl < b + ix->list_rows[l]; ++sl)
                out[ix->h_slot_rows[sl]] = (int32_t)l;
        }
        for (size_t i = 0; i < ix->tail_assign.size(); ++i)
            out[ix->count + i] = ix->tail_assign[i];
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_get_assignments", e.what());
    }
}

void moann_ivf_flat_kmeans_stats(gpu_ivf_flat_c h, double* train_ms,
                                 double* assign_ms, uint32_t* iters,
                                 uint64_t* n_train, void* errmsg) {
    try {
        auto ix = IX(h);
        if (!ix) throw std::runtime_error("null index");
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built) throw std::runtime_error("index not built");
        if (train_ms) *train_ms = ix->km_train_ms;
        if (assign_ms) *assign_ms = ix->km_assign_ms;
        if (iters) *iters = ix->km_iters_run;
        if (n_train) *n_train = ix->km_n_train;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_kmeans_stats", e.what());
    }
}

void moann_ivf_flat_select_stats(gpu_ivf_flat_c h, uint64_t* filtered,
                                 uint64_t* fallback, void* errmsg) {
    try {
        auto ix = IX(h);
        if (!ix) throw std::runtime_error("null index");
        std::lock_guard<std::mutex> lk(ix->mu);
        /* the main lists and the tail of extended rows, whose searches count
         * into the tail index's own counter */
        unsigned long long sum[2] = {0, 0};
        for (IvfIndex* part : {ix, ix->tail.get()}) {
            if (!part || !part->d_select_stats) continue;
            unsigned long long st[2];
            HIP_CHECK(hipSetDevice(part->device));
            /* a blocking copy: every search submitted so far has counted */
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(st, part->d_select_stats, sizeof st,
                                hipMemcpyDeviceToHost));
            sum[0] += st[0];
            sum[1] += st[1];
        }
        if (filtered) *filtered = sum[0];
        if (fallback) *fallback = sum[1];
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_select_stats", e.what());
    }
}

void moann_ivf_flat_set_refine_tail(gpu_ivf_flat_c h, int legacy,
                                    void* errmsg) {
    try {
        auto ix = IX(h);
        if (!ix) throw std::runtime_error("null index");
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->refine_tail_legacy = legacy != 0;
        if (ix->tail) ix->tail->refine_tail_legacy = legacy != 0;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_set_refine_tail", e.what());
    }
}

void moann_select_plan(int64_t count, int32_t k, int32_t* filter,
                       int32_t* sample, int32_t* rank, int32_t* capacity,
                       int64_t* min_count, int32_t* kmax) {
    const SelectPlan p = select_plan(count, k);
    if (filter) *filter = p.filter;
    if (sample) *sample = p.m;
    if (rank) *rank = p.t;
    if (capacity) *capacity = SELECT_CAPACITY;
    if (min_count) *min_count = SELECT_MIN_COUNT;
    if (kmax) *kmax = SELECT_KMAX;
}

void moann_select_sample_positions(int64_t count, int32_t k, int64_t* out) {
    const SelectPlan p = select_plan(count, k);
    for (int i = 0; p.filter && i < p.m; ++i)
        out[i] = select_sample_pos(count, p.m, i);
}

void moann_select_topk(const float* dists, const int64_t* qoffs, int64_t nq,
                       int32_t k, int32_t mode, int32_t* out_slots,
                       float* out_dists, uint64_t* fallbacks, double* kernel_ms,
                       void* errmsg) {
    try {
        if (nq < 0 || nq > INT32_MAX || k < 1 || k > 4096 ||
            (mode != 0 && mode != 1))
            throw std::runtime_error("bad nq, k or mode");
        if (fallbacks) *fallbacks = 0;
        if (kernel_ms) *kernel_ms = 0.0;
        if (nq == 0) return;
        for (int64_t q = 0; q < nq; ++q)
            if (qoffs[q] < 0 || qoffs[q + 1] < qoffs[q] ||
                qoffs[q + 1] - qoffs[q] > UINT32_MAX)
                throw std::runtime_error("qoffs must ascend from >= 0");
        const size_t total = (size_t)qoffs[nq], no = (size_t)nq * k;
        DevBuf d_d, d_o, d_s, d_od, d_st;
        d_d.ensure(std::max<size_t>(1, total) * 4);
        d_o.ensure((size_t)(nq + 1) * 8);
        d_s.ensure(no * 4);
        d_od.ensure(no * 4);
        d_st.ensure(16);
        HIP_CHECK(hipMemcpy(d_d.ptr, dists, total * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_o.ptr, qoffs, (size_t)(nq + 1) * 8,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_st.ptr, 0, 16));
        struct Events { /* destroyed on every way out */
            hipEvent_t e[2] = {nullptr, nullptr};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) (void)hipEventDestroy(x);
            }
        } ev;
        HIP_CHECK(hipEventCreate(&ev.e[0]));
        HIP_CHECK(hipEventCreate(&ev.e[1]));
        HIP_CHECK(hipEventRecord(ev.e[0], nullptr));
        if (mode == 1)
            launch_select(d_d.as<float>(), d_o.as<int64_t>(), (int)nq, k,
                          d_s.as<int32_t>(), d_od.as<float>(),
                          d_st.as<unsigned long long>(), nullptr);
        else
            launch_topk(d_d.as<float>(), d_o.as<int64_t>(), 0, (int)nq, k,
                        d_s.as<int32_t>(), d_od.as<float>(), nullptr);
        HIP_CHECK(hipEventRecord(ev.e[1], nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        KCHECK("select-topk");
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        unsigned long long st[2];
        HIP_CHECK(hipMemcpy(out_slots, d_s.ptr, no * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_dists, d_od.ptr, no * 4,
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(st, d_st.ptr, 16, hipMemcpyDeviceToHost));
        if (fallbacks) *fallbacks = st[1];
        if (kernel_ms) *kernel_ms = ms;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_select_topk", e.what());
    }
}

void moann_brute_force_search(const float* dataset, uint64_t count,
                              uint32_t dimension, distance_type_t metric,
                              const int64_t* ids, const float* queries,
                              uint64_t num_queries, uint32_t limit, int device,
                              int64_t* out_neighbors, float* out_distances,
                              void* errmsg) {
    /* exact search = one-list IVF with probe 1 */
    char* inner = nullptr;
    try {
        ivf_flat_build_params_t bp {1, true, 0.5};
        gpu_ivf_flat_c h = gpu_ivf_flat_new_empty(
            count, dimension, metric, bp, &device, 1, 0,
            DistributionMode_SINGLE_GPU, Quantization_F32, Quantization_F32,
            nullptr, &inner);
        if (!h) throw std::runtime_error(inner ? inner : "new failed");
        gpu_ivf_flat_add_chunk(h, dataset, count, ids, &inner);
        std::vector<float> cent(dimension, 0.f);
        moann_ivf_flat_set_centroids(h, cent.data(), 1, &inner);
        std::vector<int32_t> assign(count, 0);
        moann_ivf_flat_set_assignments(h, assign.data(), count, &inner);
        gpu_ivf_flat_build(h, &inner);
        if (inner) throw std::runtime_error(inner);
        ivf_flat_search_params_t sp {1};
        auto r = gpu_ivf_flat_search(h, queries, num_queries, dimension, limit,
                                     sp, &inner);
        if (!r.result_ptr) throw std::runtime_error(inner ? inner : "search failed");
        gpu_ivf_flat_get_neighbors(r.result_ptr, num_queries * limit,
                                   out_neighbors);
        gpu_ivf_flat_get_distances(r.result_ptr, num_queries * limit,
                                   out_distances);
        /* moann_* entries speak MO conventions (IP = -a.b,
         * distance_func.go:174-207); the cuVS-named readout above emits the
         * reference C-ABI contract (+a.b) — negate back, skip sentinels. */
        if (metric == DistanceType_InnerProduct)
            for (uint64_t i = 0; i < num_queries * (uint64_t)limit; ++i)
                if (out_distances[i] != FLT_MAX && out_distances[i] != -FLT_MAX)
                    out_distances[i] = -out_distances[i];
        gpu_ivf_flat_free_result(r.result_ptr);
        gpu_ivf_flat_destroy(h, nullptr);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_brute_force_search", e.what());
    }
    if (inner) free(inner);
}

/* Membership-filtered search: slot_bitset has one bit per
 * stored entry in SLOT order (moann_ivf_flat_slots_of_ids maps ids); a
 * cleared bit excludes the entry before top-k, mirroring the cuVS device
 * bitset filter (cgo/cuvs/ivf_flat.hpp:908-924) that backs MO's docfilter
 * membership kinds on the GPU path. */
gpu_ivf_flat_search_res_t moann_ivf_flat_search_filtered(
    gpu_ivf_flat_c h, const void* queries_data, uint64_t num_queries,
    uint32_t query_dimension, uint32_t limit, ivf_flat_search_params_t sp,
    const uint32_t* slot_bitset, uint64_t nbits, void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        if (nbits < total_len(ix))
            throw std::runtime_error("filter bitset smaller than index");
        out.result_ptr = run_search_full(ix, (const float*)queries_data,
                                         false, num_queries, limit,
                                         sp.n_probes, slot_bitset, nbits)
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_search_filtered", e.what());
    }
    return out;
}

/* id -> global slot lookup for building filter bitsets host-side.
 * out_slots[i] = -1 for unknown ids. */
void moann_ivf_flat_slots_of_ids(gpu_ivf_flat_c h, const int64_t* ids,
                                 uint64_t n, int64_t* out_slots,
                                 void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built) throw std::runtime_error("index not built");
        if (ix->id_to_slot.empty() && ix->count) {
            ix->id_to_slot.reserve(ix->count * 2);
            for (uint64_t sidx = 0; sidx < ix->count; ++sidx)
                ix->id_to_slot.emplace(ix->h_id_by_slot[sidx], (int64_t)sidx);
        }
        IvfIndex* t = ix->tail.get();
        if (t && t->count && t->id_to_slot.empty()) { /* lazy tail map */
            t->id_to_slot.reserve(t->count * 2);
            for (uint64_t sidx = 0; sidx < t->count; ++sidx)
                t->id_to_slot.emplace(t->h_id_by_slot[sidx], (int64_t)sidx);
        }
        for (uint64_t i = 0; i < n; ++i) {
            auto it = ix->id_to_slot.find(ids[i]);
            if (it != ix->id_to_slot.end()) {
                out_slots[i] = it->second;
                continue;
            }
            out_slots[i] = -1;
            if (t && t->count) {
                auto jt = t->id_to_slot.find(ids[i]);
                if (jt != t->id_to_slot.end())
                    /* tail slots follow the main slots in the global
                     * numbering (gpu_ivf_flat_extend) */
                    out_slots[i] = (int64_t)ix->count + jt->second;
            }
        }
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_slots_of_ids", e.what());
    }
}

/* ---- dataset ctor (ivf_flat_c.h:41-45) ---------------------------------- */

gpu_ivf_flat_c gpu_ivf_flat_new(const void* dataset_data,
                                uint64_t count_vectors, uint32_t dimension,
                                distance_type_t metric,
                                ivf_flat_build_params_t build_params,
                                const int* devices, int device_count,
                                uint32_t nthread,
                                distribution_mode_t dist_mode,
                                quantization_t btype, quantization_t qtype,
                                const int64_t* ids, void* errmsg) {
    char* inner = nullptr;
    gpu_ivf_flat_c h = gpu_ivf_flat_new_empty(
        count_vectors, dimension, metric, build_params, devices,
        device_count, nthread, dist_mode, btype, qtype, ids, &inner);
    if (!h) {
        set_errmsg(errmsg, "gpu_ivf_flat_new", inner ? inner : "new failed");
        if (inner) free(inner);
        return nullptr;
    }
    if (count_vectors)
        gpu_ivf_flat_add_chunk(h, dataset_data, count_vectors, ids, &inner);
    if (inner) {
        set_errmsg(errmsg, "gpu_ivf_flat_new", inner);
        free(inner);
        gpu_ivf_flat_destroy(h, nullptr);
        return nullptr;
    }
    return h;
}

/* ---- extend (ivf_flat_c.h:71-78) ---------------------------------------- */

/* rebuild the tail sub-index from the accumulated extend staging (O(tail)
 * per extend call; cheap while the tail is small relative to the corpus) */
static void rebuild_tail(IvfIndex* ix) {
    char* inner = nullptr;
    auto chk = [&](const char* what) {
        if (inner) {
            std::string m = std::string(what) + ": " + inner;
            free(inner);
            inner = nullptr;
            throw std::runtime_error(m);
        }
    };
    const uint64_t n = ix->tail_ids.size();
    ivf_flat_build_params_t bp {ix->nlist, true, 1.0};
    int dev = ix->device;
    gpu_ivf_flat_c th = gpu_ivf_flat_new_empty(
        n, ix->dim, ix->metric, bp, &dev, 1, 0,
        DistributionMode_SINGLE_GPU, ix->btype, ix->qtype, nullptr, &inner);
    chk("tail new_empty");
    if (!th) throw std::runtime_error("tail new_empty failed");
    std::unique_ptr<IvfIndex> tix((IvfIndex*)th);
    if (ix->qtype == Quantization_INT8 || ix->qtype == Quantization_UINT8) {
        gpu_ivf_flat_set_quantizer(th, (float)ix->quant_min,
                                   (float)ix->quant_max, &inner);
        chk("tail set_quantizer");
    }
    gpu_ivf_flat_add_chunk_float(th, ix->tail_staging.data(), n,
                                 ix->tail_ids.data(), &inner);
    chk("tail add_chunk");
    moann_ivf_flat_set_centroids(th, ix->h_centroids.data(), ix->nlist,
                                 &inner);
    chk("tail set_centroids");
    moann_ivf_flat_set_assignments(th, ix->tail_assign.data(), n, &inner);
    chk("tail set_assignments");
    gpu_ivf_flat_build(th, &inner);
    chk("tail build");
    tix->refine_tail_legacy = ix->refine_tail_legacy;
    ix->tail = std::move(tix);
    /* re-apply soft deletes that target tail rows */
    for (int64_t id : ix->tail_deleted) {
        IvfIndex* t = ix->tail.get();
        if (t->id_to_slot.empty() && t->count) {
            t->id_to_slot.reserve(t->count * 2);
            for (uint64_t s2 = 0; s2 < t->count; ++s2)
                t->id_to_slot.emplace(t->h_id_by_slot[s2], (int64_t)s2);
        }
        auto it = t->id_to_slot.find(id);
        if (it == t->id_to_slot.end()) continue;
        const uint64_t pos = (uint64_t)it->second;
        const uint64_t nw = (t->count + 31) / 32;
        if (t->alive.size() < nw) t->alive.resize(nw, ~0u);
        if ((t->alive[pos / 32] >> (pos % 32)) & 1u) {
            t->alive[pos / 32] &= ~(1u << (pos % 32));
            ++t->deleted_count;
        }
    }
}

void gpu_ivf_flat_extend_float(gpu_ivf_flat_c h, const float* new_data,
                               uint64_t n_rows, const int64_t* new_ids,
                               void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built)
            throw std::runtime_error("extend: index not built"); /* the
                reference throws too (index_base.hpp:2156) */
        if (n_rows == 0) return;
        /* assign to the nearest centroid under the index metric (the
         * cuvs::ivf_flat::extend rule) via the one-shot brute force */
        std::vector<int64_t> nearest(n_rows);
        std::vector<float> ndist(n_rows);
        char* inner = nullptr;
        moann_brute_force_search(ix->h_centroids.data(), ix->nlist, ix->dim,
                                 ix->metric, nullptr, new_data, n_rows, 1,
                                 ix->device, nearest.data(), ndist.data(),
                                 &inner);
        if (inner) {
            std::string m = std::string("extend assign: ") + inner;
            free(inner);
            throw std::runtime_error(m);
        }
        const uint64_t base = total_len(ix);
        ix->tail_staging.insert(ix->tail_staging.end(), new_data,
                                new_data + n_rows * ix->dim);
        for (uint64_t i = 0; i < n_rows; ++i) {
            ix->tail_ids.push_back(new_ids ? new_ids[i]
                                           : (int64_t)(base + i));
            ix->tail_assign.push_back((int32_t)nearest[i]);
        }
        rebuild_tail(ix);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_extend_float", e.what());
    }
}

void gpu_ivf_flat_extend(gpu_ivf_flat_c h, const void* new_data,
                         uint64_t n_rows, const int64_t* new_ids,
                         void* errmsg) {
    try {
        auto ix = IX(h);
        if (ix->qtype == Quantization_F32) {
            gpu_ivf_flat_extend_float(h, (const float*)new_data, n_rows,
                                      new_ids, errmsg);
            return;
        }
        std::vector<float> conv((size_t)n_rows * ix->dim);
        storage_to_f32(ix->qtype, new_data, conv.size(), ix->quant_mul,
                       ix->quant_add, conv.data());
        gpu_ivf_flat_extend_float(h, conv.data(), n_rows, new_ids, errmsg);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_extend", e.what());
    }
}

/* ---- soft delete (ivf_flat_c.h:102; index_base.hpp:1142-1167) ----------- */

void gpu_ivf_flat_delete_id(gpu_ivf_flat_c h, int64_t id, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built) throw std::runtime_error("delete_id: index not built");
        if (ix->id_to_slot.empty() && ix->count) {
            ix->id_to_slot.reserve(ix->count * 2);
            for (uint64_t sidx = 0; sidx < ix->count; ++sidx)
                ix->id_to_slot.emplace(ix->h_id_by_slot[sidx],
                                       (int64_t)sidx);
        }
        auto it = ix->id_to_slot.find(id);
        if (it != ix->id_to_slot.end()) {
            const uint64_t pos = (uint64_t)it->second;
            const uint64_t nw = (ix->count + 31) / 32;
            if (ix->alive.size() < nw) ix->alive.resize(nw, ~0u);
            if ((ix->alive[pos / 32] >> (pos % 32)) & 1u) {
                ix->alive[pos / 32] &= ~(1u << (pos % 32));
                ++ix->deleted_count;
            }
            return;
        }
        IvfIndex* t = ix->tail.get();
        if (t && t->count) {
            if (t->id_to_slot.empty()) {
                t->id_to_slot.reserve(t->count * 2);
                for (uint64_t s2 = 0; s2 < t->count; ++s2)
                    t->id_to_slot.emplace(t->h_id_by_slot[s2], (int64_t)s2);
            }
            auto jt = t->id_to_slot.find(id);
            if (jt != t->id_to_slot.end()) {
                const uint64_t pos = (uint64_t)jt->second;
                const uint64_t nw = (t->count + 31) / 32;
                if (t->alive.size() < nw) t->alive.resize(nw, ~0u);
                if ((t->alive[pos / 32] >> (pos % 32)) & 1u) {
                    t->alive[pos / 32] &= ~(1u << (pos % 32));
                    ++t->deleted_count;
                    ix->tail_deleted.push_back(id);
                }
                return;
            }
        }
        /* unknown id: silent no-op (index_base.hpp:1147) */
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_delete_id", e.what());
    }
}

/* ---- quantizer training (ivf_flat_c.h:86) ------------------------------- */

void gpu_ivf_flat_train_quantizer(gpu_ivf_flat_c h, const float* train_data,
                                  uint64_t n_samples, void* errmsg) {
    try {
        auto ix = IX(h);
        if (ix->qtype != Quantization_INT8 &&
            ix->qtype != Quantization_UINT8)
            throw std::runtime_error(
                "storage has no affine quantizer (int8/uint8 only)");
        if (n_samples == 0) throw std::runtime_error("empty training set");
        /* central-99% quantile range, the cuVS scalar-quantizer default
         * the reference trains with (quantize.hpp:60-66, cuvs
         * sq_params.quantile = 0.99); the affine map behind
         * set_quantizer keeps quantizer.go's formulas (the CPU-path
         * parity anchor). Bounded sample for large trainsets. */
        size_t n = (size_t)n_samples * ix->dim;
        size_t stride = 1;
        const size_t cap = 1u << 26;
        if (n > cap) stride = (n + cap - 1) / cap;
        /* avoid column-aliased sampling of the row-major buffer: keep the
         * stride coprime with small dim factors (dims are 2^a*3^b-ish) */
        if (stride > 1) {
            stride |= 1;
            if (stride % 3 == 0) stride += 2;
        }
        std::vector<float> samp;
        samp.reserve(n / stride + 1);
        for (size_t i = 0; i < n; i += stride) samp.push_back(train_data[i]);
        const size_t k = samp.size() / 200; /* 0.5% per side */
        std::nth_element(samp.begin(), samp.begin() + k, samp.end());
        const float lo = samp[k];
        std::nth_element(samp.begin(), samp.end() - 1 - k, samp.end());
        const float hi = samp[samp.size() - 1 - k];
        gpu_ivf_flat_set_quantizer(h, lo, hi, errmsg);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_train_quantizer", e.what());
    }
}

/* ---- info (ivf_flat_c.h:159; field set of index_base.hpp:2098-2117) ----- */

char* gpu_ivf_flat_info(gpu_ivf_flat_c h, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        char buf[512];
        snprintf(buf, sizeof buf,
                 "{\"element_size\": %zu, \"dimension\": %u, \"metric\": %d, "
                 "\"status\": \"%s\", \"capacity\": %llu, "
                 "\"current_length\": %llu, \"dist_mode\": 0, "
                 "\"has_ids\": true, \"devices\": [%d], \"n_lists\": %u, "
                 "\"qtype\": %d, \"btype\": %d, \"deleted_count\": %llu}",
                 storage_elem_bytes(ix->qtype), ix->dim, (int)ix->metric,
                 ix->built ? "Loaded" : "Empty",
                 (unsigned long long)ix->cap,
                 (unsigned long long)total_len(ix), ix->device, ix->nlist,
                 (int)ix->qtype, (int)ix->btype,
                 (unsigned long long)(ix->deleted_count +
                                      (ix->tail ? ix->tail->deleted_count
                                                : 0)));
        return strdup(buf);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_info", e.what());
        return nullptr;
    }
}

/* ---- dynamic-batching knob (ivf_flat_c.h:92) ---------------------------- */

void gpu_ivf_flat_set_dynb_conservative_dispatch(gpu_ivf_flat_c h,
                                                 bool enable, void* errmsg) {
    try {
        IX(h)->dynb_conservative = enable;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_set_dynb_conservative_dispatch",
                   e.what());
    }
}

/* ---- pre-filter INCLUDE columns (ivf_flat_c.h:165-199) ------------------ */

void gpu_ivf_flat_set_filter_columns(gpu_ivf_flat_c h,
                                     const char* col_meta_json,
                                     uint64_t total_count, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->built)
            throw std::runtime_error("set_filter_columns must precede build");
        if (!col_meta_json) throw std::runtime_error("null col_meta_json");
        (void)total_count;
        /* minimal parse: per column object, the "type" field
         * (cagra_c.h:166-167: 0=i32, 1=i64, 2=f32, 3=f64, 4=u64) */
        std::vector<int> types;
        const char* p = col_meta_json;
        while ((p = strstr(p, "\"type\""))) {
            p += 6;
            while (*p == ':' || *p == ' ') ++p;
            if (*p < '0' || *p > '9')
                throw std::runtime_error("malformed col_meta_json");
            types.push_back(atoi(p));
        }
        if (types.empty())
            throw std::runtime_error("col_meta_json declares no columns");
        for (int t : types)
            if (t < 0 || t > 4)
                throw std::runtime_error("unknown column type");
        ix->filter_cols_json = col_meta_json;
        ix->filter_col_types = std::move(types);
        ix->filter_col_data.assign(ix->filter_col_types.size(), {});
        ix->filter_col_nulls.assign(ix->filter_col_types.size(), {});
        ix->filter_col_rows.assign(ix->filter_col_types.size(), 0);
        ix->filter_col_has_nulls.assign(ix->filter_col_types.size(), false);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_set_filter_columns", e.what());
    }
}

void gpu_ivf_flat_add_filter_chunk(gpu_ivf_flat_c h, uint32_t col_idx,
                                   const void* data,
                                   const uint32_t* null_bitmap,
                                   uint64_t nrows, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->built)
            throw std::runtime_error("add_filter_chunk must precede build");
        if (col_idx >= ix->filter_col_types.size())
            throw std::runtime_error("column index out of range");
        static const size_t esz[5] = {4, 8, 4, 8, 8};
        const size_t eb = esz[ix->filter_col_types[col_idx]];
        auto& d = ix->filter_col_data[col_idx];
        auto& nl = ix->filter_col_nulls[col_idx];
        const uint64_t base = ix->filter_col_rows[col_idx];
        d.insert(d.end(), (const uint8_t*)data,
                 (const uint8_t*)data + nrows * eb);
        /* null words are re-packed from the chunk base so chunks of any
         * size concatenate (stored LSB-first over the FULL column) */
        nl.resize((size_t)((base + nrows + 31) / 32), 0);
        if (null_bitmap) {
            ix->filter_col_has_nulls[col_idx] = true;
            for (uint64_t i = 0; i < nrows; ++i)
                if ((null_bitmap[i / 32] >> (i % 32)) & 1u) {
                    const uint64_t g = base + i;
                    nl[g / 32] |= (1u << (g % 32));
                }
        }
        ix->filter_col_rows[col_idx] = base + nrows;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_add_filter_chunk", e.what());
    }
}

/* slot bitset over [main + tail] from a preds_json over the registered
 * columns; tail rows (post-build extends have no column rows) fail closed */
static std::vector<uint32_t> preds_bitset(IvfIndex* ix,
                                          const char* preds_json) {
    if (ix->filter_col_types.empty())
        throw std::runtime_error(
            "no filter columns registered (gpu_ivf_flat_set_filter_columns)");
    for (size_t c = 0; c < ix->filter_col_types.size(); ++c)
        if (ix->filter_col_rows[c] != ix->count)
            throw std::runtime_error("filter column rows != index rows");
    std::vector<const void*> cdata(ix->filter_col_types.size());
    std::vector<const uint32_t*> cnulls(ix->filter_col_types.size());
    for (size_t c = 0; c < ix->filter_col_types.size(); ++c) {
        cdata[c] = ix->filter_col_data[c].data();
        cnulls[c] = ix->filter_col_has_nulls[c]
                        ? ix->filter_col_nulls[c].data()
                        : nullptr;
    }
    const uint64_t total = total_len(ix);
    std::vector<uint32_t> words((size_t)((total + 31) / 32), 0);
    char* inner = nullptr;
    const int rc = moann_ivf_flat_filter_from_preds(
        (gpu_ivf_flat_c)ix, ix->filter_cols_json.c_str(), preds_json,
        cdata.data(), cnulls.data(), words.data(), &inner);
    if (rc != 0 || inner) {
        std::string m = inner ? inner : "predicate evaluation failed";
        if (inner) free(inner);
        throw std::runtime_error(m);
    }
    /* tail region (bits >= main count) stays 0: fail closed */
    if (ix->count % 32) {
        const uint64_t w = ix->count / 32;
        words[w] &= (1u << (ix->count % 32)) - 1u;
    }
    return words;
}

gpu_ivf_flat_search_res_t gpu_ivf_flat_search_with_filter(
    gpu_ivf_flat_c h, const void* queries_data, uint64_t num_queries,
    uint32_t query_dimension, uint32_t limit, ivf_flat_search_params_t sp,
    const char* preds_json, void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (!preds_json || !*preds_json)
            return gpu_ivf_flat_search(h, queries_data, num_queries,
                                       query_dimension, limit, sp, errmsg);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        const float* q = (const float*)queries_data;
        std::vector<float> conv;
        if (ix->qtype != Quantization_F32) {
            conv.resize((size_t)num_queries * ix->dim);
            storage_to_f32(ix->qtype, queries_data, conv.size(),
                           ix->quant_mul, ix->quant_add, conv.data());
            q = conv.data();
        }
        auto words = preds_bitset(ix, preds_json);
        out.result_ptr = run_search_full(ix, q, false, num_queries, limit,
                                         sp.n_probes, words.data(),
                                         total_len(ix))
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_with_filter", e.what());
    }
    return out;
}

gpu_ivf_flat_search_res_t gpu_ivf_flat_search_quantize_with_filter(
    gpu_ivf_flat_c h, const void* queries_data, uint64_t num_queries,
    uint32_t query_dimension, uint32_t limit, ivf_flat_search_params_t sp,
    const char* preds_json, void* errmsg) {
    gpu_ivf_flat_search_res_t out {nullptr};
    try {
        auto ix = IX(h);
        if (!preds_json || !*preds_json)
            return gpu_ivf_flat_search_quantize(h, queries_data, num_queries,
                                                query_dimension, limit, sp,
                                                errmsg);
        if (query_dimension != ix->dim)
            throw std::runtime_error("query dimension mismatch");
        const float* q = (const float*)queries_data;
        std::vector<float> conv;
        if (ix->btype != Quantization_F32) {
            conv = base_to_f32(ix->btype, queries_data,
                               (size_t)num_queries * ix->dim);
            q = conv.data();
        }
        auto words = preds_bitset(ix, preds_json);
        out.result_ptr = run_search_full(ix, q, false, num_queries, limit,
                                         sp.n_probes, words.data(),
                                         total_len(ix))
                             .release();
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_quantize_with_filter",
                   e.what());
    }
    return out;
}

uint64_t gpu_ivf_flat_search_quantize_with_filter_async(
    gpu_ivf_flat_c h, const void* queries_data, uint64_t num_queries,
    uint32_t query_dimension, uint32_t limit, ivf_flat_search_params_t sp,
    const char* preds_json, void* errmsg) {
    try {
        auto ix = IX(h);
        if (!preds_json || !*preds_json)
            return gpu_ivf_flat_search_quantize_async(
                h, queries_data, num_queries, query_dimension, limit, sp,
                errmsg);
        /* filtered async executes at submit and parks the result for
         * search_wait, like the unbatched async path */
        auto res = gpu_ivf_flat_search_quantize_with_filter(
            h, queries_data, num_queries, query_dimension, limit, sp,
            preds_json, errmsg);
        if (!res.result_ptr) return 0;
        std::lock_guard<std::mutex> lk(ix->mu);
        const uint64_t id = ix->next_job++;
        ix->jobs[id] = std::unique_ptr<Result>((Result*)res.result_ptr);
        return id;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_search_quantize_with_filter_async",
                   e.what());
        return 0;
    }
}

/* save_dir / load_dir — the persistence contract of the reference GPU
 * index (cgo/cuvs/index_base.hpp:239-249, gpu_ivf_flat_save_dir/load_dir in
 * ivf_flat_c.h:98-106): a directory with manifest.json + per-component
 * blobs; load recreates the index into a handle that was created (with
 * matching dim/metric/n_lists) and started. Vectors/ids are stored in SLOT
 * order (equivalent list contents and in-list order). */
void gpu_ivf_flat_save_dir(gpu_ivf_flat_c h, const char* dir, void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built) throw std::runtime_error("index not built");
        HIP_CHECK(hipSetDevice(ix->device));
        IvfIndex* tl = (ix->tail && ix->tail->count) ? ix->tail.get()
                                                     : nullptr;
        const uint64_t total = total_len(ix);
        const uint64_t ndel =
            ix->deleted_count + (tl ? tl->deleted_count : 0);
        std::string d(dir);
        auto wfile = [&](const std::string& name, const void* p, size_t n) {
            FILE* f = fopen((d + "/" + name).c_str(), "wb");
            if (!f) throw std::runtime_error("cannot write " + name);
            if (n && fwrite(p, 1, n, f) != n) {
                fclose(f);
                throw std::runtime_error("short write " + name);
            }
            fclose(f);
        };
        {
            char buf[512];
            snprintf(buf, sizeof buf,
                     "{\n  \"format\": \"moann-ivf-flat-v1\",\n"
                     "  \"dimension\": %u,\n  \"n_lists\": %u,\n"
                     "  \"metric\": %d,\n  \"count\": %llu,\n"
                     "  \"qtype\": %d,\n"
                     "  \"quant_min\": %.17g,\n  \"quant_max\": %.17g,\n"
                     "  \"quant_mul\": %.17g,\n"
                     "  \"deleted_count\": %llu\n}\n",
                     ix->dim, ix->nlist, (int)ix->metric,
                     (unsigned long long)total, (int)ix->qtype,
                     ix->quant_min, ix->quant_max, ix->quant_mul,
                     (unsigned long long)ndel);
            wfile("manifest.json", buf, strlen(buf));
        }
        wfile("centroids.f32", ix->h_centroids.data(),
              ix->h_centroids.size() * 4);
        /* rows are saved main-slot-order then tail-slot-order; extends fold
         * back into an ordinary (tail-free) index on load */
        {
            std::vector<int64_t> idsv(ix->h_id_by_slot.begin(),
                                      ix->h_id_by_slot.begin() + ix->count);
            if (tl)
                idsv.insert(idsv.end(), tl->h_id_by_slot.begin(),
                            tl->h_id_by_slot.begin() + tl->count);
            wfile("ids.i64", idsv.data(), idsv.size() * 8);
        }
        /* per-slot list id (assignments in slot order) */
        {
            std::vector<int32_t> a(total);
            for (uint32_t l = 0; l < ix->nlist; ++l)
                for (int64_t sidx = ix->list_slot_base[l];
                     sidx < ix->list_slot_base[l] + ix->list_rows[l]; ++sidx)
                    a[sidx] = (int32_t)l;
            if (tl)
                for (uint32_t l = 0; l < tl->nlist; ++l)
                    for (int64_t sidx = tl->list_slot_base[l];
                         sidx < tl->list_slot_base[l] + tl->list_rows[l];
                         ++sidx)
                        a[ix->count + sidx] = (int32_t)l;
            wfile("assign.i32", a.data(), total * 4);
        }
        /* soft-delete bitset in SAVED row order (bit = 1 alive), only when
         * deletions exist (index_base.hpp:246 "omitted if no deletions") */
        if (ndel) {
            std::vector<uint32_t> bits((size_t)((total + 31) / 32), ~0u);
            auto fold = [&](IvfIndex* s, uint64_t base) {
                for (size_t w = 0; w < s->alive.size(); ++w) {
                    const uint32_t inv = ~s->alive[w];
                    if (!inv) continue;
                    for (int b = 0; b < 32; ++b)
                        if ((inv >> b) & 1u) {
                            const uint64_t g = base + w * 32 + b;
                            if (g - base < s->count)
                                bits[g / 32] &= ~(1u << (g % 32));
                        }
                }
            };
            fold(ix, 0);
            if (tl) fold(tl, ix->count);
            wfile("bitset.bin", bits.data(), bits.size() * 4);
        }
        if (ix->qtype != Quantization_F32) {
            /* narrow storage: the f32 staging was dropped at build; save the
             * QUANTIZED bytes (vectors.u8). load_dir dequantizes with the
             * manifest's quantizer and re-quantizes at build — an exact
             * round trip (integer codes survive the f32 detour: the
             * reconstruction error is << 0.5 code steps). */
            FILE* f = fopen((d + "/vectors.u8").c_str(), "wb");
            if (!f) throw std::runtime_error("cannot write vectors.u8");
            const size_t s_eb = (ix->qtype == Quantization_F16 ||
                                 ix->qtype == Quantization_BF16)
                                    ? 2 : 1; /* bytes per element */
            auto dump_bytes = [&](IvfIndex* s) {
                DevBuf d_gsb, d_gv, d_tmp;
                d_gsb.ensure(s->total_groups * 8);
                d_gv.ensure(s->total_groups * 4);
                HIP_CHECK(hipMemcpy(d_gsb.ptr, s->group_slotbase.data(),
                                    s->total_groups * 8,
                                    hipMemcpyHostToDevice));
                HIP_CHECK(hipMemcpy(d_gv.ptr, s->group_valid.data(),
                                    s->total_groups * 4,
                                    hipMemcpyHostToDevice));
                const int64_t CH = 1 << 21;
                d_tmp.ensure((size_t)CH * s->dim * s_eb);
                std::vector<uint8_t> hbuf((size_t)CH * s->dim * s_eb);
                for (int64_t lo = 0; lo < (int64_t)s->count; lo += CH) {
                    const int64_t hi = std::min<int64_t>(lo + CH, s->count);
                    launch_unpack_bytes(
                        s->d_packed_q, (int)(s->dim * s_eb),
                        (int)(s->dpad * s_eb), d_gsb.as<int64_t>(),
                        d_gv.as<int32_t>(), s->total_groups, lo, hi,
                        d_tmp.as<uint8_t>(), s->stream);
                    HIP_CHECK(hipMemcpyAsync(
                        hbuf.data(), d_tmp.ptr,
                        (size_t)(hi - lo) * s->dim * s_eb,
                        hipMemcpyDeviceToHost, s->stream));
                    HIP_CHECK(hipStreamSynchronize(s->stream));
                    HIP_CHECK(hipGetLastError());
                    const size_t n = (size_t)(hi - lo) * s->dim * s_eb;
                    if (fwrite(hbuf.data(), 1, n, f) != n) {
                        fclose(f);
                        throw std::runtime_error("short write vectors.u8");
                    }
                }
            };
            dump_bytes(ix);
            if (tl) dump_bytes(tl);
            fclose(f);
        } else
        /* vectors.f32: unpack in chunks of groups */
        {
            FILE* f = fopen((d + "/vectors.f32").c_str(), "wb");
            if (!f) throw std::runtime_error("cannot write vectors.f32");
            auto dump_f32 = [&](IvfIndex* s) {
                DevBuf d_gsb, d_gv, d_tmp;
                d_gsb.ensure(s->total_groups * 8);
                d_gv.ensure(s->total_groups * 4);
                HIP_CHECK(hipMemcpy(d_gsb.ptr, s->group_slotbase.data(),
                                    s->total_groups * 8,
                                    hipMemcpyHostToDevice));
                HIP_CHECK(hipMemcpy(d_gv.ptr, s->group_valid.data(),
                                    s->total_groups * 4,
                                    hipMemcpyHostToDevice));
                const int64_t CH = 1 << 20; /* slots per chunk */
                d_tmp.ensure((size_t)CH * s->dim * 4);
                std::vector<float> hbuf((size_t)CH * s->dim);
                for (int64_t lo = 0; lo < (int64_t)s->count; lo += CH) {
                    const int64_t hi = std::min<int64_t>(lo + CH, s->count);
                    launch_unpack(s->d_packed, (int)s->dim, (int)s->dpad,
                                  d_gsb.as<int64_t>(), d_gv.as<int32_t>(),
                                  s->total_groups, lo, hi,
                                  d_tmp.as<float>(), s->stream);
                    HIP_CHECK(hipMemcpyAsync(
                        hbuf.data(), d_tmp.ptr,
                        (size_t)(hi - lo) * s->dim * 4,
                        hipMemcpyDeviceToHost, s->stream));
                    HIP_CHECK(hipStreamSynchronize(s->stream));
                    HIP_CHECK(hipGetLastError());
                    const size_t n = (size_t)(hi - lo) * s->dim * 4;
                    if (fwrite(hbuf.data(), 1, n, f) != n) {
                        fclose(f);
                        throw std::runtime_error("short write vectors.f32");
                    }
                }
            };
            dump_f32(ix);
            if (tl) dump_f32(tl);
            fclose(f);
        }
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_save_dir", e.what());
    }
}

void gpu_ivf_flat_load_dir(gpu_ivf_flat_c h, const char* dir,
                           distribution_mode_t /*target_mode*/, void* errmsg) {
    try {
        auto ix = IX(h);
        if (ix->built) throw std::runtime_error("index already built");
        std::string d(dir);
        auto rfile = [&](const std::string& name, void* p, size_t n) {
            FILE* f = fopen((d + "/" + name).c_str(), "rb");
            if (!f) throw std::runtime_error("cannot read " + name);
            const size_t got = fread(p, 1, n, f);
            fclose(f);
            if (got != n) throw std::runtime_error("short read " + name);
        };
        /* manifest: minimal field validation */
        {
            FILE* f = fopen((d + "/manifest.json").c_str(), "rb");
            if (!f) throw std::runtime_error("cannot read manifest.json");
            char buf[1024] = {0};
            size_t got = fread(buf, 1, sizeof buf - 1, f);
            fclose(f);
            (void)got;
            unsigned dim = 0, nlist = 0;
            unsigned long long count = 0;
            int metric = 0;
            if (!strstr(buf, "moann-ivf-flat-v1"))
                throw std::runtime_error("unknown manifest format");
            const char* fdim = strstr(buf, "\"dimension\":");
            const char* fnl = strstr(buf, "\"n_lists\":");
            const char* fme = strstr(buf, "\"metric\":");
            const char* fct = strstr(buf, "\"count\":");
            if (!fdim || !fnl || !fme || !fct)
                throw std::runtime_error("malformed manifest.json");
            sscanf(fdim, "\"dimension\": %u", &dim);
            sscanf(fnl, "\"n_lists\": %u", &nlist);
            sscanf(fme, "\"metric\": %d", &metric);
            sscanf(fct, "\"count\": %llu", &count);
            if (dim != ix->dim || nlist != ix->nlist ||
                metric != (int)ix->metric)
                throw std::runtime_error(
                    "manifest does not match the created index");
            if (count > ix->cap)
                throw std::runtime_error("manifest count exceeds capacity");
            int qtype = (int)Quantization_F32;
            double qmin = 0.0, qmax = 0.0;
            if (const char* q = strstr(buf, "\"qtype\":"))
                sscanf(q, "\"qtype\": %d", &qtype);
            if (const char* q = strstr(buf, "\"quant_min\":"))
                sscanf(q, "\"quant_min\": %lg", &qmin);
            if (const char* q = strstr(buf, "\"quant_max\":"))
                sscanf(q, "\"quant_max\": %lg", &qmax);
            if (qtype != (int)ix->qtype)
                throw std::runtime_error(
                    "manifest storage type does not match the created index");
            std::vector<float> cents((size_t)nlist * dim);
            rfile("centroids.f32", cents.data(), cents.size() * 4);
            moann_ivf_flat_set_centroids(h, cents.data(), nlist, errmsg);
            std::vector<int64_t> ids(count);
            rfile("ids.i64", ids.data(), count * 8);
            std::vector<int32_t> assign(count);
            rfile("assign.i32", assign.data(), count * 4);
            /* vectors streamed into add_chunk */
            const bool narrow = qtype != (int)Quantization_F32;
            const bool l_half_pre = qtype == (int)Quantization_F16 ||
                                    qtype == (int)Quantization_BF16;
            const char* vname = narrow ? "/vectors.u8" : "/vectors.f32";
            FILE* vf = fopen((d + vname).c_str(), "rb");
            if (!vf)
                throw std::runtime_error(std::string("cannot read ") + vname);
            if (narrow && !l_half_pre) {
                /* pin the quantizer BEFORE build so re-quantization uses
                 * the saved parameters (halves are plain casts) */
                gpu_ivf_flat_set_quantizer(h, (float)qmin, (float)qmax,
                                           errmsg);
            }
            const double mul = ix->quant_mul, add = ix->quant_add;
            const bool l_half = qtype == (int)Quantization_F16 ||
                                qtype == (int)Quantization_BF16;
            const size_t l_eb = l_half ? 2 : 1;
            const size_t CH = 1 << 20;
            std::vector<float> vbuf(CH * dim);
            std::vector<uint8_t> qbuf(narrow ? CH * dim * l_eb : 0);
            unsigned long long done = 0;
            while (done < count) {
                const size_t n = (size_t)std::min<unsigned long long>(
                    CH, count - done);
                if (narrow) {
                    if (fread(qbuf.data(), 1, n * dim * l_eb, vf) !=
                        n * dim * l_eb) {
                        fclose(vf);
                        throw std::runtime_error("short read vectors.u8");
                    }
                    if (l_half) {
                        const uint16_t* hp = (const uint16_t*)qbuf.data();
                        const bool bf = qtype == (int)Quantization_BF16;
                        for (size_t i = 0; i < n * dim; ++i) {
                            const uint16_t b = hp[i];
                            uint32_t u;
                            if (bf) {
                                u = (uint32_t)b << 16;
                            } else { /* IEEE binary16 -> binary32 widen */
                                const uint32_t sign = (uint32_t)(b & 0x8000)
                                                      << 16;
                                uint32_t exp = (b >> 10) & 0x1f;
                                uint32_t coef = b & 0x3ff;
                                if (exp == 0x1f) {
                                    u = sign | 0x7f800000u | (coef << 13);
                                } else if (exp == 0 && coef == 0) {
                                    u = sign;
                                } else {
                                    if (exp == 0) { /* subnormal */
                                        exp = 1;
                                        while (!(coef & 0x400)) {
                                            coef <<= 1;
                                            exp--;
                                        }
                                        coef &= 0x3ff;
                                    }
                                    u = sign | ((exp + 112) << 23) |
                                        (coef << 13);
                                }
                            }
                            float fv;
                            memcpy(&fv, &u, 4);
                            vbuf[i] = fv;
                        }
                    } else {
                        const bool uns = qtype == (int)Quantization_UINT8;
                        for (size_t i = 0; i < n * dim; ++i) {
                            const double q = uns ? (double)qbuf[i]
                                                 : (double)(int8_t)qbuf[i];
                            vbuf[i] = (float)((q - add) / mul);
                        }
                    }
                } else if (fread(vbuf.data(), 4, n * dim, vf) != n * dim) {
                    fclose(vf);
                    throw std::runtime_error("short read vectors.f32");
                }
                gpu_ivf_flat_add_chunk_float(h, vbuf.data(), n,
                                             ids.data() + done, errmsg);
                done += n;
            }
            fclose(vf);
            moann_ivf_flat_set_assignments(h, assign.data(), count, errmsg);
            gpu_ivf_flat_build(h, errmsg);
            /* soft-delete bitset (saved in ROW order, bit = 1 alive):
             * re-key to the rebuilt slot order via slot_rows */
            FILE* bf = fopen((d + "/bitset.bin").c_str(), "rb");
            if (bf) {
                std::vector<uint32_t> bits((size_t)((count + 31) / 32));
                const size_t got = fread(bits.data(), 4, bits.size(), bf);
                fclose(bf);
                if (got != bits.size())
                    throw std::runtime_error("short read bitset.bin");
                ix->alive.assign((size_t)((ix->count + 31) / 32), ~0u);
                ix->deleted_count = 0;
                for (uint64_t slot = 0; slot < ix->count; ++slot) {
                    const uint64_t row = (uint64_t)ix->h_slot_rows[slot];
                    const bool al = (bits[row / 32] >> (row % 32)) & 1u;
                    if (!al) {
                        ix->alive[slot / 32] &= ~(1u << (slot % 32));
                        ++ix->deleted_count;
                    }
                }
            }
        }
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_load_dir", e.what());
    }
}

/* ---- single-file save/load (ivf_flat_c.h:95, 48-51) ---------------------
 * Container: "MOANNPK1\n" then per blob [u32 name_len][name][u64 size]
 * [payload], wrapping the save_dir blob set. Written/read only by this
 * library (the reference's counterpart is cuVS-serialize, equally
 * internal). */

static const char* kPackMagic = "MOANNPK1\n";

static std::string pack_tmpdir() {
    char tmpl[] = "/tmp/moannpk.XXXXXX";
    char* p = mkdtemp(tmpl);
    if (!p) throw std::runtime_error("mkdtemp failed");
    return std::string(p);
}

static void rm_rf_dir(const std::string& d,
                      const std::vector<std::string>& names) {
    for (const auto& n : names) (void)remove((d + "/" + n).c_str());
    (void)remove(d.c_str());
}

static const std::vector<std::string> kPackNames = {
    "manifest.json", "centroids.f32", "ids.i64", "assign.i32",
    "bitset.bin", "vectors.f32", "vectors.u8"};

void gpu_ivf_flat_save(gpu_ivf_flat_c h, const char* filename,
                       void* errmsg) {
    std::string tmp;
    try {
        tmp = pack_tmpdir();
        char* inner = nullptr;
        gpu_ivf_flat_save_dir(h, tmp.c_str(), &inner);
        if (inner) {
            std::string m(inner);
            free(inner);
            throw std::runtime_error(m);
        }
        FILE* out = fopen(filename, "wb");
        if (!out) throw std::runtime_error("cannot write file");
        fwrite(kPackMagic, 1, strlen(kPackMagic), out);
        std::vector<uint8_t> buf(1 << 20);
        for (const auto& n : kPackNames) {
            FILE* f = fopen((tmp + "/" + n).c_str(), "rb");
            if (!f) continue; /* optional blobs (bitset, one of vectors.*) */
            fseek(f, 0, SEEK_END);
            const uint64_t sz = (uint64_t)ftell(f);
            fseek(f, 0, SEEK_SET);
            const uint32_t nl = (uint32_t)n.size();
            fwrite(&nl, 4, 1, out);
            fwrite(n.data(), 1, nl, out);
            fwrite(&sz, 8, 1, out);
            uint64_t left = sz;
            while (left) {
                const size_t c = (size_t)std::min<uint64_t>(left, buf.size());
                if (fread(buf.data(), 1, c, f) != c) {
                    fclose(f);
                    fclose(out);
                    throw std::runtime_error("short read packing " + n);
                }
                fwrite(buf.data(), 1, c, out);
                left -= c;
            }
            fclose(f);
        }
        fclose(out);
        rm_rf_dir(tmp, kPackNames);
    } catch (const std::exception& e) {
        if (!tmp.empty()) rm_rf_dir(tmp, kPackNames);
        set_errmsg(errmsg, "gpu_ivf_flat_save", e.what());
    }
}

gpu_ivf_flat_c gpu_ivf_flat_load_file(const char* filename,
                                      uint32_t dimension,
                                      distance_type_t metric,
                                      ivf_flat_build_params_t build_params,
                                      const int* devices, int device_count,
                                      uint32_t nthread,
                                      distribution_mode_t dist_mode,
                                      quantization_t btype,
                                      quantization_t qtype, void* errmsg) {
    std::string tmp;
    gpu_ivf_flat_c h = nullptr;
    try {
        FILE* in = fopen(filename, "rb");
        if (!in) throw std::runtime_error("cannot read file");
        char magic[16] = {0};
        if (fread(magic, 1, strlen(kPackMagic), in) != strlen(kPackMagic) ||
            strncmp(magic, kPackMagic, strlen(kPackMagic)) != 0) {
            fclose(in);
            throw std::runtime_error("not a moann pack file");
        }
        tmp = pack_tmpdir();
        std::vector<uint8_t> buf(1 << 20);
        uint64_t count = 0;
        for (;;) {
            uint32_t nl = 0;
            if (fread(&nl, 4, 1, in) != 1) break; /* EOF */
            if (nl == 0 || nl > 64) {
                fclose(in);
                throw std::runtime_error("corrupt pack header");
            }
            std::string name(nl, 0);
            uint64_t sz = 0;
            if (fread(&name[0], 1, nl, in) != nl ||
                fread(&sz, 8, 1, in) != 1) {
                fclose(in);
                throw std::runtime_error("corrupt pack entry");
            }
            if (name.find('/') != std::string::npos) {
                fclose(in);
                throw std::runtime_error("bad blob name");
            }
            FILE* f = fopen((tmp + "/" + name).c_str(), "wb");
            if (!f) {
                fclose(in);
                throw std::runtime_error("cannot write temp blob");
            }
            uint64_t left = sz;
            while (left) {
                const size_t c = (size_t)std::min<uint64_t>(left, buf.size());
                if (fread(buf.data(), 1, c, in) != c ||
                    fwrite(buf.data(), 1, c, f) != c) {
                    fclose(f);
                    fclose(in);
                    throw std::runtime_error("short pack payload");
                }
                left -= c;
            }
            fclose(f);
            if (name == "manifest.json") {
                /* capacity for the new_empty below */
                FILE* mf = fopen((tmp + "/manifest.json").c_str(), "rb");
                char mb[1024] = {0};
                if (mf) {
                    size_t r = fread(mb, 1, sizeof mb - 1, mf);
                    (void)r;
                    fclose(mf);
                }
                const char* fc = strstr(mb, "\"count\":");
                if (fc) sscanf(fc, "\"count\": %llu",
                               (unsigned long long*)&count);
            }
        }
        fclose(in);
        char* inner = nullptr;
        h = gpu_ivf_flat_new_empty(count, dimension, metric, build_params,
                                   devices, device_count, nthread,
                                   dist_mode, btype, qtype, nullptr, &inner);
        if (!h) {
            std::string m = inner ? inner : "new_empty failed";
            if (inner) free(inner);
            throw std::runtime_error(m);
        }
        gpu_ivf_flat_start(h, &inner);
        gpu_ivf_flat_load_dir(h, tmp.c_str(), dist_mode, &inner);
        if (inner) {
            std::string m(inner);
            free(inner);
            throw std::runtime_error(m);
        }
        rm_rf_dir(tmp, kPackNames);
        return h;
    } catch (const std::exception& e) {
        if (h) gpu_ivf_flat_destroy(h, nullptr);
        if (!tmp.empty()) rm_rf_dir(tmp, kPackNames);
        set_errmsg(errmsg, "gpu_ivf_flat_load_file", e.what());
        return nullptr;
    }
}

/* ivf_flat_c.h:93-94 set/get_quantizer: trains the affine scalar quantizer
 * from [min,max] with the reference formulas (quantizer.go:90-100 Int8Params
 * mul=255/rng, add=-min*mul-128; :232-240 Uint8Params without the -128
 * shift). Call before build; search rescales raw scores by 1/mul^2
 * (search.go:1062-1077). */
/* Two-stage scan: byte-quantized first pass (internal CLIP quantizer over
 * sampled 0.1%/99.9% quantiles — independent of the MO storage quantizer)
 * + exact f32 re-rank of the per-query top-R. Standard SQ8-with-refine;
 * cuts first-pass HBM traffic 4x. f32 storage only; opt-in (the default
 * path stays the exact one-pass scan). */
void moann_ivf_flat_enable_refine(gpu_ivf_flat_c h, uint32_t depth,
                                  void* errmsg) {
    try {
        auto ix = IX(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->built) throw std::runtime_error("index not built");
        if (ix->qtype != Quantization_F32)
            throw std::runtime_error("refine applies to f32 storage");
        if (depth == 0) { ix->refine_depth = 0; return; }
        if (depth > 4096) throw std::runtime_error("refine depth > 4096");
        HIP_CHECK(hipSetDevice(ix->device));
        if (!ix->d_rows_f32) {
            DevBuf d_gsb, d_gv;
            d_gsb.ensure(ix->total_groups * 8);
            d_gv.ensure(ix->total_groups * 4);
            HIP_CHECK(hipMemcpy(d_gsb.ptr, ix->group_slotbase.data(),
                                ix->total_groups * 8, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_gv.ptr, ix->group_valid.data(),
                                ix->total_groups * 4, hipMemcpyHostToDevice));
            /* row-major f32 copy for the exact re-rank */
            HIP_CHECK(hipMalloc(&ix->d_rows_f32,
                                std::max<uint64_t>(1, ix->count) *
                                    ix->dim * 4));
            launch_unpack(ix->d_packed, (int)ix->dim, (int)ix->dpad,
                          d_gsb.as<int64_t>(), d_gv.as<int32_t>(),
                          ix->total_groups, 0, (int64_t)ix->count,
                          ix->d_rows_f32, ix->stream);
            HIP_CHECK(hipStreamSynchronize(ix->stream));
            KCHECK("refine-unpack");
            /* clip quantizer from sampled quantiles */
            const uint64_t ns = std::min<uint64_t>(ix->count, 131072);
            std::vector<float> samp((size_t)ns * ix->dim);
            HIP_CHECK(hipMemcpy(samp.data(), ix->d_rows_f32, samp.size() * 4,
                                hipMemcpyDeviceToHost));
            const size_t nlo = samp.size() / 1000;
            std::nth_element(samp.begin(), samp.begin() + nlo, samp.end());
            const double lo = samp[nlo];
            std::nth_element(samp.begin(), samp.end() - 1 - nlo, samp.end());
            const double hi = samp[samp.size() - 1 - nlo];
            const double rng = hi - lo;
            ix->rq_mul = rng > 0 ? 255.0 / rng : 1.0;
            ix->rq_add = rng > 0 ? -lo * ix->rq_mul - 128.0 : 0.0;
            /* quantize rows -> pack (16-byte units when possible) */
            DevBuf d_qrows, d_ident;
            d_qrows.ensure((size_t)std::max<uint64_t>(1, ix->count) *
                           ix->dpad);
            launch_quantize_rows(false, ix->d_rows_f32, (int64_t)ix->count,
                                 (int)ix->dim, (int)ix->dim, (int)ix->dpad,
                                 (float)ix->rq_mul, (float)ix->rq_add,
                                 d_qrows.as<uint8_t>(), ix->stream);
            KCHECK("refine-quantize");
            std::vector<int64_t> ident(std::max<uint64_t>(1, ix->count));
            for (uint64_t i = 0; i < ix->count; ++i) ident[i] = (int64_t)i;
            d_ident.ensure(ident.size() * 8);
            HIP_CHECK(hipMemcpy(d_ident.ptr, ident.data(), ident.size() * 8,
                                hipMemcpyHostToDevice));
            HIP_CHECK(hipMalloc(&ix->d_packed_rq,
                                (size_t)ix->total_groups * 64 * ix->dpad));
            /* byte order follows the kernel that will scan: the variant
             * pick_scan gives this index's refine scan (row norms exist
             * whenever dpad % 16 == 0), fixed for the process */
            const bool norms = (ix->dpad & 15) == 0;
            ix->rq_layout = pick_refine_layout(
                ix->kmetric,
                pick_scan(ix->kmetric, (int)ix->dpad, ix->qtype, true, norms,
                          scan_overrides()).list,
                (int)ix->dpad, scan_overrides());
            if (ix->rq_layout == ByteImageLayout::MFMA64)
                launch_bytes_pack_mfma(d_qrows.as<uint8_t>(), (int)ix->dpad,
                                       d_gsb.as<int64_t>(),
                                       d_gv.as<int32_t>(),
                                       d_ident.as<int64_t>(),
                                       ix->total_groups, ix->d_packed_rq,
                                       ix->stream);
            else if (norms)
                launch_bytes_pack16(d_qrows.as<uint8_t>(), (int)ix->dpad,
                                    d_gsb.as<int64_t>(), d_gv.as<int32_t>(),
                                    d_ident.as<int64_t>(), ix->total_groups,
                                    ix->d_packed_rq, ix->stream);
            else
                launch_pq_pack(d_qrows.as<uint8_t>(), (int)ix->dpad,
                               d_gsb.as<int64_t>(), d_gv.as<int32_t>(),
                               d_ident.as<int64_t>(), ix->total_groups,
                               ix->d_packed_rq, ix->stream);
            KCHECK("refine-pack");
            if (norms) {
                HIP_CHECK(hipMalloc(&ix->d_rownorm_rq,
                                    (size_t)ix->total_groups * 64 * 4));
                launch_rownorms_i8(false, ix->rq_layout, ix->d_packed_rq,
                                   ix->total_groups,
                                   (int)ix->dpad, ix->d_rownorm_rq,
                                   ix->stream);
            }
            HIP_CHECK(hipStreamSynchronize(ix->stream));
            KCHECK("refine-build");
        }
        ix->refine_depth = (int)depth;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_ivf_flat_enable_refine", e.what());
    }
}

void gpu_ivf_flat_set_quantizer(gpu_ivf_flat_c h, float min, float max,
                                void* errmsg) {
    try {
        auto ix = IX(h);
        if (ix->qtype != Quantization_INT8 &&
            ix->qtype != Quantization_UINT8)
            throw std::runtime_error(
                "storage has no affine quantizer (int8/uint8 only)");
        const double rng = (double)max - (double)min;
        ix->quant_min = min;
        ix->quant_max = max;
        if (!(rng > 0) || std::isinf(rng)) {
            ix->quant_mul = 1.0;
            ix->quant_add = 0.0;
        } else {
            ix->quant_mul = 255.0 / rng;
            ix->quant_add = -(double)min * ix->quant_mul +
                            (ix->qtype == Quantization_INT8 ? -128.0 : 0.0);
        }
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_set_quantizer", e.what());
    }
}

void gpu_ivf_flat_get_quantizer(gpu_ivf_flat_c h, float* min, float* max,
                                void* errmsg) {
    try {
        auto ix = IX(h);
        *min = (float)ix->quant_min;
        *max = (float)ix->quant_max;
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_get_quantizer", e.what());
    }
}

/* ivf_flat_c.h:91 gpu_ivf_flat_set_batch_window: window (µs) within which
 * concurrent search_async calls are fused into one device batch
 * (dynamic_batching.hpp:19-60 precedent). 0 disables. */
void gpu_ivf_flat_set_batch_window(gpu_ivf_flat_c h, int64_t window_us,
                                   void* errmsg) {
    try {
        IX(h)->batch_window_us.store(window_us);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "gpu_ivf_flat_set_batch_window", e.what());
    }
}

void moann_ivf_flat_perf(gpu_ivf_flat_c h, moann_perf_t* out) {
    *out = IX(h)->perf.c;
}

void moann_ivf_flat_perf_reset(gpu_ivf_flat_c h) {
    IX(h)->perf.c = moann_perf_t {};
}

/* 1xN pairwise distances — the SQL l2_distance/l2_distance_sq/
 * inner_product/cosine_distance/l1_distance const-query batch
 * (metric.PairwiseDistanceLaunch, func_binary.go:9127; subsumes the legacy
 * cgo/cuda/mocl.cu l2distance kernels). Synchronous; MO conventions;
 * the l2 metric applies sqrt on output. */
void moann_pairwise_distance(distance_type_t metric, const float* query,
                             const float* rows, uint64_t n, uint32_t dim,
                             int device, float* out_dists, void* errmsg) {
    try {
        const int km = metric_kind(metric);
        const int do_sqrt = metric == DistanceType_L2SqrtExpanded;
        HIP_CHECK(hipSetDevice(device));
        DevBuf d_rows, d_q, d_out;
        d_rows.ensure((size_t)n * dim * 4);
        d_q.ensure((size_t)dim * 4);
        d_out.ensure((size_t)n * 4);
        HIP_CHECK(hipMemcpy(d_rows.ptr, rows, (size_t)n * dim * 4,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_q.ptr, query, (size_t)dim * 4,
                            hipMemcpyHostToDevice));
        float qn = 0.f;
        for (uint32_t e = 0; e < dim; ++e) qn += query[e] * query[e];
        launch_pairwise(km, d_rows.as<float>(), d_q.as<float>(), qn,
                        (int64_t)n, (int)dim, d_out.as<float>(), nullptr);
        KCHECK("pairwise");
        HIP_CHECK(hipMemcpy(out_dists, d_out.ptr, (size_t)n * 4,
                            hipMemcpyDeviceToHost));
        if (do_sqrt)
            for (uint64_t i = 0; i < n; ++i)
                out_dists[i] = (float)sqrt((double)out_dists[i]);
    } catch (const std::exception& e) {
        set_errmsg(errmsg, "moann_pairwise_distance", e.what());
    }
}

int moann_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* moann_version(void) { return "moann 0.1.0 (gfx950)"; }

}  /* extern "C" */
