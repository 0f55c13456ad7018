/* Host-side planning of the interleaved scan: which kernel variant scans a
 * given index shape, and the (list segment, query tile) job tables that
 * variant consumes. Pure integer arithmetic — no HIP, no globals — so it
 * runs (and is sanitized) on the CPU: scan_plan_check.cpp. The tile width
 * of a job table and the QT of the kernel that consumes it are ONE decision,
 * made here and passed along as a ScanVariant. */

#ifndef MOANN_SCAN_PLAN_H
#define MOANN_SCAN_PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../../include/moann.h"

namespace moann {

/* Internal metric codes (template selectors for the scan kernel). */
enum MetricKind : int {
    KM_L2SQ = 0,  /* sum((x-q)^2)                     */
    KM_IP = 1,    /* -x.q (MO convention)             */
    KM_COS = 2,   /* 1 - x.q/(|x||q|), clamp, 0 -> 1  */
    KM_L1 = 3,    /* sum|x-q|                         */
};

inline int metric_kind(distance_type_t m) {
    switch (m) {
    case DistanceType_L2Expanded:
    case DistanceType_L2SqrtExpanded: return KM_L2SQ;
    case DistanceType_CosineExpanded: return KM_COS;
    case DistanceType_InnerProduct: return KM_IP;
    case DistanceType_L1: return KM_L1;
    default: throw std::runtime_error("unsupported metric");
    }
}

/* ------------------------------ scan variant ---------------------------- */

enum class ScanKind {
    F32,        /* scan_kernel<metric, qt>, qt in {8,4,2,1}                  */
    F32_ASM768, /* scan_asm768.hip: L2SQ, dpad 768, qt 16                    */
    HALF,       /* scan_h_kernel (f16/bf16 storage), qt 8                    */
    BYTE_DOT,   /* scan_i8_dot_kernel, qt 16 or 8; at qt 16 over an MFMA64
                   image scan_i8_mfma_kernel (same jobs, same results)       */
    BYTE_U4,    /* scan_i8_kernel (uchar4 form), qt 8                        */
};

struct ScanVariant {
    ScanKind kind;
    int qt; /* query-tile width: of the job table AND of the kernel */
};

inline const char* scan_kind_name(ScanKind k) {
    static const char* const names[] = {"F32", "F32_ASM768", "HALF",
                                        "BYTE_DOT", "BYTE_U4"};
    return names[(int)k];
}

/* A/B tuning overrides (environment, read once by the IVF-Flat library). */
struct ScanOverrides {
    bool generic_f32 = false; /* MOANN_SCAN=generic: no asm kernel        */
    bool byte_qt8 = false;    /* MOANN_BYTE_QT=8: no 16-wide byte tiles   */
    int chunk_g = 0;          /* MOANN_CHUNKG: list chunk groups, 0 = 8   */
    bool byte_mfma_off = false; /* MOANN_BYTE_MFMA=0: refine image stays in
                                   ROWS16, scanned by the dot kernel      */
    bool refine_tail_legacy = false; /* MOANN_REFINE_TAIL=legacy: radix
                                   select + four-kernel refine tail; an
                                   index starts from it
                                   (moann_ivf_flat_set_refine_tail)       */
};

struct ScanChoice { /* the list scan's and the centroid-rank scan's */
    ScanVariant list, rank;
};

/* f32 scan. Flagship shape (L2SQ, dpad 768): the hand-scheduled QT=16 asm
 * kernel — lowest tile re-read multiplicity AND a pipelined load ring.
 * Otherwise QT query rows in LDS; <= 52 KiB keeps >=3 blocks/CU resident.
 * QT=8 measured best end-to-end for the compiler-scheduled kernel: hipcc
 * pipelines its inner loop with counted vmcnt (4 loads in flight) where a
 * QT=16 instantiation degrades to a full vmcnt(0) stall per iteration; the
 * extra tile re-reads at QT=8 mostly hit the XCD-affine L2 (physical fetch
 * ~1.4x compulsory vs 1.14x at QT=16, but 4.6 vs 2.6 TB/s sustained). */
inline ScanVariant pick_f32_variant(int kmetric, int dpad, bool allow_asm) {
    if (allow_asm && kmetric == KM_L2SQ && dpad == 768)
        return {ScanKind::F32_ASM768, 16};
    for (int qt : {8, 4, 2})
        if ((size_t)qt * dpad * 4 + qt * 4 <= 52 * 1024)
            return {ScanKind::F32, qt};
    return {ScanKind::F32, 1};
}

/* `refine`: the two-stage scan is active (f32 storage whose first pass runs
 * over the internal byte image). `rownorms`: the scanned byte image has its
 * per-row norms (the refine image's when `refine`). */
inline ScanChoice pick_scan(int kmetric, int dpad, quantization_t storage,
                            bool refine, bool rownorms,
                            const ScanOverrides& ov) {
    const bool f32_st = storage == Quantization_F32;
    const bool half_st = storage == Quantization_F16 ||
                         storage == Quantization_BF16;
    const bool byte_scan = f32_st ? refine : !half_st;
    ScanChoice c;
    /* rank (f32 centroid scan) keeps its own tile width, sized for F32 query
     * tiles in LDS; it takes the asm kernel only where the list scan does */
    c.rank = pick_f32_variant(kmetric, dpad,
                              f32_st && !refine && !ov.generic_f32);
    if (byte_scan) {
        /* The byte list scan has exactly two tile widths: 16 (dot form
         * only) and 8 (dot form and uchar4 kernel). The dot form needs
         * 16-dim-aligned rows and the precomputed row norms; its wide tile
         * halves the query-tile re-read multiplicity (measured 1.14x
         * compulsory at QT=8). 8 byte rows of any supported dpad fit LDS
         * with room to spare — never the f32 rank width, which drops to 4
         * above dpad 1663. */
        if (dpad % 16 == 0 && rownorms) {
            const bool wide = (size_t)16 * dpad + 80 <= 48 * 1024 &&
                              !ov.byte_qt8;
            c.list = {ScanKind::BYTE_DOT, wide ? 16 : 8};
        } else {
            c.list = {ScanKind::BYTE_U4, 8};
        }
    } else if (half_st) {
        c.list = {ScanKind::HALF, 8};
    } else {
        c.list = c.rank;
    }
    return c;
}

/* Byte order inside a 64-row group of a dot-form byte image. The group
 * stride is 64*dpad bytes in both, so job tables do not depend on it; the
 * kernel that scans does. Only the internal refine image (built once, never
 * unpacked or saved) is ever MFMA64. */
enum class ByteImageLayout {
    ROWS16, /* [g][dpad/16][64][16]: scan_i8_dot_kernel                      */
    MFMA64, /* [g][dpad/64][4][64][16], lane l of unit (J, s) = row
               16s + (l&15), dims 64J + 16(l>>4)..: scan_i8_mfma_kernel      */
};

/* What scan_i8_mfma_kernel covers: the 16-wide dot-form variant, signed
 * bytes (the caller's concern), every metric but L1, whole 64-dim steps. */
inline bool byte_mfma_applies(int kmetric, ScanVariant list, int dpad) {
    return list.kind == ScanKind::BYTE_DOT && list.qt == 16 &&
           kmetric != KM_L1 && dpad % 64 == 0;
}

/* Layout of the refine image, decided once when it is built: `list` is the
 * variant pick_scan gives the refine scan of this index. */
inline ByteImageLayout pick_refine_layout(int kmetric, ScanVariant list,
                                          int dpad, const ScanOverrides& ov) {
    return byte_mfma_applies(kmetric, list, dpad) && !ov.byte_mfma_off
               ? ByteImageLayout::MFMA64
               : ByteImageLayout::ROWS16;
}

/* ---------------------------- host job tables --------------------------- */

/* SoA mirror of ScanJobs (moann_internal.h) in host memory; the planners
 * clear and refill it, so a warm pipeline allocates nothing. slot_base stays
 * empty for the rank scan (no membership filter). */
struct HostScanJobs {
    std::vector<int64_t> databaseg, qslot_outbase, slot_base;
    std::vector<int32_t> gstart, gcount, rows, nq, qbase, qslot_query;
    int njobs = 0, nqslots = 0;
    void clear() {
        for (auto* v : {&databaseg, &qslot_outbase, &slot_base}) v->clear();
        for (auto* v : {&gstart, &gcount, &rows, &nq, &qbase, &qslot_query})
            v->clear();
        njobs = nqslots = 0;
    }
};

/* Centroid rank: scan the centroid matrix (one "list" of nlist rows packed
 * into cent_groups groups) for every query. Tile queries by qt, chunk the
 * centroid groups to fill the chip; query q's distances land at q*nlist. */
inline void plan_rank_scan(uint64_t nq, int qt, uint32_t nlist,
                           int64_t cent_groups, HostScanJobs& out) {
    out.clear();
    const int ntiles = (int)((nq + qt - 1) / qt);
    /* target ~1024 jobs: enough to fill 256 CUs without paying the
     * 48 KiB query-tile LDS fill per tiny single-group job */
    const int64_t want_chunks = std::min<int64_t>(
        cent_groups, std::max<int64_t>(1, (1024 + ntiles - 1) / ntiles));
    const int chunk = (int)((cent_groups + want_chunks - 1) / want_chunks);
    const int nchunk = (int)((cent_groups + chunk - 1) / chunk);
    out.njobs = ntiles * nchunk;
    out.nqslots = ntiles * qt;
    for (int t = 0; t < ntiles; ++t) {
        const int q0 = t * qt;
        const int tn = (int)std::min<int64_t>(qt, (int64_t)nq - q0);
        for (int u = 0; u < qt; ++u) {
            const int qi = std::min<int>(q0 + u, (int)nq - 1);
            out.qslot_query.push_back(qi);
            out.qslot_outbase.push_back((int64_t)qi * nlist);
        }
        for (int c = 0; c < nchunk; ++c) { /* tile-outer, chunk-inner */
            out.databaseg.push_back(0);
            out.gstart.push_back((int32_t)(c * chunk));
            out.gcount.push_back(
                (int32_t)std::min<int64_t>(chunk, cent_groups - c * chunk));
            out.rows.push_back((int32_t)nlist);
            out.nq.push_back(tn);
            out.qbase.push_back(q0);
        }
    }
}

/* Where each (query, probe rank) pair's candidates live in the ragged
 * candidate buffer: query q owns [qoffs[q], qoffs[q+1]), and within it rank
 * r starts at probe_offs[q*(probe+1) + r]. A probe entry of -1 is empty. */
struct ProbeOffsets {
    std::vector<int64_t> probe_offs; /* [nq][probe+1] */
    std::vector<int64_t> qoffs;      /* [nq+1]        */
    int64_t total_cand = 0;
};

inline void plan_probe_offsets(const int32_t* h_probe, uint64_t nq,
                               uint32_t probe,
                               const std::vector<int32_t>& list_rows,
                               ProbeOffsets& out) {
    out.probe_offs.resize((size_t)nq * (probe + 1));
    out.qoffs.assign(nq + 1, 0);
    for (uint64_t q = 0; q < nq; ++q) {
        int64_t acc = 0;
        out.probe_offs[q * (probe + 1)] = 0;
        for (uint32_t r = 0; r < probe; ++r) {
            const int32_t l = h_probe[q * probe + r];
            if (l >= 0) acc += list_rows[l];
            out.probe_offs[q * (probe + 1) + r + 1] = acc;
        }
        out.qoffs[q + 1] = out.qoffs[q] + acc;
    }
    out.total_cand = out.qoffs[nq];
}

/* The list scan's job table plus the planner's per-list scratch (kept so a
 * reused plan allocates nothing). lcount is also what the perf counters
 * read: the (query, rank) pairs probing each non-empty list. */
struct ListScanPlan {
    HostScanJobs jobs;
    std::vector<int32_t> lcount, pair_q; /* [nlist] pairs per list; scratch */
    std::vector<int64_t> lbase, cursor, pair_ob; /* scratch */
};

/* List scan: group the (query, rank) pairs by list, then emit per list
 * query tiles of qt x group CHUNKS of chunk_g groups.
 * Chunking serves two ends at once:
 *  - tail balance: a job is <= ~3.5 MB of list data, so hub lists
 *    (many rows AND many query tiles) become many small jobs instead
 *    of one straggler workgroup;
 *  - L2 reuse: jobs are emitted lists ascending, then chunk-OUTER,
 *    tile-INNER, and the XCD-aware remap in the kernel gives each XCD a
 *    contiguous job range — so the ~96 co-resident jobs of an XCD are
 *    different query tiles over the SAME <=3.5 MB chunk (< 4 MB per-XCD
 *    L2), and the tile re-read multiplicity is served from L2, not HBM.
 * This job ORDER is part of the contract (scan_plan_check.cpp pins it). */
inline void plan_list_scan(const int32_t* h_probe, uint64_t nq,
                           uint32_t probe, int qt, int64_t chunk_g,
                           const std::vector<int32_t>& list_rows,
                           const std::vector<int64_t>& list_gbase,
                           const std::vector<int64_t>& list_slot_base,
                           const ProbeOffsets& offs, ListScanPlan& out) {
    const uint32_t nlist = (uint32_t)list_rows.size();
    /* group (query, rank) pairs by list */
    out.lcount.assign(nlist, 0);
    for (uint64_t q = 0; q < nq; ++q)
        for (uint32_t r = 0; r < probe; ++r) {
            const int32_t l = h_probe[q * probe + r];
            if (l >= 0 && list_rows[l] > 0) out.lcount[l]++;
        }
    out.lbase.assign(nlist + 1, 0);
    for (uint32_t l = 0; l < nlist; ++l)
        out.lbase[l + 1] = out.lbase[l] + out.lcount[l];
    const int64_t npairs = out.lbase[nlist];
    out.pair_q.resize(npairs);
    out.pair_ob.resize(npairs);
    out.cursor.assign(out.lbase.begin(), out.lbase.end() - 1);
    for (uint64_t q = 0; q < nq; ++q)
        for (uint32_t r = 0; r < probe; ++r) {
            const int32_t l = h_probe[q * probe + r];
            if (l < 0 || list_rows[l] == 0) continue;
            const int64_t pos = out.cursor[l]++;
            out.pair_q[pos] = (int32_t)q;
            out.pair_ob[pos] =
                offs.qoffs[q] + offs.probe_offs[q * (probe + 1) + r];
        }

    HostScanJobs& jb = out.jobs;
    jb.clear();
    for (uint32_t l = 0; l < nlist; ++l) {
        const int64_t n = out.lcount[l];
        if (!n) continue;
        const int64_t lg = (list_rows[l] + 63) / 64;
        const int64_t ntiles = (n + qt - 1) / qt;
        const int32_t qslot0 = (int32_t)jb.qslot_query.size();
        for (int64_t i = 0; i < ntiles * qt; ++i) {
            /* the last tile's pad lanes repeat its last pair */
            const int64_t pi = out.lbase[l] + std::min(i, n - 1);
            jb.qslot_query.push_back(out.pair_q[pi]);
            jb.qslot_outbase.push_back(out.pair_ob[pi]);
        }
        for (int64_t g0 = 0; g0 < lg; g0 += chunk_g)
            for (int64_t t = 0; t < ntiles; ++t) {
                jb.slot_base.push_back(list_slot_base[l]);
                jb.databaseg.push_back(list_gbase[l]);
                jb.gstart.push_back((int32_t)g0);
                jb.gcount.push_back(
                    (int32_t)std::min<int64_t>(chunk_g, lg - g0));
                jb.rows.push_back(list_rows[l]);
                jb.nq.push_back((int32_t)std::min<int64_t>(qt, n - t * qt));
                jb.qbase.push_back(qslot0 + (int32_t)(t * qt));
            }
    }
    jb.njobs = (int)jb.databaseg.size();
    jb.nqslots = (int)jb.qslot_query.size();
}

/* Groups per list-scan chunk. The target is BYTES (~1.5 MB: 8 groups of 64
 * f32 rows at dpad 768; measured best of {6,8,10,12,14,18,36} end-to-end),
 * so narrow storage, with more rows per byte, scales the group count. */
inline int64_t list_chunk_groups(quantization_t storage,
                                 const ScanOverrides& ov) {
    const bool half_st = storage == Quantization_F16 ||
                         storage == Quantization_BF16;
    return (int64_t)(ov.chunk_g > 0 ? ov.chunk_g : 8) *
           (storage == Quantization_F32 ? 1 : half_st ? 2 : 4);
}

}  // namespace moann

#endif
