/* CPU check of the scan planner (moann_scan_plan.h): builds plans for seeded
 * shapes at the tile / group / chunk edges and asserts the geometry the
 * scan kernels rely on, plus the variant table. Host compiler only, built
 * with ASan + UBSan by `make scan_plan_check`; run by tests/test_scan_plan.py.
 * Exit 0 and a one-line summary on success, first violated invariant on
 * stderr and exit 1 otherwise. */

#include "moann_scan_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

using namespace moann;

namespace {

char g_case[256] = "";

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "scan_plan_check: %s:%d: %s\n  case: %s\n",   \
                    __FILE__, __LINE__, #cond, g_case);                   \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

struct Rng { /* small LCG: the cases must not depend on the C library */
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

/* ------------------------------ list scan ------------------------------- */

struct Lists {
    std::vector<int32_t> rows;
    std::vector<int64_t> gbase, slot_base;
    explicit Lists(std::vector<int32_t> r) : rows(std::move(r)) {
        int64_t g = 0, s = 1000; /* nonzero base: catches base mix-ups */
        for (int32_t n : rows) {
            gbase.push_back(g);
            slot_base.push_back(s);
            g += (n + 63) / 64;
            s += n;
        }
    }
};

int64_t check_list_plan(const std::vector<int32_t>& h_probe, uint64_t nq,
                        uint32_t probe, int qt, int64_t chunk_g,
                        const Lists& L) {
    const uint32_t nlist = (uint32_t)L.rows.size();
    ProbeOffsets offs;
    ListScanPlan plan;
    plan_probe_offsets(h_probe.data(), nq, probe, L.rows, offs);
    plan_list_scan(h_probe.data(), nq, probe, qt, chunk_g, L.rows, L.gbase,
                   L.slot_base, offs, plan);
    const HostScanJobs& jb = plan.jobs;

    /* probe offsets against a straight restatement; expected pairs keyed by
     * their output base (distinct for pairs over non-empty lists) */
    CHECK(offs.qoffs.size() == nq + 1 && offs.qoffs[0] == 0);
    CHECK(offs.probe_offs.size() == (size_t)nq * (probe + 1));
    struct Pair { int32_t q, l; int64_t lanes; };
    std::map<int64_t, Pair> expect;
    std::vector<int32_t> want_lcount(nlist, 0);
    int64_t total = 0, want_lanes = 0;
    for (uint64_t q = 0; q < nq; ++q) {
        CHECK(offs.qoffs[q] == total);
        int64_t acc = 0;
        for (uint32_t r = 0; r < probe; ++r) {
            CHECK(offs.probe_offs[q * (probe + 1) + r] == acc);
            const int32_t l = h_probe[q * probe + r];
            if (l < 0 || L.rows[l] == 0) continue;
            CHECK(expect.emplace(total + acc, Pair {(int32_t)q, l, 0}).second);
            want_lcount[l]++;
            want_lanes += ((L.rows[l] + 63) / 64 + chunk_g - 1) / chunk_g;
            acc += L.rows[l];
        }
        CHECK(offs.probe_offs[q * (probe + 1) + probe] == acc);
        total += acc;
    }
    CHECK(offs.qoffs[nq] == total && offs.total_cand == total);
    CHECK(plan.lcount == want_lcount);

    /* table shape */
    const size_t nj = (size_t)jb.njobs, ns = (size_t)jb.nqslots;
    CHECK(jb.njobs >= 0 && jb.nqslots >= 0 && ns % qt == 0);
    CHECK(jb.databaseg.size() == nj && jb.slot_base.size() == nj);
    CHECK(jb.gstart.size() == nj && jb.gcount.size() == nj);
    CHECK(jb.rows.size() == nj && jb.nq.size() == nj);
    CHECK(jb.qbase.size() == nj);
    CHECK(jb.qslot_query.size() == ns && jb.qslot_outbase.size() == ns);

    std::map<int64_t, int32_t> list_of_gbase; /* non-empty lists only */
    for (uint32_t l = 0; l < nlist; ++l)
        if (L.rows[l] > 0) list_of_gbase[L.gbase[l]] = (int32_t)l;

    std::vector<std::pair<int64_t, int64_t>> ranges; /* written [lo, hi) */
    std::map<std::pair<int64_t, int64_t>, int> seen; /* (outbase, chunk) */
    int64_t lanes = 0;
    int32_t prev_l = -1, prev_g0 = -1, prev_qb = -1, next_qslot = 0;
    std::vector<int32_t> first_chunk_tiles; /* qbase order in chunk 0 */
    size_t tile_i = 0;
    for (size_t j = 0; j < nj; ++j) {
        /* the job's list, and that it describes that list */
        const auto it = list_of_gbase.find(jb.databaseg[j]);
        CHECK(it != list_of_gbase.end());
        const int32_t l = it->second;
        CHECK(jb.rows[j] == L.rows[l]);
        CHECK(jb.slot_base[j] == L.slot_base[l]);
        CHECK(plan.lcount[l] > 0);
        /* chunk geometry */
        const int64_t lg = (L.rows[l] + 63) / 64;
        const int32_t g0 = jb.gstart[j], gc = jb.gcount[j];
        CHECK(g0 >= 0 && g0 % chunk_g == 0 && g0 < lg);
        CHECK(gc == std::min<int64_t>(chunk_g, lg - g0));
        CHECK(gc >= 1 && (int64_t)g0 + gc <= lg);
        /* tile geometry */
        const int32_t qb = jb.qbase[j], tn = jb.nq[j];
        CHECK(qb >= 0 && qb % qt == 0 && (size_t)qb + qt <= ns);
        CHECK(tn >= 1 && tn <= qt);
        /* order: lists ascending, chunk-outer, tile-inner; every chunk of
         * a list walks the same tiles, and tiles take qslots in job order */
        if (l != prev_l) {
            CHECK(l > prev_l && g0 == 0);
            first_chunk_tiles.clear();
            tile_i = 0;
        } else if (g0 != prev_g0) {
            CHECK(g0 == prev_g0 + chunk_g);
            CHECK(tile_i == first_chunk_tiles.size());
            tile_i = 0;
        } else {
            CHECK(qb > prev_qb);
        }
        if (g0 == 0) {
            CHECK(qb == next_qslot);
            next_qslot += qt;
            first_chunk_tiles.push_back(qb);
        } else {
            CHECK(tile_i < first_chunk_tiles.size());
            CHECK(first_chunk_tiles[tile_i] == qb);
        }
        ++tile_i;
        prev_l = l, prev_g0 = g0, prev_qb = qb;
        /* lanes */
        for (int u = 0; u < qt; ++u) {
            const int32_t q = jb.qslot_query[qb + u];
            const int64_t ob = jb.qslot_outbase[qb + u];
            if (u >= tn) { /* padding repeats the tile's last pair */
                CHECK(q == jb.qslot_query[qb + tn - 1]);
                CHECK(ob == jb.qslot_outbase[qb + tn - 1]);
                continue;
            }
            const auto e = expect.find(ob);
            CHECK(e != expect.end());
            CHECK(e->second.q == q && e->second.l == l);
            const std::pair<int64_t, int64_t> in_chunk(ob, g0 / chunk_g);
            CHECK(seen[in_chunk]++ == 0);
            e->second.lanes++;
            ++lanes;
            const int64_t lo = ob + (int64_t)g0 * 64;
            const int64_t hi =
                ob + std::min<int64_t>(L.rows[l], ((int64_t)g0 + gc) * 64);
            CHECK(lo < hi);
            ranges.push_back({lo, hi});
        }
    }
    CHECK((size_t)next_qslot == ns);
    /* every pair once in EACH chunk of its list, nothing else */
    CHECK(lanes == want_lanes);
    for (const auto& e : expect) {
        const int64_t lg = (L.rows[e.second.l] + 63) / 64;
        CHECK(e.second.lanes == (lg + chunk_g - 1) / chunk_g);
    }
    /* written ranges are disjoint and their union is [0, total_cand) */
    std::sort(ranges.begin(), ranges.end());
    int64_t at = 0;
    for (const auto& r : ranges) {
        CHECK(r.first == at);
        at = r.second;
    }
    CHECK(at == total);
    return (int64_t)nj;
}

/* probe table: `probe` distinct lists per query in random order, `hub`
 * (if >= 0) first for every query, about one entry in `holes` set to -1 */
std::vector<int32_t> make_probe(Rng& rng, uint64_t nq, uint32_t probe,
                                uint32_t nlist, int32_t hub, uint32_t holes) {
    std::vector<int32_t> out, perm(nlist);
    for (uint64_t q = 0; q < nq; ++q) {
        for (uint32_t l = 0; l < nlist; ++l) perm[l] = (int32_t)l;
        for (uint32_t i = nlist - 1; i > 0; --i)
            std::swap(perm[i], perm[rng.below(i + 1)]);
        if (hub >= 0)
            std::swap(perm[0], *std::find(perm.begin(), perm.end(), hub));
        for (uint32_t r = 0; r < probe; ++r) {
            const bool hole = holes && !(hub >= 0 && r == 0) &&
                              rng.below(holes) == 0;
            out.push_back(hole ? -1 : perm[r]);
        }
    }
    return out;
}

int64_t check_list_cases() {
    Rng rng {0x5ca9u};
    int64_t cases = 0, jobs = 0;
    for (int qt : {1, 2, 4, 8, 16})
        for (int64_t chunk_g : {1, 8, 32}) {
            /* group edges, empty lists, one list past a chunk boundary */
            const int32_t longl = (int32_t)(chunk_g * 64 + 1);
            const Lists L({0, 1, 63, 64, 65, longl, 0, 130});
            const uint32_t nlist = (uint32_t)L.rows.size();
            for (int nq : {1, qt - 1, qt, qt + 1, 33}) {
                if (nq < 1) continue;
                struct { uint32_t probe; int32_t hub; uint32_t holes; }
                kinds[] = {
                    {3, -1, 5},    /* sparse probe with -1 entries      */
                    {2, 5, 0},     /* hub: every query probes the long list */
                    {nlist, -1, 0}, /* probe == nlist                   */
                    {nlist, 5, 4}, /* all of the above                  */
                    {1, 0, 0},     /* only an empty list: no jobs       */
                };
                for (const auto& k : kinds) {
                    snprintf(g_case, sizeof g_case,
                             "list scan qt=%d chunk_g=%d nq=%d probe=%u "
                             "hub=%d holes=%u", qt, (int)chunk_g, nq,
                             k.probe, k.hub, k.holes);
                    const auto pr = make_probe(rng, nq, k.probe, nlist,
                                               k.hub, k.holes);
                    const int64_t nj =
                        check_list_plan(pr, nq, k.probe, qt, chunk_g, L);
                    if (k.probe == 1) CHECK(nj == 0);
                    jobs += nj;
                    ++cases;
                }
            }
        }
    CHECK(jobs > 0);
    return cases;
}

/* ------------------------------ rank scan ------------------------------- */

int64_t check_rank_cases() {
    int64_t cases = 0;
    HostScanJobs jb; /* reused across cases, like the search contexts do */
    for (int qt : {1, 2, 4, 8, 16})
        for (int nq : {1, qt - 1, qt, qt + 1, 33, 3000})
            for (uint32_t nlist : {1u, 63u, 64u, 65u, 1000u, 70000u}) {
                if (nq < 1) continue;
                snprintf(g_case, sizeof g_case, "rank scan qt=%d nq=%d "
                         "nlist=%u", qt, nq, nlist);
                const int64_t cg = (nlist + 63) / 64;
                plan_rank_scan((uint64_t)nq, qt, nlist, cg, jb);
                const size_t nj = (size_t)jb.njobs, ns = (size_t)jb.nqslots;
                CHECK(jb.njobs > 0 && ns == (size_t)((nq + qt - 1) / qt) * qt);
                CHECK(jb.databaseg.size() == nj && jb.slot_base.empty());
                CHECK(jb.gstart.size() == nj && jb.gcount.size() == nj);
                CHECK(jb.rows.size() == nj && jb.nq.size() == nj);
                CHECK(jb.qbase.size() == nj);
                CHECK(jb.qslot_query.size() == ns);
                CHECK(jb.qslot_outbase.size() == ns);
                /* every (query, centroid group) covered exactly once */
                std::vector<uint8_t> cover((size_t)nq * cg, 0);
                for (size_t j = 0; j < nj; ++j) {
                    CHECK(jb.databaseg[j] == 0);
                    CHECK(jb.rows[j] == (int32_t)nlist);
                    const int32_t g0 = jb.gstart[j], gc = jb.gcount[j];
                    CHECK(g0 >= 0 && gc >= 1 && (int64_t)g0 + gc <= cg);
                    const int32_t qb = jb.qbase[j], tn = jb.nq[j];
                    CHECK(qb >= 0 && qb % qt == 0 && (size_t)qb + qt <= ns);
                    CHECK(tn >= 1 && tn <= qt);
                    for (int u = 0; u < qt; ++u) {
                        const int32_t q = jb.qslot_query[qb + u];
                        CHECK(q == std::min(qb + u, qb + tn - 1) && q < nq);
                        CHECK(jb.qslot_outbase[qb + u] == (int64_t)q * nlist);
                        if (u >= tn) continue;
                        for (int32_t g = g0; g < g0 + gc; ++g)
                            CHECK(cover[(size_t)q * cg + g]++ == 0);
                    }
                }
                for (uint8_t c : cover) CHECK(c == 1);
                ++cases;
            }
    return cases;
}

/* ----------------------------- variant table ---------------------------- */

size_t f32_lds(int qt, int dpad) { return (size_t)qt * dpad * 4 + qt * 4; }

void check_f32(ScanVariant v, int km, int dpad, bool asm_allowed) {
    if (v.kind == ScanKind::F32_ASM768) {
        CHECK(asm_allowed && km == KM_L2SQ && dpad == 768 && v.qt == 16);
    } else {
        CHECK(v.kind == ScanKind::F32);
        CHECK(!(asm_allowed && km == KM_L2SQ && dpad == 768));
        CHECK(v.qt == 8 || v.qt == 4 || v.qt == 2 || v.qt == 1);
        /* the widest width that fits */
        CHECK(v.qt == 8 || f32_lds(v.qt * 2, dpad) > 52 * 1024);
    }
    CHECK(f32_lds(v.qt, dpad) <= 52 * 1024);
}

int64_t check_variant_table() {
    const distance_type_t metrics[] = {
        DistanceType_L2Expanded, DistanceType_L2SqrtExpanded,
        DistanceType_CosineExpanded, DistanceType_L1,
        DistanceType_InnerProduct};
    const quantization_t storages[] = {
        Quantization_F32, Quantization_F16, Quantization_INT8,
        Quantization_UINT8, Quantization_BF16};
    /* 20/100/772: dpads that are no multiple of 16 (the uchar4 form) */
    const int dpads[] = {16, 48, 64, 768, 1648, 1664, 3056, 3072, 3088,
                         20, 100, 772};
    int64_t cases = 0;
    for (distance_type_t m : metrics)
        for (quantization_t st : storages)
            for (int dpad : dpads)
                for (int bits = 0; bits < 16; ++bits) {
                    const bool refine = bits & 1, norms = bits & 2;
                    ScanOverrides ov;
                    ov.generic_f32 = bits & 4;
                    ov.byte_qt8 = bits & 8;
                    snprintf(g_case, sizeof g_case, "variant metric=%d "
                             "storage=%d dpad=%d refine=%d norms=%d "
                             "generic=%d byte_qt8=%d", (int)m, (int)st, dpad,
                             refine, norms, ov.generic_f32, ov.byte_qt8);
                    const int km = metric_kind(m);
                    const ScanChoice c =
                        pick_scan(km, dpad, st, refine, norms, ov);
                    const bool f32 = st == Quantization_F32;
                    const bool half = st == Quantization_F16 ||
                                      st == Quantization_BF16;
                    const bool asm_ok = f32 && !refine && !ov.generic_f32;
                    /* rank: always the f32 scan of the centroids */
                    check_f32(c.rank, km, dpad, asm_ok);
                    const ScanVariant v = c.list;
                    if (f32 && !refine) {
                        CHECK(v.kind == c.rank.kind && v.qt == c.rank.qt);
                    } else if (half) {
                        CHECK(v.kind == ScanKind::HALF && v.qt == 8);
                        CHECK((size_t)8 * dpad * 2 + 48 <= 64 * 1024);
                    } else { /* byte kernels: storage or refine image */
                        const bool dot = dpad % 16 == 0 && norms;
                        CHECK(v.kind == (dot ? ScanKind::BYTE_DOT
                                             : ScanKind::BYTE_U4));
                        const bool wide = dot && !ov.byte_qt8 &&
                                          (size_t)16 * dpad + 80 <= 48 * 1024;
                        CHECK(v.qt == (wide ? 16 : 8));
                        CHECK((size_t)v.qt * dpad + v.qt * 4 + 16 <=
                              (v.qt == 16 ? 48 : 64) * 1024);
                    }
                    /* stated independently of the branches above */
                    if (v.kind == ScanKind::BYTE_DOT ||
                        v.kind == ScanKind::BYTE_U4)
                        CHECK(v.qt == 8 || v.qt == 16);
                    if (v.kind == ScanKind::BYTE_DOT) CHECK(dpad % 16 == 0);
                    if (v.kind == ScanKind::BYTE_U4) CHECK(v.qt == 8);
                    if (v.kind == ScanKind::F32_ASM768)
                        CHECK(km == KM_L2SQ && dpad == 768 && f32 &&
                              !refine && !ov.generic_f32);
                    ++cases;
                }
    /* today's choices, pinned */
    const ScanOverrides none;
    ScanOverrides generic, bq8;
    generic.generic_f32 = true;
    bq8.byte_qt8 = true;
    auto list = [](int km, int dpad, quantization_t st, bool refine,
                   bool norms, const ScanOverrides& ov) {
        return pick_scan(km, dpad, st, refine, norms, ov).list;
    };
    auto is = [](ScanVariant v, ScanKind k, int qt) {
        return v.kind == k && v.qt == qt;
    };
    snprintf(g_case, sizeof g_case, "pinned variants");
    const auto F = Quantization_F32, I8 = Quantization_INT8;
    CHECK(is(list(KM_L2SQ, 768, F, false, false, none),
             ScanKind::F32_ASM768, 16));
    CHECK(is(list(KM_L2SQ, 768, F, false, false, generic), ScanKind::F32, 8));
    CHECK(is(list(KM_IP, 768, F, false, false, none), ScanKind::F32, 8));
    CHECK(is(list(KM_L2SQ, 1648, F, false, false, none), ScanKind::F32, 8));
    CHECK(is(list(KM_L2SQ, 1664, F, false, false, none), ScanKind::F32, 4));
    CHECK(is(list(KM_L2SQ, 3088, F, false, false, none), ScanKind::F32, 4));
    CHECK(is(list(KM_L2SQ, 768, Quantization_F16, false, false, none),
             ScanKind::HALF, 8));
    CHECK(is(list(KM_L2SQ, 768, I8, false, true, none),
             ScanKind::BYTE_DOT, 16));
    CHECK(is(list(KM_L2SQ, 768, I8, false, true, bq8),
             ScanKind::BYTE_DOT, 8));
    CHECK(is(list(KM_L2SQ, 3056, I8, false, true, none),
             ScanKind::BYTE_DOT, 16));
    CHECK(is(list(KM_L2SQ, 3072, I8, false, true, none),
             ScanKind::BYTE_DOT, 8));
    CHECK(is(list(KM_L2SQ, 768, I8, false, false, none),
             ScanKind::BYTE_U4, 8));
    CHECK(is(list(KM_L2SQ, 772, I8, false, true, none),
             ScanKind::BYTE_U4, 8));
    /* refine: byte list scan, rank stays the generic f32 scan; a byte scan
     * never inherits the rank width (4 above dpad 1663) */
    const ScanChoice r = pick_scan(KM_L2SQ, 768, F, true, true, none);
    CHECK(is(r.list, ScanKind::BYTE_DOT, 16) && is(r.rank, ScanKind::F32, 8));
    const ScanChoice w = pick_scan(KM_L2SQ, 1664, F, true, true, none);
    CHECK(is(w.list, ScanKind::BYTE_DOT, 16) && is(w.rank, ScanKind::F32, 4));
    /* chunk groups scale with the storage width */
    ScanOverrides cg;
    cg.chunk_g = 6;
    CHECK(list_chunk_groups(F, none) == 8 && list_chunk_groups(F, cg) == 6);
    CHECK(list_chunk_groups(Quantization_BF16, none) == 16);
    CHECK(list_chunk_groups(I8, none) == 32);
    return cases + 1;
}

}  // namespace

int main() {
    const int64_t nl = check_list_cases();
    const int64_t nr = check_rank_cases();
    const int64_t nv = check_variant_table();
    printf("scan_plan_check OK: %lld list-scan plans, %lld rank plans, "
           "%lld variant rows\n", (long long)nl, (long long)nr,
           (long long)nv);
    return 0;
}
