/* CPU check of the brute-force planner (moann_bf_plan.h): slices, query
 * batches, buffer sizes and the capacity rule at their edges. Host compiler
 * only, built with ASan + UBSan by `make bf_plan_check`; run by
 * tests/test_bf_plan.py. Exit 0 and a one-line summary on success, first
 * violated invariant on stderr and exit 1 otherwise. */

#include "moann_bf_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace moann;

namespace {

char g_case[256] = "";
int g_checks = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            fprintf(stderr, "bf_plan_check: %s:%d: %s\n  case: %s\n",      \
                    __FILE__, __LINE__, #cond, g_case);                    \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

template <typename F>
bool refuses(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

/* every invariant of one plan */
BfPlan check_plan(int64_t n, int64_t nq, int64_t k, int mode,
                  int64_t slice_rows, int cus) {
    snprintf(g_case, sizeof g_case,
             "n=%lld nq=%lld k=%lld mode=%d slice_rows=%lld cus=%d",
             (long long)n, (long long)nq, (long long)k, mode,
             (long long)slice_rows, cus);
    const BfPlan p = bf_plan(n, nq, k, mode, slice_rows, cus);
    CHECK(p.mode == BF_FUSED || p.mode == BF_GEMM);
    if (mode != BF_AUTO) CHECK(p.mode == mode);
    if (mode == BF_AUTO) {
        CHECK(p.mode == bf_auto_mode(n, nq, k));
        if (k > BF_FUSED_KMAX || n < BF_AUTO_MIN_ROWS) CHECK(p.mode == BF_GEMM);
    }
    if (p.mode == BF_FUSED) CHECK(k <= BF_FUSED_KMAX);

    /* tiles and slices: whole tiles, every row once, no slice empty */
    CHECK(p.tiles == (n + BF_TILE - 1) / BF_TILE);
    CHECK(p.tiles_per_slice >= 1 && p.tiles_per_slice <= p.tiles);
    CHECK(p.slice_rows == p.tiles_per_slice * BF_TILE);
    CHECK(p.slices >= 1);
    CHECK((p.slices - 1) * p.tiles_per_slice < p.tiles); /* last not empty */
    CHECK(p.slices * p.tiles_per_slice >= p.tiles);      /* all covered    */
    if (slice_rows) CHECK(p.slice_rows == slice_rows || p.slices == 1);
    {
        /* walk the slices (sampled when there are many): contiguous cover */
        const int64_t step = p.slices > 4096 ? p.slices / 1021 : 1;
        int64_t lo, hi;
        bf_slice_range(p, n, 0, &lo, &hi);
        CHECK(lo == 0);
        for (int64_t s = 0; s < p.slices; s += step) {
            bf_slice_range(p, n, s, &lo, &hi);
            CHECK(lo < hi && hi <= n);
            CHECK(lo == s * p.slice_rows);
            if (s + 1 < p.slices) {
                int64_t lo2, hi2;
                bf_slice_range(p, n, s + 1, &lo2, &hi2);
                CHECK(lo2 == hi);
            }
        }
        bf_slice_range(p, n, p.slices - 1, &lo, &hi);
        CHECK(hi == n);
    }

    /* query batches */
    CHECK(p.q_batch >= 1 && p.q_batch <= nq && p.q_batch <= BF_QBATCH_MAX);
    CHECK(p.passes == (nq + p.q_batch - 1) / p.q_batch);
    CHECK(p.query_blocks == (p.q_batch + BF_QTILE - 1) / BF_QTILE);
    CHECK(p.query_blocks * p.slices < ((int64_t)1 << 31)); /* fused grid */

    /* sizes: what launch_topk indexes with int32, what is allocated */
    CHECK(p.slices * k < ((int64_t)1 << 31));
    CHECK(p.cand_entries == p.q_batch * p.slices * k);
    CHECK(p.cand_entries > 0 && p.cand_entries * 8 <= BF_CAND_CAP);
    if (p.mode == BF_GEMM) {
        const int64_t chunk = p.slice_rows < n ? p.slice_rows : n;
        CHECK(p.dmat_entries == p.q_batch * chunk);
        /* one tile per chunk is the floor, taken only without an override */
        CHECK(p.dmat_entries * 4 <= BF_DMAT_CAP ||
              (!slice_rows && p.tiles_per_slice == 1));
        CHECK(chunk < ((int64_t)1 << 31));
    } else {
        CHECK(p.dmat_entries == 0);
    }

    /* the planner's own slice count: about two blocks per CU */
    if (p.mode == BF_FUSED && !slice_rows) {
        int64_t want = 2 * (int64_t)(cus < 1 ? 1 : cus) / p.query_blocks;
        if (want < 1) want = 1;
        CHECK(p.slices <= want);
        if (p.tiles >= want) CHECK(2 * p.slices > want); /* ceil/ceil rule */
    }
    return p;
}

bool same_plan(const BfPlan& a, const BfPlan& b) {
    return a.mode == b.mode && a.q_batch == b.q_batch &&
           a.passes == b.passes && a.query_blocks == b.query_blocks &&
           a.tiles == b.tiles && a.tiles_per_slice == b.tiles_per_slice &&
           a.slice_rows == b.slice_rows && a.slices == b.slices &&
           a.cand_entries == b.cand_entries &&
           a.dmat_entries == b.dmat_entries && a.wide_bytes == b.wide_bytes;
}

/* The plan over a narrow store whose gemm slices are widened to f32 rows of
 * `wide` bytes, against the plan `base` of the same search over f32 rows
 * (made by check_plan, which has checked every older invariant of it).
 * Returns false where the planner refuses, which it may only where even one
 * query's candidates of the capped slices do not fit. */
bool check_wide_plan(const BfPlan& base, int64_t n, int64_t nq, int64_t k,
                     int mode, int cus, int64_t wide) {
    snprintf(g_case, sizeof g_case,
             "n=%lld nq=%lld k=%lld mode=%d cus=%d wide=%lld", (long long)n,
             (long long)nq, (long long)k, mode, cus, (long long)wide);
    /* wide = 0 is the old plan, field by field, also when passed explicitly */
    CHECK(same_plan(bf_plan(n, nq, k, mode, 0, cus, 0), base));
    CHECK(base.wide_bytes == 0);
    /* auto over a narrow store has a pair bound of its own */
    const int want_mode =
        mode == BF_AUTO ? bf_auto_mode(n, nq, k, true) : mode;
    if (mode == BF_AUTO && base.mode == BF_FUSED) CHECK(want_mode == BF_FUSED);
    const int64_t wt = bf_wide_tiles(wide);
    CHECK(wt >= 1 && (wt == 1 || wt * BF_TILE * wide <= BF_WIDE_CAP));
    BfPlan p;
    try {
        p = bf_plan(n, nq, k, mode, 0, cus, wide); /* returns: terminates */
    } catch (const std::invalid_argument&) {
        const int64_t tiles = (n + BF_TILE - 1) / BF_TILE;
        const int64_t S = (tiles + wt - 1) / wt;
        CHECK(want_mode == BF_GEMM);
        CHECK(S * k * 8 > BF_CAND_CAP || S * k >= ((int64_t)1 << 31));
        return false;
    }
    CHECK(p.mode == want_mode && p.tiles == base.tiles);
    if (p.mode == BF_FUSED) { /* nothing is widened: the f32 store's plan */
        CHECK(same_plan(p, bf_plan(n, nq, k, BF_FUSED, 0, cus)));
        return true;
    }
    CHECK(p.tiles_per_slice >= 1 && p.tiles_per_slice <= p.tiles);
    CHECK(p.slice_rows == p.tiles_per_slice * BF_TILE);
    CHECK((p.slices - 1) * p.tiles_per_slice < p.tiles);
    CHECK(p.slices * p.tiles_per_slice >= p.tiles);
    const int64_t chunk = p.slice_rows < n ? p.slice_rows : n;
    CHECK(p.wide_bytes == chunk * wide);
    CHECK(p.wide_bytes <= BF_WIDE_CAP || p.tiles_per_slice == 1);
    CHECK(p.q_batch >= 1 && p.q_batch <= nq);
    CHECK(p.passes == (nq + p.q_batch - 1) / p.q_batch);
    CHECK(p.slices * k < ((int64_t)1 << 31));
    CHECK(p.cand_entries == p.q_batch * p.slices * k);
    CHECK(p.cand_entries * 8 <= BF_CAND_CAP);
    CHECK(p.dmat_entries == p.q_batch * chunk);
    CHECK(p.dmat_entries * 4 <= BF_DMAT_CAP || p.tiles_per_slice == 1);
    /* a cap that does not bind changes nothing */
    if (base.mode == BF_GEMM && base.tiles_per_slice <= wt)
        CHECK(same_plan(p, [&] {
        BfPlan b = base;
        b.wide_bytes = chunk * wide;
        return b;
    }()));
    return true;
}

}  // namespace

int main() {
    const int modes[] = {BF_AUTO, BF_FUSED, BF_GEMM};
    const int64_t ns[] = {1,    2,    127,     128,      129,       255,
                          256,  257,  300,     10000,    1000000,   10000000,
                          ((int64_t)1 << 31) - 1};
    const int64_t nqs[] = {1, 16, 127, 128, 129, 257, 1024, 100000, 5000000};
    const int64_t ks[] = {1, 10, 63, 64, 65, 1000, 4096};
    const int cuss[] = {1, 8, 256, 304};
    int64_t wide_plans = 0;
    for (int mode : modes)
        for (int64_t n : ns)
            for (int64_t nq : nqs)
                for (int64_t k : ks)
                    for (int cus : cuss) {
                        if (mode == BF_FUSED && k > BF_FUSED_KMAX) continue;
                        const BfPlan base = check_plan(n, nq, k, mode, 0, cus);
                        /* f16 store: dpad4 * 4 bytes per widened row, at dim
                         * 1, 8, 768, 4096, and a row longer than the cap */
                        for (int64_t wide : {(int64_t)4, (int64_t)32,
                                             (int64_t)3072, (int64_t)16384,
                                             BF_WIDE_CAP / 64})
                            wide_plans +=
                                check_wide_plan(base, n, nq, k, mode, cus, wide);
                    }
    CHECK(wide_plans > 0);

    /* k > n plans like any other k: padding is the kernels' business */
    check_plan(3, 5, 10, BF_FUSED, 0, 256);
    check_plan(3, 5, 10, BF_GEMM, 0, 256);

    /* overrides: one tile per slice, uneven last slice */
    for (int mode : {BF_FUSED, BF_GEMM}) {
        BfPlan p = check_plan(300, 7, 10, mode, 128, 256);
        CHECK(p.slices == 3 && p.tiles_per_slice == 1);
        int64_t lo, hi;
        bf_slice_range(p, 300, 2, &lo, &hi);
        CHECK(lo == 256 && hi == 300);
        p = check_plan(300, 7, 10, mode, 256, 256);
        CHECK(p.slices == 2);
        p = check_plan(300, 7, 10, mode, 1024, 256); /* longer than n */
        CHECK(p.slices == 1);
        check_plan(1000000, 1024, 10, mode, 128, 256);
        check_plan(1000000, 1024, 10, mode, 65536, 256);
    }

    /* widened tile: 1M x 768 in gemm mode is cut at 682 tiles (87 296 rows of
     * 3072 bytes, 255.75 MiB); an override past that is refused, one inside
     * it is kept; the fused mode ignores the figure */
    {
        snprintf(g_case, sizeof g_case, "wide tile");
        CHECK(bf_wide_tiles(3072) == 682);
        const BfPlan p = bf_plan(1000000, 16, 10, BF_GEMM, 0, 256, 3072);
        CHECK(p.tiles_per_slice == 682 && p.slices == 12);
        CHECK(p.wide_bytes == 682 * 128 * 3072);
        CHECK(refuses([] {
            bf_plan(1000000, 16, 10, BF_GEMM, 683 * 128, 256, 3072);
        }));
        CHECK(bf_plan(1000000, 16, 10, BF_GEMM, 682 * 128, 256, 3072)
                  .slices == 12);
        CHECK(bf_plan(300, 16, 10, BF_GEMM, 1024, 256, 3072).slices == 1);
        CHECK(bf_plan(1000000, 16, 10, BF_FUSED, 683 * 128, 256, 3072)
                  .slice_rows == 683 * 128);
        CHECK(refuses([] { bf_plan(300, 1, 10, BF_GEMM, 0, 256, -4); }));
    }

    /* the flagship shape: 1M rows, 1024 queries, 256 CUs -> 8 query blocks,
     * 64 slices of 123 tiles (the last one shorter) */
    {
        const BfPlan p = check_plan(1000000, 1024, 10, BF_AUTO, 0, 256);
        CHECK(p.mode == BF_FUSED && p.query_blocks == 8 && p.passes == 1);
        CHECK(p.tiles == 7813 && p.tiles_per_slice == 123 && p.slices == 64);
    }
    /* auto at the measured shapes (profiles/r05_README.md) */
    snprintf(g_case, sizeof g_case, "auto rule");
    for (int64_t nq : {4, 8, 16, 128, 1024})
        CHECK(bf_auto_mode(1000000, nq, 10) == BF_FUSED);
    CHECK(bf_auto_mode(1000000, 1024, 64) == BF_FUSED);
    CHECK(bf_auto_mode(1000000, 1024, 65) == BF_GEMM);
    CHECK(bf_auto_mode(100000, 128, 10) == BF_FUSED);
    CHECK(bf_auto_mode(100000, 1024, 10) == BF_FUSED);
    CHECK(bf_auto_mode(30000, 1024, 10) == BF_FUSED);
    CHECK(bf_auto_mode(10000, 1024, 10) == BF_GEMM);
    CHECK(bf_auto_mode(100000, 16, 10) == BF_GEMM);
    CHECK(bf_auto_mode(1000000, 1, 10) == BF_GEMM);
    CHECK(bf_auto_mode(BF_MAX_ROWS, (int64_t)1 << 40, 10) == BF_FUSED);
    /* auto over an f16 store at the measured shapes (profiles/r06_README.md) */
    for (int64_t nq : {1, 16, 128, 1024})
        CHECK(bf_auto_mode(1000000, nq, 10, true) == BF_FUSED);
    CHECK(bf_auto_mode(1000000, 1024, 64, true) == BF_FUSED);
    CHECK(bf_auto_mode(1000000, 1024, 65, true) == BF_GEMM);
    for (int64_t nq : {16, 128, 1024})
        CHECK(bf_auto_mode(100000, nq, 10, true) == BF_FUSED);
    CHECK(bf_auto_mode(30000, 1024, 10, true) == BF_FUSED);
    CHECK(bf_auto_mode(10000, 1024, 10, true) == BF_GEMM);
    CHECK(bf_auto_mode(100000, 9, 10, true) == BF_GEMM);
    CHECK(bf_plan(1000000, 1, 10, BF_AUTO, 0, 256, 3072).mode == BF_FUSED);
    CHECK(bf_plan(1000000, 1, 10, BF_AUTO, 0, 256).mode == BF_GEMM);

    /* one query still spreads over the device */
    {
        const BfPlan p = check_plan(1000000, 1, 10, BF_FUSED, 0, 256);
        CHECK(p.slices > 256 && p.slices <= 512);
    }

    /* refusals */
    snprintf(g_case, sizeof g_case, "refusals");
    CHECK(refuses([] { bf_plan(300, 1, 10, BF_AUTO, 100, 256); }));
    CHECK(refuses([] { bf_plan(300, 1, 10, BF_AUTO, 129, 256); }));
    CHECK(refuses([] { bf_plan(300, 1, 10, BF_AUTO, -128, 256); }));
    CHECK(refuses([] { bf_plan(0, 1, 10, BF_AUTO, 0, 256); }));
    CHECK(refuses([] { bf_plan((int64_t)1 << 31, 1, 10, BF_AUTO, 0, 256); }));
    CHECK(refuses([] { bf_plan(300, 0, 10, BF_AUTO, 0, 256); }));
    CHECK(refuses([] { bf_plan(300, 1, 0, BF_AUTO, 0, 256); }));
    CHECK(refuses([] { bf_plan(300, 1, 4097, BF_AUTO, 0, 256); }));
    CHECK(refuses([] { bf_plan(300, 1, 65, BF_FUSED, 0, 256); }));
    CHECK(refuses([] { bf_plan(300, 1, 10, 3, 0, 256); }));
    /* 2^24 one-tile slices of k = 4096 candidates: past int32 and the cap */
    CHECK(refuses([] {
        bf_plan(((int64_t)1 << 31) - 1, 1, 4096, BF_GEMM, 128, 256);
    }));

    /* capacity: unchanged while rows fit, doubling, the 2^31-1 ceiling */
    CHECK(bf_next_capacity(0, 0, 1) == 64);
    CHECK(bf_next_capacity(0, 0, 100) == 128);
    CHECK(bf_next_capacity(128, 100, 28) == 128);
    CHECK(bf_next_capacity(128, 100, 29) == 256);
    CHECK(bf_next_capacity(128, 100, 200) == 512);
    CHECK(bf_next_capacity(1000, 1000, 1) == 2000);
    CHECK(bf_next_capacity(0, 0, BF_MAX_ROWS) == BF_MAX_ROWS);
    CHECK(bf_next_capacity((int64_t)1 << 30, (int64_t)1 << 30, 1) ==
          BF_MAX_ROWS);
    CHECK(bf_next_capacity(BF_MAX_ROWS, BF_MAX_ROWS - 1, 1) == BF_MAX_ROWS);
    CHECK(refuses([] { bf_next_capacity(BF_MAX_ROWS, BF_MAX_ROWS, 1); }));
    CHECK(refuses([] { bf_next_capacity(0, 0, (int64_t)1 << 31); }));
    CHECK(refuses([] { bf_next_capacity(128, 100, BF_MAX_ROWS - 99); }));
    CHECK(refuses([] { bf_next_capacity(128, -1, 1); }));

    printf("bf_plan_check OK: %d checks\n", g_checks);
    return 0;
}
