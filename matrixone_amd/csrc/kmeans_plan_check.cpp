/* CPU check of the k-means build rules (moann_kmeans_plan.h): the sample,
 * init, reseed and stop rules at their edges. Host compiler only, built with
 * ASan + UBSan by `make kmeans_plan_check`; run by tests/test_kmeans_plan.py.
 * Exit 0 and a one-line summary on success, first violated invariant on
 * stderr and exit 1 otherwise. */

#include "moann_kmeans_plan.h"

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
            fprintf(stderr, "kmeans_plan_check: %s:%d: %s\n  case: %s\n",  \
                    __FILE__, __LINE__, #cond, g_case);                    \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

/* sample + init invariants for one (n, nlist, fraction, cap) */
void check_sample(uint64_t n, uint32_t nlist, double fraction, uint64_t cap,
                  uint64_t want_n_train) {
    snprintf(g_case, sizeof g_case, "n=%llu nlist=%u fraction=%g cap=%llu",
             (unsigned long long)n, nlist, fraction, (unsigned long long)cap);
    const uint64_t nt = kmeans_n_train(n, nlist, fraction, cap);
    CHECK(nt == want_n_train);
    CHECK(nt >= nlist && nt <= n);
    /* training rows: first is 0, strictly increasing, inside [0, n) */
    uint64_t prev = 0;
    const uint64_t step = nt > 4096 ? nt / 1021 : 1; /* sample big cases */
    for (uint64_t i = 0; i < nt; i += step) {
        const uint64_t r = kmeans_train_row(i, n, nt);
        CHECK(r < n);
        CHECK(r >= i); /* n >= n_train */
        if (i == 0) CHECK(r == 0);
        else CHECK(r > prev);
        prev = r;
    }
    CHECK(kmeans_train_row(nt - 1, n, nt) < n);
    if (nt == n)
        for (uint64_t i = 0; i < nt; i += step)
            CHECK(kmeans_train_row(i, n, nt) == i);
    /* init rows: centroid 0 is training row 0, distinct, inside [0, nt) */
    int64_t pj = -1;
    for (uint32_t j = 0; j < nlist; ++j) {
        const uint64_t r = kmeans_init_row(j, nt, nlist);
        CHECK(r < nt);
        CHECK((int64_t)r > pj);
        pj = (int64_t)r;
    }
    CHECK(kmeans_init_row(0, nt, nlist) == 0);
    if (nt == nlist)
        for (uint32_t j = 0; j < nlist; ++j)
            CHECK(kmeans_init_row(j, nt, nlist) == j);
}

bool throws_n_lt_nlist(uint64_t n, uint32_t nlist) {
    try {
        (void)kmeans_n_train(n, nlist, 0.5, 0);
    } catch (const std::runtime_error& e) {
        return std::string(e.what()).find("fewer vectors") != std::string::npos;
    }
    return false;
}

void check_reseed() {
    snprintf(g_case, sizeof g_case, "reseed: plain order");
    {
        const float best[] = {1.f, 9.f, 3.f, 7.f, 5.f};
        auto r = kmeans_pick_reseeds(best, 5, 3);
        CHECK(r.size() == 3 && r[0] == 1 && r[1] == 3 && r[2] == 4);
        CHECK(kmeans_pick_reseeds(best, 5, 0).empty());
    }
    snprintf(g_case, sizeof g_case, "reseed: ties go to the lower row");
    {
        const float best[] = {2.f, 5.f, 5.f, 1.f, 5.f, 2.f};
        auto r = kmeans_pick_reseeds(best, 6, 4);
        CHECK(r.size() == 4 && r[0] == 1 && r[1] == 2 && r[2] == 4 &&
              r[3] == 0);
    }
    snprintf(g_case, sizeof g_case,
             "reseed: more empties than distinct far rows");
    {
        /* one far row, everything else at distance 0: the rest of the
         * empties take the lowest rows, each row once */
        std::vector<float> best(10, 0.f);
        best[6] = 4.f;
        auto r = kmeans_pick_reseeds(best.data(), best.size(), 5);
        CHECK(r.size() == 5 && r[0] == 6 && r[1] == 0 && r[2] == 1 &&
              r[3] == 2 && r[4] == 3);
        /* every row needed */
        auto all = kmeans_pick_reseeds(best.data(), best.size(), best.size());
        std::vector<int64_t> sorted = all;
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 0; i < sorted.size(); ++i) CHECK(sorted[i] == (int64_t)i);
        bool threw = false;
        try {
            (void)kmeans_pick_reseeds(best.data(), best.size(), 11);
        } catch (const std::logic_error&) {
            threw = true;
        }
        CHECK(threw);
    }
    snprintf(g_case, sizeof g_case, "reseed: NaN ranks last, inf first");
    {
        const float best[] = {NAN, 1.f, INFINITY, NAN, 2.f};
        auto r = kmeans_pick_reseeds(best, 5, 4);
        CHECK(r[0] == 2 && r[1] == 4 && r[2] == 1 && r[3] == 0);
    }
}

void check_stop_and_params() {
    snprintf(g_case, sizeof g_case, "stop rule / parameter defaults");
    CHECK(kmeans_iters(0) == 20 && kmeans_iters(7) == 7);
    CHECK(kmeans_fraction(0.0) == 0.5 && kmeans_fraction(-1.0) == 0.5);
    CHECK(kmeans_fraction(1.5) == 0.5 && kmeans_fraction(NAN) == 0.5);
    CHECK(kmeans_fraction(1.0) == 1.0 && kmeans_fraction(0.25) == 0.25);
    CHECK(kmeans_should_stop(0, 1, false, 3));   /* last allowed iteration */
    CHECK(kmeans_should_stop(19, 0, false, 0));  /* default 20 */
    CHECK(!kmeans_should_stop(18, 0, false, 0));
    CHECK(kmeans_should_stop(3, 20, true, 0));   /* converged */
    CHECK(!kmeans_should_stop(3, 20, true, 1));  /* converged but reseeded */
    CHECK(!kmeans_should_stop(3, 20, false, 0));
}

}  // namespace

int main() {
    /* n == nlist: everything trains, row i seeds centroid i */
    check_sample(16, 16, 0.5, 0, 16);
    check_sample(1, 1, 0.5, 0, 1);
    /* n_train == nlist exactly from the fraction */
    check_sample(64, 32, 0.5, 0, 32);
    /* fraction giving n_train < nlist: raised to nlist */
    check_sample(100, 40, 0.1, 0, 40);
    check_sample(1000, 999, 0.001, 0, 999);
    /* ceil */
    check_sample(777, 33, 0.5, 0, 389);
    check_sample(5000, 24, 0.5, 0, 2500);
    check_sample(4112, 16, 1.0, 0, 4112);
    /* invalid fractions fall back to 0.5 */
    check_sample(1000, 10, 0.0, 0, 500);
    check_sample(1000, 10, 7.0, 0, 500);
    /* the cap: bounds from above, not below nlist, no effect when larger */
    check_sample(1000, 10, 1.0, 300, 300);
    check_sample(1000, 10, 0.5, 5, 10);
    check_sample(1000, 10, 0.5, 100000, 500);
    /* past 2^31 elements and 2^32 in i*n */
    check_sample(10000000, 4096, 0.5, 0, 5000000);
    check_sample(6000000000ull, 65536, 1.0, 4000000000ull, 4000000000ull);
    CHECK(kmeans_train_row(3999999999ull, 6000000000ull, 4000000000ull) ==
          5999999998ull);

    snprintf(g_case, sizeof g_case, "n < nlist is an error");
    CHECK(throws_n_lt_nlist(15, 16));
    CHECK(throws_n_lt_nlist(0, 1));

    check_reseed();
    check_stop_and_params();
    printf("kmeans_plan_check OK: %d checks\n", g_checks);
    return 0;
}
