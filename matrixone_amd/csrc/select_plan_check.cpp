/* CPU check of the threshold-filter selection's rule (moann_select_plan.h):
 * where it engages, the sample positions and the threshold rank at their
 * edges. Host compiler only, built with ASan + UBSan by
 * `make select_plan_check`; run by tests/test_select_plan.py. Exit 0 and a
 * one-line summary on success, first violated invariant on stderr and exit 1
 * otherwise. */

#include "moann_select_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace moann;

namespace {

char g_case[128] = "";
int g_checks = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            fprintf(stderr, "select_plan_check: %s:%d: %s\n  case: %s\n",  \
                    __FILE__, __LINE__, #cond, g_case);                    \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

void check_plan(int64_t count, int k) {
    snprintf(g_case, sizeof g_case, "count=%lld k=%d", (long long)count, k);
    const SelectPlan p = select_plan(count, k);
    CHECK(p.filter ==
          (k >= 1 && k <= SELECT_KMAX && count >= SELECT_MIN_COUNT));
    if (!p.filter) return;
    CHECK(p.m == SELECT_SAMPLE && p.m % SELECT_THREADS == 0);
    CHECK(p.m % SELECT_CLUSTER == 0);
    CHECK(p.t >= SELECT_T_MIN && p.t <= p.m);
    /* expected collected keys t*count/m: at least OVERSAMPLE*k, and either
     * within one sample step of it or at the rank floor */
    const double expect = (double)p.t * (double)count / p.m;
    CHECK(expect >= (double)SELECT_OVERSAMPLE * k);
    CHECK(expect < (double)SELECT_OVERSAMPLE * k + (double)count / p.m ||
          p.t == SELECT_T_MIN);
    /* k <= expect: a threshold at its expectation never undershoots; the
     * capacity is at least twice the target while the floor does not bind */
    if (p.t > SELECT_T_MIN) CHECK(2 * expect <= SELECT_CAPACITY + 2.0 * count / p.m);
    /* sample positions: inside the row, strictly ascending, first at 0, runs
     * of SELECT_CLUSTER consecutive keys, the last run within one run step
     * of the end */
    const int runs = p.m / SELECT_CLUSTER;
    int64_t prev = -1;
    for (int i = 0; i < p.m; ++i) {
        const int64_t pos = select_sample_pos(count, p.m, i);
        CHECK(pos > prev && pos < count);
        if (i % SELECT_CLUSTER) CHECK(pos == prev + 1);
        prev = pos;
    }
    CHECK(select_sample_pos(count, p.m, 0) == 0);
    CHECK(count - prev <= count / runs + 1);
}

}  // namespace

int main() {
    const int64_t M = SELECT_MIN_COUNT;
    const int64_t counts[] = {0, 1, 63, 64, 4095, 4096, M - 1, M, M + 1,
                              M + 2, M + 3, M + 17, 3 * M + 5, 20000, 78000,
                              78125, 1000000, 10000000,
                              ((int64_t)1 << 31) - 1, (int64_t)1 << 32,
                              (int64_t)1 << 40};
    const int ks[] = {-1, 0, 1, 10, 63, 64, 65, SELECT_KMAX, SELECT_KMAX + 1,
                      1024, 4096};
    for (int64_t c : counts)
        for (int k : ks) check_plan(c, k);

    /* the constants hang together */
    snprintf(g_case, sizeof g_case, "constants");
    CHECK(SELECT_OVERSAMPLE * SELECT_KMAX * 2 <= SELECT_CAPACITY);
    CHECK(SELECT_MIN_COUNT >= SELECT_SAMPLE && SELECT_MIN_COUNT > SELECT_KMAX);
    CHECK(SELECT_SAMPLE % SELECT_THREADS == 0);
    /* largest rank: smallest row, largest k */
    CHECK(select_plan(SELECT_MIN_COUNT, SELECT_KMAX).t ==
          SELECT_OVERSAMPLE * SELECT_KMAX * SELECT_SAMPLE / SELECT_MIN_COUNT);

    /* the flagship: 78 000 candidates, top 64 -> rank 27, ~514 collected */
    {
        const SelectPlan p = select_plan(78000, 64);
        CHECK(p.filter && p.t == 27);
        CHECK(!select_plan(78000, SELECT_KMAX + 1).filter);
        CHECK(select_plan(78000, 10).t == SELECT_T_MIN);
    }
    printf("select_plan_check OK: %d checks\n", g_checks);
    return 0;
}
