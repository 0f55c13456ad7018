/* Sampling rule of the threshold-filter selection (select_filter_kernel,
 * moann_kernels.hip): which rows take the filter path, where the sample is
 * read, which sample rank becomes the threshold. Pure integer arithmetic, no
 * HIP and no globals, evaluated per row by the kernel and by the host alike;
 * checked on the CPU by select_plan_check.cpp.
 *
 * The filter finds the k smallest of a long row in one read: every key not
 * above a threshold is collected in LDS and sorted. The threshold is the key
 * of rank t among m keys sampled over the row, so about t*count/m keys pass
 * it (relative spread about 1/sqrt(t)). The rule aims that figure at
 * SELECT_OVERSAMPLE * k, well under SELECT_CAPACITY; a row that collects
 * fewer than k keys, or more than the capacity, falls back to the radix
 * select, so the rule decides time only, never the result.
 *
 * The sample is m / SELECT_CLUSTER runs of SELECT_CLUSTER consecutive keys,
 * the runs spread evenly over the row. Single keys at an even stride touch
 * every cache line of a 78 000-key row, a second full read of it (measured:
 * profiles/r07_README.md); runs touch 1/19 of the lines. Neighbours in the
 * candidate buffer are unrelated rows of one list, so a run samples its list
 * as well as 16 scattered keys would. */

#ifndef MOANN_SELECT_PLAN_H
#define MOANN_SELECT_PLAN_H

#include <cstdint>

#if defined(__HIPCC__)
#define MOANN_SELECT_HD __host__ __device__
#else
#define MOANN_SELECT_HD
#endif

namespace moann {

constexpr int SELECT_THREADS = 256;   /* one block per row                   */
constexpr int SELECT_SAMPLE = 4096;   /* m: 16 keys per thread, in registers */
constexpr int SELECT_CLUSTER = 16;    /* consecutive keys per sampled run    */
constexpr int SELECT_CAPACITY = 2048; /* collected (key, index) pairs in LDS */
constexpr int SELECT_OVERSAMPLE = 8;  /* expected collected / k              */
constexpr int SELECT_T_MIN = 8;       /* smallest threshold rank             */
/* largest k: SELECT_OVERSAMPLE * k is half the capacity, ~8 sigma below it
 * at the smallest t this k can get (64) */
constexpr int SELECT_KMAX = 128;
/* smallest row: the sample is at most a quarter of it (runs stay apart) */
constexpr int64_t SELECT_MIN_COUNT = 4 * (int64_t)SELECT_SAMPLE;

struct SelectPlan {
    bool filter; /* false: the row goes straight to the radix select */
    int m;       /* sampled keys                                     */
    int t;       /* threshold = t-th smallest sampled key, 1-based   */
};

/* position (row-relative) of sample i < m: run i / SELECT_CLUSTER starts at
 * that share of the row; ascending, distinct and inside the row while
 * count >= m */
MOANN_SELECT_HD inline int64_t select_sample_pos(int64_t count, int m, int i) {
    const int runs = m / SELECT_CLUSTER;
    return (int64_t)(i / SELECT_CLUSTER) * count / runs + i % SELECT_CLUSTER;
}

MOANN_SELECT_HD inline SelectPlan select_plan(int64_t count, int k) {
    SelectPlan p;
    p.m = SELECT_SAMPLE;
    p.t = 0;
    p.filter = k >= 1 && k <= SELECT_KMAX && count >= SELECT_MIN_COUNT;
    if (!p.filter) return p;
    /* t * count / m ~ SELECT_OVERSAMPLE * k, rounded up */
    const int64_t want = (int64_t)SELECT_OVERSAMPLE * k * p.m;
    int64_t t = (want + count - 1) / count;
    if (t < SELECT_T_MIN) t = SELECT_T_MIN;
    p.t = (int)t; /* <= OVERSAMPLE * KMAX * m / MIN_COUNT = 256 */
    return p;
}

}  // namespace moann

#endif
