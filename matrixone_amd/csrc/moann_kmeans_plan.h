/* Host-side arithmetic of the native k-means build: which staged rows form
 * the training sample, which of them seed the centroids, which rows refill
 * empty centroids, and when training stops. Pure integer / comparison code —
 * no HIP, no globals — so it runs (and is sanitized) on the CPU:
 * kmeans_plan_check.cpp. These rules are part of the documented build
 * contract (include/moann.h): a caller can restate them and
 * predict the centroids an index trains. */

#ifndef MOANN_KMEANS_PLAN_H
#define MOANN_KMEANS_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

namespace moann {

constexpr uint32_t KMEANS_DEFAULT_ITERS = 20;      /* cuVS's default      */
constexpr double KMEANS_DEFAULT_FRACTION = 0.5;    /* the reference's      */

/* build_params.kmeans_trainset_fraction as stored on the index: values
 * <= 0, > 1 or NaN fall back to the reference default. */
inline double kmeans_fraction(double f) {
    return (f > 0.0 && f <= 1.0) ? f : KMEANS_DEFAULT_FRACTION;
}

inline uint32_t kmeans_iters(uint32_t n_iters) {
    return n_iters ? n_iters : KMEANS_DEFAULT_ITERS;
}

/* Training sample size: ceil(fraction * n), never below min(n, nlist) (one
 * row per centroid), never above n; `max_train_rows` (0 = no cap) bounds it
 * from above but not below that floor. n < nlist is an error. */
inline uint64_t kmeans_n_train(uint64_t n, uint32_t nlist, double fraction,
                               uint64_t max_train_rows) {
    if (nlist == 0) throw std::runtime_error("kmeans: n_lists is 0");
    if (n < nlist)
        throw std::runtime_error(
            "kmeans: fewer vectors (" + std::to_string(n) + ") than lists (" +
            std::to_string(nlist) + ")");
    const uint64_t floor_rows = std::min<uint64_t>(n, nlist);
    uint64_t want = (uint64_t)std::ceil(kmeans_fraction(fraction) * (double)n);
    if (max_train_rows) want = std::min(want, max_train_rows);
    return std::min(n, std::max(want, floor_rows));
}

/* Training row i (0 <= i < n_train) is staged row (i*n)/n_train: an even
 * stride over the add order, strictly increasing because n >= n_train. */
inline uint64_t kmeans_train_row(uint64_t i, uint64_t n, uint64_t n_train) {
    return (uint64_t)(((unsigned __int128)i * n) / n_train);
}

/* Centroid j starts as training row (j*n_train)/nlist. */
inline uint64_t kmeans_init_row(uint32_t j, uint64_t n_train, uint32_t nlist) {
    return (uint64_t)(((unsigned __int128)j * n_train) / nlist);
}

/* Rows that refill `n_empty` empty centroids: the training rows with the
 * largest `best` distance, ties to the lower row, each row once. Entry e
 * goes to the e-th empty centroid in ascending centroid index. NaN ranks
 * below every number. */
inline std::vector<int64_t> kmeans_pick_reseeds(const float* best,
                                                uint64_t n_train,
                                                uint64_t n_empty) {
    if (n_empty > n_train)
        throw std::logic_error("kmeans: more empty centroids than rows");
    std::vector<int64_t> idx(n_train);
    std::iota(idx.begin(), idx.end(), (int64_t)0);
    auto key = [best](int64_t r) {
        const float b = best[r];
        return std::isnan(b) ? -INFINITY : b;
    };
    std::partial_sort(idx.begin(), idx.begin() + (int64_t)n_empty, idx.end(),
                      [&](int64_t a, int64_t b) {
                          const float ka = key(a), kb = key(b);
                          return ka != kb ? ka > kb : a < b;
                      });
    idx.resize(n_empty);
    return idx;
}

/* Stop after iteration `iter` (0-based) when it was the last allowed one,
 * or when it changed no assignment and left no centroid empty. */
inline bool kmeans_should_stop(uint32_t iter, uint32_t n_iters,
                               bool same_assignment, uint64_t n_empty) {
    if (iter + 1 >= kmeans_iters(n_iters)) return true;
    return same_assignment && n_empty == 0;
}

}  // namespace moann

#endif
