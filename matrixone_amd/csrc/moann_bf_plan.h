/* Planner of the resident brute-force index (moann_bf_lib.cpp): how one
 * search is cut into query batches, row slices and candidate buffers, and how
 * the row store grows. Pure integer host code, no HIP: bf_plan_check.cpp
 * asserts its invariants under ASan + UBSan.
 *
 * A search runs in one of two modes over the same candidate-buffer shape
 * [q_batch][slices][k] of (distance, row) pairs:
 *   fused  bf_fused_topk_kernel: grid = slices x query blocks of 128 queries,
 *          a slice is a whole number of 128-row tiles;
 *   gemm   launch_rank_gemm into a [q_batch][slice_rows] distance tile, then
 *          launch_topk per slice ("chunk"). Over an f16 row store the slice
 *          is first widened to an f32 tile [slice_rows][dpad4], which has a
 *          byte cap of its own.
 * Both end in one launch_topk over slices*k candidates per query. */

#ifndef MOANN_BF_PLAN_H
#define MOANN_BF_PLAN_H

#include <cstdint>
#include <stdexcept>
#include <string>

namespace moann {

constexpr int64_t BF_TILE = 128;        /* rows per tile (both modes)        */
constexpr int64_t BF_QTILE = 128;       /* queries per fused block           */
constexpr int64_t BF_FUSED_KMAX = 64;   /* largest k of the fused kernel     */
constexpr int64_t BF_K_LIMIT = 4096;    /* launch_topk's limit               */
constexpr int64_t BF_MAX_ROWS = 2147483647; /* rows are int32 in candidates  */
/* byte caps of the two per-search buffers: (distance f32, row i32) pairs of
 * the candidate buffer, and the f32 distance tile of the gemm mode */
constexpr int64_t BF_CAND_CAP = (int64_t)256 << 20;
constexpr int64_t BF_DMAT_CAP = (int64_t)256 << 20;
/* byte cap of the widened f32 tile of the gemm mode over an f16 store */
constexpr int64_t BF_WIDE_CAP = (int64_t)256 << 20;
constexpr int64_t BF_QBATCH_MAX = (int64_t)1 << 20; /* keeps every grid int32 */

enum BfMode : int { BF_AUTO = 0, BF_FUSED = 1, BF_GEMM = 2 };

struct BfPlan {
    int mode = BF_GEMM;     /* BF_FUSED or BF_GEMM, never BF_AUTO            */
    int64_t q_batch = 0;    /* queries per pass; passes are independent      */
    int64_t passes = 0;     /* ceil(nq / q_batch)                            */
    int64_t query_blocks = 0; /* fused blocks along the queries, full pass   */
    int64_t tiles = 0;      /* ceil(n / BF_TILE)                             */
    int64_t tiles_per_slice = 0;
    int64_t slice_rows = 0; /* tiles_per_slice * BF_TILE                     */
    int64_t slices = 0;     /* S; slice s = rows [s*slice_rows, ...) cut at n */
    int64_t cand_entries = 0; /* q_batch * slices * k                        */
    int64_t dmat_entries = 0; /* gemm: q_batch * min(slice_rows, n), else 0  */
    int64_t wide_bytes = 0; /* gemm over a narrow store: min(slice_rows, n) *
                               wide_row_bytes, else 0                        */
};

inline int64_t bf_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

/* Longest gemm slice, in tiles, whose widened f32 copy stays inside
 * BF_WIDE_CAP; one tile at least. wide_row_bytes > 0. */
inline int64_t bf_wide_tiles(int64_t wide_row_bytes) {
    const int64_t t = BF_WIDE_CAP / wide_row_bytes / BF_TILE;
    return t < 1 ? 1 : t;
}

/* The `auto` rule, from the medians in profiles/r05_README.md (MI355X,
 * dim 768 unless noted): the fused kernel where it can serve k and the search
 * is large enough to fill its 128-query x 128-row blocks. Fused beat gemm at
 * (rows, nq) = (1M, 4..1024), (100k, 128), (100k, 1024), (30k, 1024), also
 * at k = 64 and at dim 128; gemm beat fused at (10k, 1024), (100k, 16) and
 * (1M, 1). The two bounds below separate those two sets; between the
 * measured shapes they are an interpolation. */
constexpr int64_t BF_AUTO_MIN_ROWS = 30000;
constexpr int64_t BF_AUTO_MIN_PAIRS = 4000000; /* rows * queries */
/* Over an f16 store (`narrow`), from the medians in profiles/r06_README.md
 * (same machine and shapes, wall ms fused / gemm): the gemm mode pays for
 * widening each slice and the fused kernel runs on the f16 MFMA, so fused
 * also won where it lost over f32: (1M, 1) 1.02 / 5.43, (1M, 16) 1.08 /
 * 5.51, (100k, 16) 0.60 / 0.70; and as over f32 at (1M, 128) 1.05 / 8.58,
 * (1M, 1024) 3.64 / 37.3, (100k, 128) 0.59 / 1.06, (100k, 1024) 1.18 / 4.11,
 * (30k, 1024) 0.92 / 1.55, k = 64 10.4 / 37.4, dim 128 1.73 / 11.6. At
 * (10k, 1024) the two were level, 0.81 / 0.84, inside the run-to-run spread,
 * and fewer rows were not measured: the row bound stays, the pair bound
 * drops to the smallest product at which fused won. */
constexpr int64_t BF_AUTO_MIN_PAIRS_NARROW = 1000000;

inline int bf_auto_mode(int64_t n, int64_t nq, int64_t k,
                        bool narrow = false) {
    /* n < 2^31 and nq capped first: the product stays inside int64 */
    const int64_t q = nq < BF_QBATCH_MAX ? nq : BF_QBATCH_MAX;
    return k <= BF_FUSED_KMAX && n >= BF_AUTO_MIN_ROWS &&
                   n * q >= (narrow ? BF_AUTO_MIN_PAIRS_NARROW
                                    : BF_AUTO_MIN_PAIRS)
               ? BF_FUSED
               : BF_GEMM;
}

/* Row range of slice s. */
inline void bf_slice_range(const BfPlan& p, int64_t n, int64_t s, int64_t* lo,
                           int64_t* hi) {
    *lo = s * p.slice_rows;
    const int64_t end = *lo + p.slice_rows;
    *hi = end < n ? end : n;
}

/* n rows, nq queries, top k; `mode` as passed to moann_bf_set_params,
 * `slice_rows` its override (0 = choose here), `cus` the device's compute
 * units. n >= 1 and nq >= 1: the caller answers n = 0 and nq = 0 itself.
 * `wide_row_bytes`: bytes of one row of the f32 tile a gemm slice is widened
 * to (f16 store: dpad4 * 4), 0 for an f32 store; with 0 the plan is the one
 * this function always made. Throws std::invalid_argument for arguments
 * outside the contract. */
inline BfPlan bf_plan(int64_t n, int64_t nq, int64_t k, int mode,
                      int64_t slice_rows, int cus,
                      int64_t wide_row_bytes = 0) {
    if (n < 1 || n > BF_MAX_ROWS)
        throw std::invalid_argument("row count outside [1, 2^31-1]");
    if (nq < 1) throw std::invalid_argument("no queries to plan for");
    if (k < 1 || k > BF_K_LIMIT)
        throw std::invalid_argument("k must be in [1, 4096]");
    if (mode != BF_AUTO && mode != BF_FUSED && mode != BF_GEMM)
        throw std::invalid_argument("mode must be 0 (auto), 1 (fused) or 2 (gemm)");
    if (slice_rows < 0 || slice_rows % BF_TILE != 0)
        throw std::invalid_argument(
            "slice_rows must be 0 or a multiple of the 128-row tile");
    if (wide_row_bytes < 0 || wide_row_bytes > ((int64_t)1 << 40))
        throw std::invalid_argument("widened row bytes outside [0, 2^40]");
    if (cus < 1) cus = 1;

    BfPlan p;
    p.mode = mode == BF_AUTO ? bf_auto_mode(n, nq, k, wide_row_bytes != 0)
                             : mode;
    if (p.mode == BF_FUSED && k > BF_FUSED_KMAX)
        throw std::invalid_argument(
            "fused mode serves k <= " + std::to_string(BF_FUSED_KMAX) +
            " (moann_bf_fused_kmax); use mode auto or gemm");
    p.tiles = bf_ceil_div(n, BF_TILE);

    /* gemm over a narrow store: no slice longer than its widened tile allows */
    const int64_t wide_tps = p.mode == BF_GEMM && wide_row_bytes
                                 ? bf_wide_tiles(wide_row_bytes)
                                 : p.tiles;
    if (slice_rows && (slice_rows / BF_TILE < p.tiles ? slice_rows / BF_TILE
                                                       : p.tiles) > wide_tps)
        throw std::invalid_argument(
            "slice_rows is too long for this storage in gemm mode: the "
            "widened f32 tile would exceed its cap (at most " +
            std::to_string(wide_tps * BF_TILE) + " rows)");

    /* Shrink the query batch until both buffers fit their caps. Fewer
     * queries per pass mean more slices in the fused mode (more blocks are
     * wanted along the rows) but never more than 2*cus of them, and longer
     * chunks in the gemm mode, so the loop ends at q_batch = 1 at the latest
     * unless an override forces short slices over many rows. */
    int64_t qb = nq < BF_QBATCH_MAX ? nq : BF_QBATCH_MAX;
    for (;;) {
        int64_t tps;
        if (slice_rows) {
            tps = slice_rows / BF_TILE;
        } else if (p.mode == BF_FUSED) {
            const int64_t qblocks = bf_ceil_div(qb, BF_QTILE);
            int64_t want = (2 * (int64_t)cus) / qblocks;
            if (want < 1) want = 1;
            if (want > p.tiles) want = p.tiles;
            tps = bf_ceil_div(p.tiles, want);
        } else {
            tps = BF_DMAT_CAP / 4 / qb / BF_TILE;
            if (tps < 1) tps = 1;
        }
        if (tps > p.tiles) tps = p.tiles;
        if (tps > wide_tps) tps = wide_tps;
        const int64_t S = bf_ceil_div(p.tiles, tps);
        /* S <= 2^24, k <= 2^12, qb <= 2^20: the products stay inside int64 */
        const bool fits = S * k < ((int64_t)1 << 31) &&
                          qb * S * k * 8 <= BF_CAND_CAP &&
                          bf_ceil_div(qb, BF_QTILE) * S < ((int64_t)1 << 31) &&
                          (p.mode != BF_GEMM ||
                           qb * (tps * BF_TILE < n ? tps * BF_TILE : n) * 4 <=
                               BF_DMAT_CAP || (!slice_rows && tps == 1));
        if (fits) {
            p.q_batch = qb;
            p.tiles_per_slice = tps;
            p.slice_rows = tps * BF_TILE;
            p.slices = S;
            break;
        }
        if (qb == 1)
            throw std::invalid_argument(
                slice_rows || !wide_row_bytes
                    ? "slice_rows does not fit this many rows: a search "
                      "buffer would exceed its cap"
                    : "this many rows do not fit the gemm mode over this "
                      "storage: the candidate buffer would exceed its cap");
        /* whole query tiles while there are several, then halves */
        qb = qb > BF_QTILE ? bf_ceil_div(qb / 2, BF_QTILE) * BF_QTILE : qb / 2;
    }
    p.passes = bf_ceil_div(nq, p.q_batch);
    p.query_blocks = bf_ceil_div(p.q_batch, BF_QTILE);
    p.cand_entries = p.q_batch * p.slices * k;
    if (p.mode == BF_GEMM)
        p.dmat_entries = p.q_batch * (p.slice_rows < n ? p.slice_rows : n);
    if (p.mode == BF_GEMM)
        p.wide_bytes = (p.slice_rows < n ? p.slice_rows : n) * wide_row_bytes;
    return p;
}

/* Capacity after adding `add` rows to `len` stored ones: unchanged while they
 * fit, else doubled until they do (at least 64 rows), never above
 * BF_MAX_ROWS. More rows than that is an error. */
inline int64_t bf_next_capacity(int64_t cap, int64_t len, int64_t add) {
    if (len < 0 || add < 0 || len > BF_MAX_ROWS || add > BF_MAX_ROWS - len)
        throw std::invalid_argument(
            "the index holds at most 2^31-1 rows");
    const int64_t need = len + add;
    if (need <= cap) return cap;
    int64_t c = cap < 64 ? 64 : cap;
    while (c < need) c = c > BF_MAX_ROWS / 2 ? BF_MAX_ROWS : c * 2;
    return c;
}

}  // namespace moann

#endif
