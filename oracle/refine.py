"""ORACLE — test infrastructure ONLY: reference for the two-stage refine scan.

The product's refine mode (moann_ivf_flat_enable_refine) runs
  1. a byte first pass over an internal clip-quantized image of the rows,
  2. a per-query top-R by byte distance,
  3. an exact f32 re-rank of those R candidates,
  4. a top-k of the re-ranked set.
Stage 2 may break byte-distance ties any way it likes, so the result is not a
single array but a SET of admissible arrays. This module restates the
quantizer and the byte distance (numpy + the existing oracle), derives the
band of candidates stage 1 must / may keep, and checks a result against that
tie-tolerant contract. It never reads anything back from the index: the
quantizer is re-derived from the rows.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as orc

FLT_MAX = np.float32(np.finfo(np.float32).max)
# the project's parity bar (tests/test_parity_gpu.py::_assert_parity)
RTOL = 1e-5
ATOL = 1e-6
# the product samples the first RQ_SAMPLE_ROWS rows in slot order
RQ_SAMPLE_ROWS = 131072


def rq_params(vecs):
    """Clip quantizer of enable_refine: the 0.1% / 99.9% order statistics of
    the flattened rows -> (mul, add) computed in f64, used as f32."""
    v = np.asarray(vecs, dtype=np.float32)
    # sample == all rows, so slot order does not matter
    assert v.shape[0] <= RQ_SAMPLE_ROWS, "reference models n <= 131072 only"
    flat = np.sort(v.reshape(-1))
    nlo = flat.size // 1000
    lo = float(flat[nlo])
    hi = float(flat[flat.size - 1 - nlo])
    rng = hi - lo
    if rng > 0:
        mul = 255.0 / rng
        add = -lo * mul - 128.0
    else:
        mul, add = 1.0, 0.0
    return np.float32(mul), np.float32(add)


def rq_quantize(x, mul, add):
    """Signed-byte codes of rows or queries. The kernel always evaluates
    x*mul+add (two f32 roundings); orc.quantize skips the arithmetic for the
    identity map, which gives the same bytes."""
    return orc.quantize(x, float(mul), float(add), unsigned=False)


def byte_dists(metric, codes, qcode):
    """Stage-1 distances: exact integer-domain metric, then the kernel's
    (float) cast — monotone, and it can merge neighbours above 2^24."""
    return orc._int_metric_dists(metric, codes, qcode).astype(np.float32)


def stage1_band(bdist, pass_mask, R, cos=False):
    """Which candidates a correct top-R by byte distance MUST keep (strictly
    below the R-th smallest passing byte distance T) and MAY keep (<= T).
    When no more than R pass, all passing candidates are both. For cosine the
    byte distance goes through f64 sqrt/div, so the band is one f32 ulp wider
    on each side of T."""
    b = np.asarray(bdist, dtype=np.float32)
    pm = np.asarray(pass_mask, dtype=bool)
    npass = int(pm.sum())
    if npass <= R:
        return pm.copy(), pm.copy()
    T = np.partition(b[pm], R - 1)[R - 1]
    t_lo, t_hi = T, T
    if cos:
        t_lo = np.nextafter(T, np.float32(-np.inf))
        t_hi = np.nextafter(T, np.float32(np.inf))
    return pm & (b < t_lo), pm & (b <= t_hi)


@dataclass
class TwoStageRef:
    """Everything check_two_stage needs for one (index, metric, queries,
    probe): per query the candidate rows in candidate-position order (probe
    lists in probe order, rows in list order), their byte distances and their
    exact oracle distances."""
    metric: int
    orig_l2: bool
    row_ids: np.ndarray               # id of every row
    cand_rows: list = field(default_factory=list)
    bdist: list = field(default_factory=list)
    exact: list = field(default_factory=list)

    @property
    def nq(self):
        return len(self.cand_rows)


def build_ref(idx: "orc.IvfIndex", metric, queries, probe, orig_l2=False,
              params=None, codes=None) -> TwoStageRef:
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    nq = queries.shape[0]
    n = idx.vecs.shape[0]
    if params is None:
        params = rq_params(idx.vecs)
    mul, add = params
    if codes is None:
        codes = rq_quantize(idx.vecs, mul, add)
    row_ids = (idx.ids if idx.ids is not None
               else np.arange(n, dtype=np.int64))
    ref = TwoStageRef(metric, orig_l2, row_ids)
    _, _, probe_ids = idx.search(metric, queries, probe, 1, orig_l2=orig_l2,
                                 want_probe=True)
    kmax = 1
    for qi in range(nq):
        rows = [idx.slot_rows[idx.list_offsets[l]:idx.list_offsets[l + 1]]
                for l in probe_ids[qi] if l >= 0]
        rows = (np.concatenate(rows) if rows
                else np.empty(0, dtype=np.int64))
        ref.cand_rows.append(rows)
        kmax = max(kmax, rows.size)
    # exact distances of every candidate: one full-depth oracle search (the
    # same C distance kernels as orc.distance, conventions + sqrt applied)
    order = np.argsort(row_ids, kind="stable")
    sorted_ids = row_ids[order]
    all_ids, all_d = idx.search(metric, queries, probe, kmax, orig_l2=orig_l2)
    qcodes = rq_quantize(queries, mul, add)
    for qi in range(nq):
        rows = ref.cand_rows[qi]
        live = all_ids[qi] >= 0
        assert int(live.sum()) == rows.size
        by_row = np.full(n, np.nan, dtype=np.float32)
        by_row[order[np.searchsorted(sorted_ids, all_ids[qi][live])]] = \
            all_d[qi][live]
        ex = by_row[rows]
        assert not np.isnan(ex).any()
        ref.exact.append(ex)
        ref.bdist.append(byte_dists(metric, codes[rows], qcodes[qi])
                         if rows.size else np.empty(0, dtype=np.float32))
    return ref


def _pass_mask(ref, qi, allowed):
    rows = ref.cand_rows[qi]
    if allowed is None:
        return np.ones(rows.size, dtype=bool)
    return np.asarray(allowed, dtype=bool)[rows]


def ideal_two_stage(ref: TwoStageRef, k, R, allowed=None, stage1_edit=None):
    """The result of an exact implementation that breaks every tie by
    candidate position. `allowed` is a bool mask over ROWS (filter and soft
    deletes). stage1_edit=(query, drop_pos, add_pos or None) corrupts that
    query's stage-1 selection (self-test of the checker)."""
    nq = ref.nq
    out_ids = np.full((nq, k), -1, dtype=np.int64)
    out_d = np.full((nq, k), FLT_MAX, dtype=np.float32)
    for qi in range(nq):
        pm = _pass_mask(ref, qi, allowed)
        pos = np.flatnonzero(pm)
        sel = pos[np.argsort(ref.bdist[qi][pos], kind="stable")[:R]]
        if stage1_edit is not None and stage1_edit[0] == qi:
            _, drop, add_pos = stage1_edit
            sel = sel[sel != drop]
            if add_pos is not None:
                sel = np.append(sel, add_pos)
        sel = np.sort(sel)
        top = sel[np.argsort(ref.exact[qi][sel], kind="stable")[:k]]
        out_ids[qi, :top.size] = ref.row_ids[ref.cand_rows[qi][top]]
        out_d[qi, :top.size] = ref.exact[qi][top]
    return out_ids, out_d


def check_two_stage(got_ids, got_dists, ref: TwoStageRef, k, R, allowed=None,
                    ctx="", only=None):
    """Tie-tolerant contract of the two-stage scan. Per query:
      (a) every returned id is a stage-1 MAY candidate and passes the filter;
      (b) its distance is the oracle's exact distance (rtol 1e-5, atol 1e-6);
      (c) distances ascend; padding is (-1, FLT_MAX) and only at the tail;
      (d) exactly min(k, #passing, R) entries are live;
      (e) every stage-1 MUST candidate whose exact distance is below the last
          live distance by more than the tolerance is present.
    MUST candidates within the tolerance of that cut-off may legitimately fall
    on either side; they are counted, not judged.
    Returns (skipped, n_must); raises AssertionError naming the clause."""
    got_ids = np.asarray(got_ids)
    got_dists = np.asarray(got_dists, dtype=np.float32)
    assert got_ids.shape == (ref.nq, k) and got_dists.shape == (ref.nq, k), \
        f"{ctx}: result shape {got_ids.shape} != {(ref.nq, k)}"
    cos = ref.metric == orc.METRIC_COS
    skipped = n_must = 0
    for qi in (range(ref.nq) if only is None else only):
        where = f"{ctx} query {qi}"
        rows = ref.cand_rows[qi]
        pm = _pass_mask(ref, qi, allowed)
        must, may = stage1_band(ref.bdist[qi], pm, R, cos=cos)
        gi, gd = got_ids[qi], got_dists[qi]
        live = gi >= 0
        nlive = int(live.sum())
        expect = min(k, int(pm.sum()), R)
        assert nlive == expect, \
            f"(d) {where}: {nlive} live entries, expected {expect}"
        assert live[:nlive].all() and (gi[nlive:] == -1).all() and \
            (gd[nlive:] == FLT_MAX).all(), \
            f"(c) {where}: padding is not (-1, FLT_MAX) at the tail"
        gi, gd = gi[:nlive], gd[:nlive]
        assert (np.diff(gd) >= 0).all(), f"(c) {where}: not ascending: {gd}"
        # returned ids -> candidate positions
        cand_ids = ref.row_ids[rows]
        order = np.argsort(cand_ids, kind="stable")
        sid = cand_ids[order]
        at = np.minimum(np.searchsorted(sid, gi), max(sid.size - 1, 0))
        found = (sid[at] == gi) if sid.size else np.zeros(nlive, dtype=bool)
        assert found.all(), \
            f"(a) {where}: ids {gi[~found]} are not candidates of the probe"
        pos = order[at]
        assert np.unique(pos).size == nlive, \
            f"(a) {where}: an id is returned twice: {gi}"
        assert pm[pos].all(), \
            f"(a) {where}: filtered-out ids returned: {gi[~pm[pos]]}"
        assert may[pos].all(), \
            f"(a) {where}: ids {gi[~may[pos]]} lie outside the stage-1 band"
        ex = ref.exact[qi]
        err = np.abs(gd.astype(np.float64) - ex[pos].astype(np.float64))
        lim = ATOL + RTOL * np.abs(ex[pos].astype(np.float64))
        assert (err <= lim).all(), (
            f"(b) {where}: distance off the exact value by up to "
            f"{(err / np.maximum(lim, 1e-300)).max():.1f}x the tolerance")
        # completeness
        cutoff = float(gd[-1]) if (nlive == k and nlive) else np.inf
        tol = ATOL + RTOL * abs(cutoff) if np.isfinite(cutoff) else 0.0
        present = np.zeros(rows.size, dtype=bool)
        present[pos] = True
        missing = must & ~present
        exd = ex.astype(np.float64)
        bad = missing & (exd < cutoff - tol)
        assert not bad.any(), (
            f"(e) {where}: {int(bad.sum())} stage-1 MUST candidates closer "
            f"than the cut-off {cutoff} are absent, ids "
            f"{cand_ids[bad][:8]} exact {ex[bad][:8]}")
        skipped += int((missing & (np.abs(exd - cutoff) <= tol)).sum())
        n_must += int(must.sum())
    return skipped, n_must
