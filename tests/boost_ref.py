"""numpy fp32 restatement of the boosted search (``rass_index_search_boosted``) and of its column builders
(``rass_index_bonus_scatter`` / ``_from_attr_clauses`` / ``_mask``), for the tests.  Every operation is a separate float32
array operation, so each step is rounded on its own exactly as the kernels round it (scan_boost.hip, bonus.hip); ties are
broken by id ascending; the rule for scores that are not finite is applied.  No GPU, no engine."""
import numpy as np

NEG_INF = np.float32(-np.inf)
ATTR_MISSING = -(1 << 31)


def transform(s, mode):
    """T(cos), fp32: mode 0 / "raw" = s, 1 / "opensearch" = 1 / (2 - s) as two rounded operations."""
    s = np.asarray(s, dtype=np.float32)
    if mode in (0, "raw"):
        return s
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.float32(1) / (np.float32(2) - s)).astype(np.float32)


def fused_scores(s, boost, bonus, mode=0):
    """boost * T(s) + bonus over one query's rows: a rounded product, then a rounded sum (never an fma)."""
    t = transform(s, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (np.float32(boost) * t).astype(np.float32)
        return (prod + np.asarray(bonus, dtype=np.float32)).astype(np.float32)


def rank(s, fused, live, k, after=None):
    """(scores [k], ids [k]) of one query: the rows with ``live`` set, a cosine above -inf and a fused score above -inf (NaN
    fails both tests), by (fused desc, id asc), cut at k and padded with (-inf, -1).  ``after``: (score, id) continuation."""
    s, fused = np.asarray(s, dtype=np.float32), np.asarray(fused, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.asarray(live, dtype=bool) & (s > NEG_INF) & (fused > NEG_INF)
    rows = np.flatnonzero(ok)
    if after is not None:
        f = fused[rows]
        rows = rows[(f < after[0]) | ((f == after[0]) & (rows > after[1]))]
    order = np.lexsort((rows, -fused[rows].astype(np.float64)))[:k]
    out_s = np.full(k, NEG_INF, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[:len(order)], out_i[:len(order)] = fused[rows[order]], rows[order]
    return out_s, out_i


def search(scores, k, boost=None, bonus=None, mode=0, live=None, bonus_rows=None):
    """The whole answer.  ``scores`` [nq, n]: the cosines as the scan computes them.  ``bonus``: [n'] shared or [nq, n'] (n'
    >= bonus_rows), None = zeros; rows at or past ``bonus_rows`` (default n') read 0.  ``boost``: [nq] or None (1.0).
    ``live``: bool [n] or [nq, n] (tombstones and filters folded in by the caller), None = every row."""
    scores = np.asarray(scores, dtype=np.float32)
    nq, n = scores.shape
    out_s = np.full((nq, k), NEG_INF, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        b = np.zeros(n, dtype=np.float32)
        if bonus is not None:
            col = np.asarray(bonus, dtype=np.float32)
            col = col if col.ndim == 1 else col[q]
            m = min(n, len(col) if bonus_rows is None else bonus_rows)
            b[:m] = col[:m]
        lv = np.ones(n, dtype=bool) if live is None else (live if np.ndim(live) == 1 else live[q])
        f = fused_scores(scores[q], 1.0 if boost is None else boost[q], b, mode)
        out_s[q], out_i[q] = rank(scores[q], f, lv, k)
    return out_s, out_i


def scatter(bonus, q_of, rows, values):
    """bonus[q_of[i], rows[i]] += values[i], one rounded add per entry, in place; the pairs are unique."""
    bonus = bonus if bonus.ndim == 2 else bonus[None, :]
    for q, r, v in zip(q_of, rows, values):
        bonus[q, r] = np.float32(bonus[q, r]) + np.float32(v)
    return bonus


def clause_holds(cols, clause):
    """bool [n]: clause (query, col, lo, hi, negate) over the int32 columns ``cols`` (dict col -> [n]; absent = all missing)."""
    _, c, lo, hi, neg = (int(x) for x in clause)
    n = len(next(iter(cols.values())))
    v = np.asarray(cols.get(c, np.full(n, ATTR_MISSING, dtype=np.int64)), dtype=np.int64)
    return ((v != ATTR_MISSING) & (lo <= v) & (v <= hi)) != bool(neg)


def from_attr_clauses(bonus, cols, clauses, weights, n_rows, op="replace"):
    """Per (query, row < n_rows): b = 0 (replace) or the cell (add), then b += weight for every clause of the query that
    holds, in list order, one rounded fp32 add each; in place.  ``bonus`` [n_bonus, stride] (or [stride]: query 0)."""
    bonus = bonus if bonus.ndim == 2 else bonus[None, :]
    for q in range(bonus.shape[0]):
        b = np.zeros(n_rows, dtype=np.float32) if op == "replace" else bonus[q, :n_rows].copy()
        for cl, w in zip(clauses, weights):
            if int(cl[0]) != q:
                continue
            b = np.where(clause_holds(cols, cl)[:n_rows], (b + np.float32(w)).astype(np.float32), b)
        bonus[q, :n_rows] = b
    return bonus


def mask(bonus, bits, n_rows):
    """bonus[q, r] = -inf where bits[q or 0, r] is clear, r < n_rows; in place.  ``bits``: bool [1 or n_bonus, >= n_rows]."""
    bonus = bonus if bonus.ndim == 2 else bonus[None, :]
    for q in range(bonus.shape[0]):
        b = bits[0] if bits.shape[0] == 1 else bits[q]
        bonus[q, :n_rows][~b[:n_rows]] = NEG_INF
    return bonus
