"""A numpy restatement of the stats aggregation over a key column (``rass_index_aggregate_stats_keys``), for the tests:
nothing here comes from the engine.  From a score matrix the caller computed (the oracle's), tags, keys, values, thresholds,
bitmap and filters it gives, per (query, group), ``count``, ``vcount``, ``sum`` (int64), ``min``, ``max`` and the best row, and
from those the listed buckets under each order, ``n_buckets`` and ``total_hits``.  All of it is integer arithmetic."""
import numpy as np

from groupkeys_ref import NEG_INF, pack_bits  # noqa: F401  (re-exported for the tests)

MISSING = -(1 << 31)
BY_COUNT, BY_VALUE_COUNT, BY_MIN, BY_MAX = range(4)
NAMES = ("groups", "counts", "scores", "ids", "value_counts", "sums", "mins", "maxs", "n_buckets", "total_hits")


def hits(scores, tags, keys, thr, q, allow=None, qfilter=None, qmask=None):
    """bool [n]: the rows that are hits of query q — live, filter passed, a group (key >= 0; ``keys`` None: every row is in
    group 0), bit set, ``s >= thr[q]`` (NaN: nothing; -inf: every such row with a score above -inf)."""
    n = scores.shape[1]
    ok = tags != -1
    if keys is not None:
        ok = ok & (keys >= 0)
    if qfilter is not None and qfilter[q] >= 0:
        ok = ok & (((tags & qmask[q]) if qmask is not None else tags) == qfilter[q])
    if allow is not None:
        ok = ok & (allow if allow.ndim == 1 else allow[q])[:n]
    with np.errstate(invalid="ignore"):
        return ok & (scores[q] >= thr[q]) & (scores[q] > NEG_INF)


def table(scores, tags, keys, values, n_groups, thr, allow=None, qfilter=None, qmask=None):
    """Per query a dict of arrays over the groups with a hit, group ascending — ``group``, ``count``, ``vcount``, ``sum``
    (int64), ``min``, ``max`` (int64; meaningless where vcount is 0), ``best_row``, ``best_score`` — and the status flag (a
    hit with key >= n_groups, left out)."""
    nq, n = scores.shape
    keys64 = None if keys is None else np.asarray(keys, dtype=np.int64)[:n]
    g_of = np.zeros(n, dtype=np.int64) if keys64 is None else keys64
    vals = np.full(n, MISSING, dtype=np.int64) if values is None else np.asarray(values, dtype=np.int64)[:n]
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
    out, status = [], 0
    for q in range(nq):
        h = hits(scores, tags, keys64, thr, q, allow, qfilter, qmask)
        if np.any(h & (g_of >= n_groups)):
            status = 1
        rows = np.flatnonzero(h & (g_of < n_groups))
        ug, inv = np.unique(g_of[rows], return_inverse=True)
        m = len(ug)
        v = vals[rows]
        has = v != MISSING
        sm = np.zeros(m, dtype=np.int64)
        mn = np.full(m, np.iinfo(np.int64).max, dtype=np.int64)
        mx = np.full(m, np.iinfo(np.int64).min, dtype=np.int64)
        np.add.at(sm, inv[has], v[has])
        np.minimum.at(mn, inv[has], v[has])
        np.maximum.at(mx, inv[has], v[has])
        rank = np.lexsort((rows, -scores[q, rows]))           # score desc, row asc
        _, first = np.unique(inv[rank], return_index=True)    # a group's best row: its first in the ranking
        best = rows[rank[first]] if m else np.zeros(0, dtype=np.int64)
        out.append(dict(group=ug, count=np.bincount(inv, minlength=m).astype(np.int64),
                        vcount=np.bincount(inv[has], minlength=m).astype(np.int64), sum=sm, min=mn, max=mx, best_row=best,
                        best_score=scores[q, best]))
    return out, status


def order_buckets(per, order_by, descending):
    """Positions into one query's table in the listing order: the metric ascending or descending, ties by group ascending, and
    (for the metrics of the value) the groups without a present value last in both directions, group ascending."""
    sign = -1 if descending else 1
    if order_by == BY_COUNT:
        return np.lexsort((per["group"], sign * per["count"]))
    metric = per[{BY_VALUE_COUNT: "vcount", BY_MIN: "min", BY_MAX: "max"}[order_by]]
    none = per["vcount"] == 0
    return np.lexsort((per["group"], np.where(none, 0, sign * metric), none))


def expect(scores, tags, keys, values, n_groups, size, thr, order_by=BY_COUNT, descending=True, allow=None, qfilter=None,
           qmask=None, ids=None, tab=None):
    """(groups [nq, size] int32, counts int64, scores float32, ids int64, value_counts int64, sums int64, mins int32, maxs
    int32, n_buckets [nq] int64, total_hits [nq] int64, status).  ``tab``: a ``table()`` result to reuse."""
    nq, n = scores.shape
    per_q, status = tab if tab is not None else table(scores, tags, keys, values, n_groups, thr, allow, qfilter, qmask)
    row_id = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    eg = np.full((nq, size), -1, dtype=np.int32)
    ec = np.zeros((nq, size), dtype=np.int64)
    es = np.full((nq, size), NEG_INF, dtype=np.float32)
    ei = np.full((nq, size), -1, dtype=np.int64)
    evc = np.zeros((nq, size), dtype=np.int64)
    esum = np.zeros((nq, size), dtype=np.int64)
    emin = np.zeros((nq, size), dtype=np.int32)
    emax = np.zeros((nq, size), dtype=np.int32)
    eb = np.zeros(nq, dtype=np.int64)
    et = np.zeros(nq, dtype=np.int64)
    for q, per in enumerate(per_q):
        eb[q] = len(per["group"])
        et[q] = per["count"].sum()
        o = order_buckets(per, order_by, descending)[:size]
        m = len(o)
        has = per["vcount"][o] > 0
        eg[q, :m], ec[q, :m], es[q, :m], ei[q, :m] = per["group"][o], per["count"][o], per["best_score"][o], row_id[per["best_row"][o]]
        evc[q, :m], esum[q, :m] = per["vcount"][o], np.where(has, per["sum"][o], 0)
        emin[q, :m], emax[q, :m] = np.where(has, per["min"][o], 0), np.where(has, per["max"][o], 0)
    return eg, ec, es, ei, evc, esum, emin, emax, eb, et, status
