"""A numpy restatement of the key-column builders and of the grouped search / aggregation over a key column, for the tests:
nothing here comes from the engine.  Keys: ``value - base`` or ``np.searchsorted(edges, v, side="right") - 1`` with the
out-of-range and missing rules of include/rass_engine.h.  Grouping: over a score matrix the caller computed (the oracle's)."""
import numpy as np

MISSING = -(1 << 31)
KEY_NONE = -1
INT32_MAX = (1 << 31) - 1
NEG_INF = np.float32(-np.inf)


def keys_from_attr(values, base, missing_key, n_keys):
    """int32 [n_keys]: ``v - base`` where it lies in [0, INT32_MAX] (no overflow: int64), ``missing_key`` for a missing value,
    -1 otherwise and past the values."""
    v = np.asarray(values, dtype=np.int64)
    d = v - int(base)
    k = np.where((d < 0) | (d > INT32_MAX), KEY_NONE, d)
    k = np.where(v == MISSING, int(missing_key), k)
    out = np.full(n_keys, KEY_NONE, dtype=np.int32)
    out[:len(v)] = k
    return out


def keys_from_edges(values, edges, missing_key, n_keys):
    """int32 [n_keys]: j where ``edges[j] <= v < edges[j + 1]``, -1 below the first edge and at or above the last,
    ``missing_key`` for a missing value, -1 past the values."""
    v = np.asarray(values, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64)
    j = np.searchsorted(e, v, side="right") - 1
    k = np.where((j < 0) | (j >= len(e) - 1), KEY_NONE, j)
    k = np.where(v == MISSING, int(missing_key), k)
    out = np.full(n_keys, KEY_NONE, dtype=np.int32)
    out[:len(v)] = k
    return out


def attr_minmax(values, tags):
    """(min, max, n_present) over the live rows with a value; (None, None, 0) without one."""
    v = np.asarray(values, dtype=np.int64)
    ok = (v != MISSING) & (np.asarray(tags) != -1)
    return (int(v[ok].min()), int(v[ok].max()), int(ok.sum())) if ok.any() else (None, None, 0)


def _matches(tags, keys, q, allow, qfilter, qmask):
    """The rows that match query q and have a group: live, filter passed, bit set, key >= 0."""
    ok = (tags != -1) & (keys >= 0)
    if qfilter is not None and qfilter[q] >= 0:
        ok &= ((tags & qmask[q]) if qmask is not None else tags) == qfilter[q]
    if allow is not None:
        ok &= allow if allow.ndim == 1 else allow[q]
    return ok


def expect_grouped(scores, tags, keys, n_groups, k, allow=None, qfilter=None, qmask=None, ids=None):
    """(scores [nq, k], ids, groups, totals [nq], status) of the grouped search over a key column.  ``keys``: one int per
    row of ``tags`` (the caller pads a short column with -1).  ``allow``: bool [n] or [nq, n], or None."""
    nq, n = scores.shape
    keys = np.asarray(keys, dtype=np.int64)[:n]
    row_id = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    es = np.full((nq, k), NEG_INF, dtype=np.float32)
    ei = np.full((nq, k), -1, dtype=np.int64)
    eg = np.full((nq, k), -1, dtype=np.int32)
    et = np.zeros(nq, dtype=np.int64)
    status = 0
    for q in range(nq):
        ok = _matches(tags, keys, q, allow, qfilter, qmask)
        if np.any(ok & (keys >= n_groups)):
            status = 1
        rows = np.flatnonzero(ok & (keys < n_groups))
        if len(rows) == 0:
            continue
        s = scores[q, rows]
        order = np.lexsort((rows, -s))                     # score desc, row asc
        rows, s = rows[order], s[order]
        _, first = np.unique(keys[rows], return_index=True)   # a group's representative = its first row in the ranking
        first = np.sort(first)                             # ... and the representatives in that same order
        et[q] = len(first)
        m = min(len(first), k)
        es[q, :m], ei[q, :m], eg[q, :m] = s[first[:m]], row_id[rows[first[:m]]], keys[rows[first[:m]]]
    return es, ei, eg, et, status


def expect_counts(scores, tags, keys, n_groups, size, thr, allow=None, qfilter=None, qmask=None, ids=None):
    """(groups [nq, size], counts, scores, ids, n_buckets [nq], total_hits [nq], status) of the aggregation over a key
    column: the hits are the matching rows with a group and ``s >= thr[q]``."""
    nq, n = scores.shape
    keys = np.asarray(keys, dtype=np.int64)[:n]
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
    row_id = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    eg = np.full((nq, size), -1, dtype=np.int32)
    ec = np.zeros((nq, size), dtype=np.int64)
    es = np.full((nq, size), NEG_INF, dtype=np.float32)
    ei = np.full((nq, size), -1, dtype=np.int64)
    eb = np.zeros(nq, dtype=np.int64)
    et = np.zeros(nq, dtype=np.int64)
    status = 0
    for q in range(nq):
        hit = _matches(tags, keys, q, allow, qfilter, qmask) & (scores[q] >= thr[q])
        if np.any(hit & (keys >= n_groups)):
            status = 1
        rows = np.flatnonzero(hit & (keys < n_groups))
        et[q] = len(rows)
        if len(rows) == 0:
            continue
        uk, count = np.unique(keys[rows], return_counts=True)
        order = np.lexsort((uk, -count))                   # doc_count desc, then key asc
        uk, count = uk[order], count[order]
        eb[q] = len(uk)
        s = scores[q, rows]
        rank = np.lexsort((rows, -s))
        rows, s = rows[rank], s[rank]
        ku, first = np.unique(keys[rows], return_index=True)
        best = dict(zip(ku.tolist(), first.tolist()))
        m = min(len(uk), size)
        f = np.array([best[g] for g in uk[:m].tolist()], dtype=np.int64)
        eg[q, :m], ec[q, :m], es[q, :m], ei[q, :m] = uk[:m], count[:m], s[f], row_id[rows[f]]
    return eg, ec, es, ei, eb, et, status


def pack_bits(mask):
    """bool [..., n] -> uint32 words [..., ceil(n / 32)], bit (r & 31) of word r >> 5 = row r."""
    m = np.asarray(mask, dtype=bool)
    n = m.shape[-1]
    pad = (-n) % 32
    m = np.concatenate([m, np.zeros(m.shape[:-1] + (pad,), dtype=bool)], axis=-1)
    b = m.reshape(m.shape[:-1] + (-1, 32)).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
