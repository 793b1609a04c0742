"""A numpy restatement of the terms aggregation with a top_hits sub-aggregation over a key column
(``rass_index_aggregate_hits_keys``), for the tests: nothing here comes from the engine.  Who matches is
``groupkeys_ref._matches``; the scores are a matrix the caller computed (the oracle's)."""
import numpy as np

from groupkeys_ref import NEG_INF, _matches, pack_bits  # noqa: F401  (pack_bits: for the tests that import this module alone)

BY_COUNT, BY_SCORE = 0, 1
ORDER_NAMES = {BY_COUNT: "_count", BY_SCORE: "max_score"}
NAMES = ("groups", "counts", "scores", "ids", "n_buckets", "total_hits")


def expect_top_hits(scores, tags, keys, n_groups, size, top_hits, thr, order=BY_COUNT, allow=None, qfilter=None, qmask=None, ids=None):
    """(groups [nq, size] i32, counts i64, scores [nq, size, top_hits] f32, ids i64, n_buckets [nq], total_hits [nq], status).
    The hits of query q: the matching rows with a group and ``s >= thr[q]``, ``s > -inf``; one with ``key >= n_groups`` sets
    status and is left out.  Per query the hits are put under ``np.lexsort((rows, -s))``; a bucket's list is its hits in that
    order, cut at ``top_hits``; the buckets are ordered by (count desc, key asc) or by the place of their best hit in that
    order, and the ``size`` first are listed."""
    nq, n = scores.shape
    keys = np.asarray(keys, dtype=np.int64)[:n]
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
    row_id = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    eg = np.full((nq, size), -1, dtype=np.int32)
    ec = np.zeros((nq, size), dtype=np.int64)
    es = np.full((nq, size, top_hits), NEG_INF, dtype=np.float32)
    ei = np.full((nq, size, top_hits), -1, dtype=np.int64)
    eb = np.zeros(nq, dtype=np.int64)
    et = np.zeros(nq, dtype=np.int64)
    status = 0
    for q in range(nq):
        with np.errstate(invalid="ignore"):
            hit = _matches(tags, keys, q, allow, qfilter, qmask) & (scores[q] >= thr[q]) & (scores[q] > NEG_INF)
        if np.any(hit & (keys >= n_groups)):
            status = 1
        rows = np.flatnonzero(hit & (keys < n_groups))
        et[q] = len(rows)
        if len(rows) == 0:
            continue
        rows = rows[np.lexsort((rows, -scores[q, rows]))]      # score desc, row asc
        s = scores[q, rows]
        uk, first, inv, count = np.unique(keys[rows], return_index=True, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        eb[q] = len(uk)
        order_of = np.lexsort((uk, -count)) if order == BY_COUNT else np.argsort(first)
        for j, b in enumerate(order_of[:size].tolist()):
            mine = np.flatnonzero(inv == b)[:top_hits]          # already best first
            eg[q, j], ec[q, j] = uk[b], count[b]
            es[q, j, :len(mine)] = s[mine]
            ei[q, j, :len(mine)] = row_id[rows[mine]]
    return eg, ec, es, ei, eb, et, status


def brute_force(scores, tags, keys, n_groups, size, top_hits, thr, order, allow=None, qfilter=None, qmask=None):
    """The same answer by plain Python loops over rows and buckets: dictionaries and ``sorted``, no numpy ranking."""
    nq, n = scores.shape
    out = []
    status = 0
    for q in range(nq):
        buckets = {}
        for r in range(n):
            if tags[r] == -1 or keys[r] < 0:
                continue
            if qfilter is not None and qfilter[q] >= 0 and ((int(tags[r]) & int(qmask[q])) if qmask is not None else int(tags[r])) != qfilter[q]:
                continue
            if allow is not None and not (allow[r] if allow.ndim == 1 else allow[q, r]):
                continue
            s = float(scores[q, r])
            t = float(np.broadcast_to(thr, (nq,))[q])
            if not (s >= t) or s == float("-inf"):
                continue
            if keys[r] >= n_groups:
                status = 1
                continue
            buckets.setdefault(int(keys[r]), []).append((-s, r))
        for g in buckets:
            buckets[g].sort()
        if order == BY_COUNT:
            listed = sorted(buckets, key=lambda g: (-len(buckets[g]), g))
        else:
            listed = sorted(buckets, key=lambda g: buckets[g][0])
        out.append(dict(n_buckets=len(buckets), total=sum(len(v) for v in buckets.values()),
                        buckets=[(g, len(buckets[g]), [(r, -ms) for ms, r in buckets[g][:top_hits]]) for g in listed[:size]]))
    return out, status


def count_and_cascade(keys, levels, rng):
    """``grouphits_ref.cascade`` with the counter the top-hits emission keeps next to the chain: one thread per key (distinct,
    > 0), the threads' memory steps interleaved at random.  A thread first adds 1 to the counter, THEN makes the relaxed
    pre-read of the last slot, which may end it, then walks the chain.  Returns (counter, slots)."""
    slot = [0] * levels
    count = 0
    threads = [dict(key=int(key), level=-2) for key in keys]    # level -2: the count is still to come, -1: the pre-read
    live = list(range(len(threads)))
    while live:
        pick = int(rng.integers(len(live)))
        t = threads[live[pick]]
        if t["level"] == -2:
            count += 1
            t["level"] = -1
        elif t["level"] == -1:
            if t["key"] <= slot[levels - 1]:
                live.pop(pick)
            else:
                t["level"] = 0
        else:
            old = slot[t["level"]]
            slot[t["level"]] = max(old, t["key"])
            t["key"] = min(old, t["key"])
            t["level"] += 1
            if t["key"] == 0 or t["level"] == levels:
                live.pop(pick)
    return count, slot
