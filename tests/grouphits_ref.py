"""A numpy restatement of the grouped search with inner hits over a key column (``rass_index_search_group_hits_keys``) and of
the slot cascade its scan keeps per (query, group), for the tests: nothing here comes from the engine.  Who matches is
``groupkeys_ref._matches``; the scores are a matrix the caller computed (the oracle's)."""
import numpy as np

from groupkeys_ref import NEG_INF, _matches


def expect_group_hits(scores, tags, keys, n_groups, k, group_size, allow=None, qfilter=None, qmask=None, ids=None):
    """(scores [nq, k, group_size], ids, groups [nq, k], totals [nq], capped scores [nq, k], capped ids, status).  Per query:
    the matching rows under ``np.lexsort((rows, -s))``; a row's rank within its group is its position among the group's rows
    in that order (so each group is sorted by the same lexsort), the first ``group_size`` of a group are kept; the groups are
    ordered by their best row, the first ``k`` listed.  Capped: the first ``k`` rows of that order after dropping, per
    group, everything past its ``group_size`` best, over EVERY group: no use is made of the k best groups sufficing."""
    nq, n = scores.shape
    keys = np.asarray(keys, dtype=np.int64)[:n]
    row_id = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    hs = np.full((nq, k, group_size), NEG_INF, dtype=np.float32)
    hi = np.full((nq, k, group_size), -1, dtype=np.int64)
    eg = np.full((nq, k), -1, dtype=np.int32)
    et = np.zeros(nq, dtype=np.int64)
    cs = np.full((nq, k), NEG_INF, dtype=np.float32)
    ci = np.full((nq, k), -1, dtype=np.int64)
    status = 0
    for q in range(nq):
        ok = _matches(tags, keys, q, allow, qfilter, qmask)
        with np.errstate(invalid="ignore"):
            ok &= scores[q] > NEG_INF                      # NaN and -inf never rank: no match, no status
        if np.any(ok & (keys >= n_groups)):
            status = 1
        rows = np.flatnonzero(ok & (keys < n_groups))
        if len(rows) == 0:
            continue
        rows = rows[np.lexsort((rows, -scores[q, rows]))]  # score desc, row asc
        s = scores[q, rows]
        uniq, first, inv = np.unique(keys[rows], return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        pos = np.empty(len(uniq), dtype=np.int64)          # a group's place: by its first (best) row in the ranking
        pos[np.argsort(first)] = np.arange(len(uniq))
        by_group = np.argsort(inv, kind="stable")          # the ranking, cut into its groups
        start = np.searchsorted(inv[by_group], np.arange(len(uniq)))
        rank = np.empty(len(rows), dtype=np.int64)         # a row's place within its group
        rank[by_group] = np.arange(len(rows)) - start[inv[by_group]]
        et[q] = len(uniq)
        m = min(len(uniq), k)
        eg[q, :m] = uniq[np.argsort(first)[:m]]
        sel = (pos[inv] < k) & (rank < group_size)
        hs[q, pos[inv][sel], rank[sel]] = s[sel]
        hi[q, pos[inv][sel], rank[sel]] = row_id[rows[sel]]
        pool = np.flatnonzero(rank < group_size)[:k]
        cs[q, :len(pool)] = s[pool]
        ci[q, :len(pool)] = row_id[rows[pool]]
    return hs, hi, eg, et, cs, ci, status


def cascade(keys, levels, rng):
    """The chain of ``levels`` slots of one (query, group) after every key of ``keys`` (distinct, > 0) went through the
    scan's emission, one thread per key, the threads' individual memory steps interleaved at random: a relaxed pre-read of the
    last slot (which may skip the key), then per level one atomic max that returns the old value, the smaller of the two
    moving down, until it is 0 or falls off the end.  Returns the slots, level 0 first."""
    slot = [0] * levels
    threads = [dict(key=int(key), level=-1) for key in keys]    # level -1: the pre-read is still to come
    live = list(range(len(threads)))
    while live:
        pick = int(rng.integers(len(live)))
        t = threads[live[pick]]
        if t["level"] < 0:
            if t["key"] <= slot[levels - 1]:
                live.pop(pick)
                continue
            t["level"] = 0
            continue
        old = slot[t["level"]]
        slot[t["level"]] = max(old, t["key"])
        t["key"] = min(old, t["key"])
        t["level"] += 1
        if t["key"] == 0 or t["level"] == levels:
            live.pop(pick)
    return slot
