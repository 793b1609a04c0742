"""Numpy restatements of the IVF probe within a row bitmap (``rass_ivf_search_allowed_delta``): the slab-order words the
bridge kernel produces, the rows a probe may return, and the byte rule that routes a filtered search."""
import numpy as np


def slab_words(slab_ids: np.ndarray, allow_bits: np.ndarray, tiles, rows) -> np.ndarray:
    """The slab-order word of each of ``tiles`` (with ``rows`` valid rows each) for ONE query: bit r = allow_bits[slab_ids[32 *
    tile + r]], 0 where r >= rows, the position is padding (-1) or the source row lies past the bitmap."""
    out = np.zeros(len(tiles), dtype=np.uint32)
    n = allow_bits.shape[0]
    for j, (t, nr) in enumerate(zip(tiles, rows)):
        w = 0
        for r in range(min(int(nr), 32)):
            src = int(slab_ids[32 * int(t) + r])
            if 0 <= src < n and allow_bits[src]:
                w |= 1 << r
        out[j] = w
    return out


def member_bits(assign: np.ndarray, probe_lists_q, covered: int, n: int) -> np.ndarray:
    """bool [n]: the rows a probe of the lists ``probe_lists_q`` (ids; -1 = none) may return — the covered rows assigned to
    one of them, and every row from ``covered`` on (the delta)."""
    lists = [int(l) for l in np.asarray(probe_lists_q).reshape(-1) if int(l) >= 0]
    m = np.zeros(n, dtype=bool)
    m[:covered] = np.isin(np.asarray(assign)[:covered], lists)
    m[covered:] = True
    return m


def route(counts, nq: int, shared: bool, nprobe: int, covered: int, nlist: int, factor: float = 1.0) -> str:
    """The byte rule: "ivf" iff 32 * C > factor * nprobe * covered / nlist for the call's largest launch group of 32 queries,
    C = the group's summed bitmap counts (the one count of a shared bitmap); else "flat"."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if nq <= 0 or counts.size == 0 or nlist <= 0:
        return "flat"
    if shared:
        c = int(counts[0])
    else:
        c = max(int(counts[g:g + 32].sum()) for g in range(0, min(nq, counts.size), 32))
    return "ivf" if 32 * c > factor * nprobe * covered / nlist else "flat"
