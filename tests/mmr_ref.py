"""The reference of the diversified (MMR) search, in numpy (include/rass_engine.h, rass_index_search_mmr).

``select_f32`` restates the selection rule operation by operation in ``np.float32`` (every product and the difference are
rounded to fp32 on their own, as the kernel's ``__fmul_rn`` / ``__fsub_rn``): given the engine's own candidate scores and
Gram matrix its answer must be EQUAL to the device's.  ``gram_f64`` and ``mmr_f64`` are float64 and serve the accuracy
bound of the Gram kernel and the sanity properties of the rule."""
import numpy as np

F32 = np.float32


def select_f32(s, G, lam, k):
    """``s`` [fetch_k] candidate scores (score desc), ``G`` [fetch_k, fetch_k], ``lam`` in [0, 1], ``k``; ``c`` = the number
    of real candidates = entries of ``s`` above -inf.  Returns the picked ranks, ``min(k, c)`` of them, in selection order."""
    s = np.asarray(s, dtype=F32)
    G = np.asarray(G, dtype=F32)
    c = int(np.count_nonzero(s > -np.inf))
    lam = F32(lam)
    m = F32(F32(1.0) - lam)
    rel = (lam * s[:c]).astype(F32)                 # one rounding per product
    pen = np.zeros(c, dtype=F32)
    free = np.ones(c, dtype=bool)
    picked = []
    for t in range(min(int(k), c)):
        second = np.zeros(c, dtype=F32) if t == 0 else (m * pen).astype(F32)
        obj = (rel - second).astype(F32)
        obj = np.where(free, obj, -np.inf)
        p = int(np.argmax(obj))                     # the first of the largest: ties go to the lowest rank
        picked.append(p)
        free[p] = False
        g = G[p, :c]
        pen = g.copy() if t == 0 else np.where(g > pen, g, pen)
    return np.array(picked, dtype=np.int32)


def gram_f64(rows):
    """``rows`` [L, dim] -> their Gram matrix in float64."""
    r = np.asarray(rows, dtype=np.float64)
    return r @ r.T


def mmr_f64(q, rows, lam, k):
    """The same greedy rule in float64 over a query ``q`` [dim] and candidate ``rows`` [c, dim] given in rank order.
    Returns the picked ranks."""
    r = np.asarray(rows, dtype=np.float64)
    s = r @ np.asarray(q, dtype=np.float64)
    G = r @ r.T
    c = len(s)
    pen = np.zeros(c)
    free = np.ones(c, dtype=bool)
    picked = []
    for t in range(min(int(k), c)):
        obj = lam * s - (0.0 if t == 0 else (1.0 - lam) * pen)
        obj = np.where(free, obj, -np.inf)
        p = int(np.argmax(obj))
        picked.append(p)
        free[p] = False
        pen = G[p].copy() if t == 0 else np.maximum(pen, G[p])
    return np.array(picked, dtype=np.int32)
