"""numpy restatement of the function-score search (``rass_index_search_scored``) and of its column builder
(``rass_index_fn_from_attr``), for the tests.  No GPU, no engine.

The builder is restated in float64 with the operations in the order include/rass_engine.h gives, each numpy operation rounded
on its own, and rounded to float32 once at the end: cells built from + - * / sqrt and comparisons alone are what the device
computes bit for bit (IEEE double on both sides); cells through exp or a logarithm may differ from the device's by what two
libm's differ by before that one rounding (``through_libm`` says which cells those are).

The scan is restated in float32 with every operation rounded on its own, max / min as a compare and a select, the gate on the
transformed similarity, the exclusion rules, and ties by id ascending (``boost_ref.rank``)."""
import math

import numpy as np

import boost_ref as B

NEG_INF = np.float32(-np.inf)
ATTR_MISSING = -(1 << 31)
MAX_SCORE_FNS = 16
COMBINE = ("sum", "multiply", "avg", "max", "min", "replace")
SCORE_MODES = ("multiply", "sum", "avg", "first", "max", "min")
DECAY = ("gauss", "exp", "linear")
LIBM_MODIFIERS = ("log", "log1p", "log2p", "ln", "ln1p", "ln2p")


# ---- the builder, float64
def decay_constant(kind, scale, decay):
    """The per-function constant the host derives in double (libm's log, as the C++ entry point's)."""
    if kind == "gauss":
        return math.log(decay) / (scale * scale)
    if kind == "exp":
        return math.log(decay) / scale
    return scale / (1.0 - decay)


def modifier(name, x):
    with np.errstate(all="ignore"):
        if name in (None, "none"):
            return x
        if name == "log":
            return np.log10(x)
        if name == "log1p":
            return np.log10(1.0 + x)
        if name == "log2p":
            return np.log10(2.0 + x)
        if name == "ln":
            return np.log(x)
        if name == "ln1p":
            return np.log(1.0 + x)
        if name == "ln2p":
            return np.log(2.0 + x)
        if name == "square":
            return x * x
        if name == "sqrt":
            return np.sqrt(x)
        if name == "reciprocal":
            return 1.0 / x
    raise ValueError(name)


def fn_value(fn, cols, n):
    """(value f64 [n], applies bool [n]) of one function before its filter: weight * kind(v)."""
    kind = fn["kind"]
    applies = np.ones(n, dtype=bool)
    if kind == "weight":
        x = np.ones(n, dtype=np.float64)
    else:
        v = np.asarray(cols.get(int(fn.get("col", 0)), np.full(n, ATTR_MISSING)), dtype=np.int64)[:n]
        miss = v == ATTR_MISSING
        vd = v.astype(np.float64)
        if kind in DECAY:
            c = np.float64(decay_constant(kind, float(fn["scale"]), float(fn["decay"])))
            dist = np.abs(vd - np.float64(fn["origin"])) - np.float64(fn.get("offset", 0.0))
            d = np.where(dist > 0.0, dist, 0.0)
            with np.errstate(all="ignore"):
                if kind == "gauss":
                    x = np.exp(d * d * c)
                elif kind == "exp":
                    x = np.exp(d * c)
                else:
                    lin = (c - d) / c
                    x = np.where(lin > 0.0, lin, 0.0)
            x = np.where(miss, 1.0, x)
        else:
            missing = fn.get("missing")
            if missing is None:
                applies = ~miss
                missing = np.nan
            with np.errstate(all="ignore"):
                x = modifier(fn.get("modifier"), np.float64(fn.get("factor", 1.0)) * np.where(miss, np.float64(missing), vd))
    with np.errstate(all="ignore"):
        return np.float64(fn.get("weight", 1.0)) * x, applies


def through_libm(fn):
    """Whether the function's cells pass through exp or a logarithm (the 1-ulp allowance of the builder test)."""
    return fn["kind"] in ("gauss", "exp") or (fn["kind"] == "field_value_factor" and fn.get("modifier") in LIBM_MODIFIERS)


def build_column(functions, cols, n, n_fn=1, score_mode="multiply", max_boost=None, filters=None, as_f64=False):
    """The column block [n_fn, n] (float32, or the float64 before the one rounding).  ``functions``: dicts as
    ``FlatIndex.fn_from_attr`` takes them; ``cols``: {col: int [n]} (absent: all missing); ``filters``: bool [n_filters, n]."""
    assert score_mode in SCORE_MODES
    cap = np.float64(np.inf if max_boost is None else max_boost)
    out = np.ones((n_fn, n), dtype=np.float64)
    for q in range(n_fn):
        acc = np.ones(n, dtype=np.float64)
        wsum = np.zeros(n, dtype=np.float64)
        seen = np.zeros(n, dtype=bool)
        for fn in functions:
            if int(fn.get("query", 0)) != q:
                continue
            x, applies = fn_value(fn, cols, n)
            if fn.get("filter") is not None:
                applies = applies & np.asarray(filters[int(fn["filter"])][:n], dtype=bool)
            with np.errstate(all="ignore"):
                if score_mode == "multiply":
                    nxt = acc * x
                elif score_mode in ("sum", "avg"):
                    nxt = acc + x
                elif score_mode == "first":
                    nxt = acc
                elif score_mode == "max":
                    nxt = np.where(x > acc, x, acc)
                else:
                    nxt = np.where(x < acc, x, acc)
                nxt = np.where(seen, nxt, x)
                acc = np.where(applies, nxt, acc)
                wsum = np.where(applies, wsum + np.float64(fn.get("weight", 1.0)), wsum)
            seen = seen | applies
        with np.errstate(all="ignore"):
            val = acc / wsum if score_mode == "avg" else acc
            val = np.where(val > cap, cap, val)
        out[q] = np.where(seen, val, 1.0)
    if as_f64:
        return out
    with np.errstate(all="ignore"):
        return out.astype(np.float32)


def libm_cells(functions, cols, n, n_fn=1, filters=None):
    """bool [n_fn, n]: the cells some exp / logarithm function applies to (may differ from the device's by one fp32 ulp)."""
    out = np.zeros((n_fn, n), dtype=bool)
    for fn in functions:
        if not through_libm(fn):
            continue
        _, applies = fn_value(fn, cols, n)
        if fn.get("filter") is not None:
            applies = applies & np.asarray(filters[int(fn["filter"])][:n], dtype=bool)
        out[int(fn.get("query", 0))] |= applies
    return out


def ulp_distance(a, b):
    """Distance in fp32 representable values between two float32 arrays; NaN against NaN is 0, a NaN against anything else
    is a huge number."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)

    d = np.abs(key(a) - key(b))
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    bad = np.isnan(a) != np.isnan(b)
    return np.where(same, 0, np.where(bad, 1 << 40, d))


# ---- the scan, float32
def combine(a, f, mode):
    """fused = combine(a, f): separately rounded fp32 operations; max / min as a compare and a select."""
    a, f = np.asarray(a, dtype=np.float32), np.asarray(f, dtype=np.float32)
    with np.errstate(all="ignore"):
        if mode == "sum":
            return (a + f).astype(np.float32)
        if mode == "multiply":
            return (a * f).astype(np.float32)
        if mode == "avg":
            return ((a + f).astype(np.float32) * np.float32(0.5)).astype(np.float32)
        if mode == "max":
            return np.where(f > a, f, a).astype(np.float32)
        if mode == "min":
            return np.where(f < a, f, a).astype(np.float32)
        if mode == "replace":
            return f.copy()
    raise ValueError(mode)


def fused_scores(s, boost, f, transform=0, mode="multiply"):
    """(t, fused) over one query's rows."""
    t = B.transform(s, transform)
    with np.errstate(all="ignore"):
        a = (np.float32(boost) * t).astype(np.float32)
    return t, combine(a, f, mode)


def search(scores, k, column, boost=None, transform=0, mode="multiply", min_score=None, live=None):
    """The whole answer.  ``scores`` [nq, n]: the cosines as the scan computes them; ``column`` [n] shared or [nq, n];
    ``boost`` [nq] or None (1.0); ``min_score`` [nq] or None (no gate); ``live`` bool [n] or [nq, n] or None."""
    scores = np.asarray(scores, dtype=np.float32)
    nq, n = scores.shape
    col = np.asarray(column, dtype=np.float32)
    out_s = np.full((nq, k), NEG_INF, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        f = (col if col.ndim == 1 else col[q])[:n]
        lv = np.ones(n, dtype=bool) if live is None else np.asarray(live if np.ndim(live) == 1 else live[q], dtype=bool)
        t, fused = fused_scores(scores[q], 1.0 if boost is None else boost[q], f, transform, mode)
        with np.errstate(invalid="ignore"):
            ok = lv & (f > NEG_INF)
            if min_score is not None:
                ok = ok & (t >= np.float32(min_score[q]))
            else:
                ok = ok & (t >= NEG_INF)
        out_s[q], out_i[q] = B.rank(scores[q], fused, ok, k)
    return out_s, out_i
