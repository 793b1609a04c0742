"""Function-score search against the CPU oracle: ``rass_index_search_scored(_device)`` and ``rass_index_fn_from_attr``.

The expected answer of a search is always ``fscore_ref`` (a numpy fp32 restatement: every operation rounded on its own, max /
min as compare and select, the gate, the exclusion rules, ties by id) over ``oracle.scores(KIND_F32_MFMA)`` for the queries
as the GPU normalised them; never the engine's own top-k.  Ids and scores must be EQUAL: no tolerance in any ranking assertion.

The builder is read back and compared against the fp64 restatement: cells built from + - * / sqrt, max / min and comparisons
must be EQUAL; cells through exp or a logarithm may differ by at most 1 fp32 ulp — derived, not measured: the two fp64 values
differ by a few fp64 ulps (two libm's, |argument| <= 745), five orders of magnitude below half an fp32 ulp, so after the one
rounding they are equal or adjacent.  Wherever a search test uses the builder it takes the device-built column read back, so
that allowance never reaches a ranking assertion.

Shapes are the boosted tests': n = 20, 1 000 and 4 128 at dims 128 and 1024; every row-stride class at n = 1 000 with nq 5
and 32; nq = 1, 5, 32, 33, 70; k = 1, 10, 32, 100; tombstones and masked tag filters as there.  Worlds are built once.
"""
import ctypes
import datetime as dt
import itertools

import numpy as np
import pytest

import attr_ref as AR
import boost_ref as B
import fscore_ref as F
from test_gpu_boost_search import (KINDS, KS, NOW, NQ_MAX, NQS, ORACLE_MAX_K, SHAPES, STRIDE_DIMS, World, _corpus, assert_same, deep_rows,
                                    filters)

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
ERR_INVALID, ERR_UNSUPPORTED = -1, -5     # rass_status in include/rass_engine.h
MODES = F.COMBINE
TRANSFORMS = ("raw", "opensearch")


def check(w, nq, k, column, mode, boost=None, transform="raw", gate=None, qfilter=None, qmask=None, what="", entries=(False, True)):
    """Host and device entry points against the restatement; returns the expected answer."""
    col = np.asarray(column, dtype=np.float32)
    col = col if col.ndim == 1 else col[:nq]
    bst = None if boost is None else np.asarray(boost, dtype=np.float32)[:nq]
    gt = None if gate is None else np.asarray(gate, dtype=np.float32)[:nq]
    f = None if qfilter is None else qfilter[:nq]
    m = None if qmask is None else qmask[:nq]
    want = F.search(w.scores[:nq], k, col, bst, transform, mode, gt, w.live(nq, f, m))
    d_block = w.torch.from_numpy(w.column(col)).cuda()      # the padding past n is poison
    for on_device in entries:
        got = w.idx.search_scored(w.q_raw[:nq], k, d_block, boost=bst, transform=transform, combine=mode, min_score=gt, q_filter=f,
                                  q_filter_mask=m, on_device=on_device)
        assert_same(got, want, (what, mode, "device" if on_device else "host", w.n, w.dim, nq, k, transform))
    return want


@pytest.fixture(scope="module")
def worlds(gpu, oracle):
    made = {}

    def get(n, dim):
        if (n, dim) not in made:
            made[(n, dim)] = World(gpu, oracle, n, dim, name="fscore")
        return made[(n, dim)]

    yield get
    for w in made.values():
        w.eng.close()


def random_boosts(rng):
    b = rng.uniform(-2.0, 2.0, size=NQ_MAX).astype(np.float32)
    b[1], b[3], b[34] = 0.0, -1.0, 0.0
    return b


# ---- 1. every combine mode on dense random columns of both signs: per query and shared, both transforms, random boosts
@pytest.mark.parametrize("n,dim", SHAPES)
def test_every_mode_on_dense_columns(worlds, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(1021 + n + dim)
    per_query = (rng.standard_normal((NQ_MAX, n)) * 0.5).astype(np.float32)
    boost = random_boosts(rng)
    for i, (nq, k) in enumerate(itertools.product(NQS, KS)):      # every (nq, k) under a rotating mode and transform
        mode, tr = MODES[i % 6], TRANSFORMS[(i // 6) % 2]
        check(w, nq, k, per_query, mode, boost=boost, transform=tr, what="per-query")
        check(w, nq, k, per_query[3], MODES[(i + 3) % 6], boost=boost, transform=TRANSFORMS[(i // 3) % 2], what="shared")
    for mode, tr in itertools.product(MODES, TRANSFORMS):           # every mode x transform at two launch groups
        check(w, 33, 10, per_query, mode, boost=boost, transform=tr, what="all modes")
        check(w, 5, 32, per_query[1], mode, boost=None, transform=tr, what="all modes shared, boost 1")
    qf, qm = filters(w, NQ_MAX)
    for i, (nq, k) in enumerate(((5, 10), (33, 100), (33, 10), (5, 100), (70, 32), (32, 1))):
        check(w, nq, k, per_query, MODES[i], boost=boost, qfilter=qf, qmask=qm, transform=TRANSFORMS[i % 2], what="masked filter")
        check(w, nq, k, per_query[0], MODES[5 - i], qfilter=np.where(qm == -1, qf, -1).astype(np.int32), what="exact filter")


@pytest.mark.parametrize("dim", STRIDE_DIMS)
def test_every_stride_class(worlds, dim):
    w = worlds(1000, dim)
    rng = np.random.default_rng(1031 + dim)
    per_query = (rng.standard_normal((32, 1000)) * 0.5).astype(np.float32)
    boost = rng.uniform(-2.0, 2.0, size=32).astype(np.float32)
    gate = np.where(np.arange(32) % 2 == 0, NEG_INF, np.float32(0.0)).astype(np.float32)
    for i, mode in enumerate(MODES):
        for nq in (5, 32):
            check(w, nq, 10 if i % 2 else 32, per_query, mode, boost=boost, transform=TRANSFORMS[i % 2], gate=gate, what="stride")


# ---- 2. -inf and NaN cells exclude the row in every mode, max and replace included
def test_nonfinite_cells_exclude_in_every_mode(worlds):
    w = worlds(1000, 128)
    rng = np.random.default_rng(1051)
    per_query = (rng.standard_normal((NQ_MAX, 1000)) * 0.5).astype(np.float32)
    per_query[rng.random((NQ_MAX, 1000)) < 0.3] = NEG_INF
    per_query[rng.random((NQ_MAX, 1000)) < 0.1] = np.nan
    per_query[2] = NEG_INF                      # a query with every row excluded: the empty answer
    per_query[40] = np.nan
    per_query[4, 100:] = NEG_INF                # fewer than k rows left
    boost = random_boosts(rng)
    excluded = ~(per_query > NEG_INF)
    for mode in MODES:
        for nq, k, tr in ((33, 32, "raw"), (70, 100, "opensearch"), (5, 10, "raw")):
            want = check(w, nq, k, per_query, mode, boost=boost, transform=tr, what="non-finite cells")
            assert (want[1][2] == -1).all() and (want[0][2] == NEG_INF).all()
            assert nq <= 40 or (want[1][40] == -1).all()
            for q in range(nq):
                ids = want[1][q][want[1][q] >= 0]
                assert not excluded[q][ids].any()
        shared = per_query[0]
        want = check(w, 33, 100, shared, mode, what="non-finite cells, shared")
        assert not excluded[0][want[1][want[1] >= 0]].any()


# ---- 3. the gate on the transformed similarity
@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
def test_gate_on_the_transformed_similarity(worlds, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(1061 + n)
    per_query = (rng.standard_normal((NQ_MAX, n)) * 0.5).astype(np.float32)
    live = w.tags != -1
    for tr in TRANSFORMS:
        t = B.transform(w.scores, tr)
        pivot = np.zeros(NQ_MAX, dtype=np.int64)
        gate = np.full(NQ_MAX, NEG_INF, dtype=np.float32)
        for q in range(NQ_MAX):
            order = np.argsort(-np.where(live, t[q], -np.inf), kind="stable")
            pivot[q] = order[7]                                     # the 8th most similar live row
            own = t[q, pivot[q]]
            gate[q] = (own, np.nextafter(own, np.float32(np.inf)), np.float32(10.0), NEG_INF)[q % 4]
        zero = np.zeros(n, dtype=np.float32)
        for nq in (5, 32, 33):
            want = check(w, nq, 100, zero, "sum", transform=tr, gate=gate, what="gate, fused = t")
            for q in range(nq):
                ids = want[1][q][want[1][q] >= 0]
                if q % 4 == 0:
                    assert pivot[q] in ids and len(ids) >= 8        # a gate equal to a row's own t keeps the row
                elif q % 4 == 1:
                    assert pivot[q] not in ids and len(ids) >= 1    # one ulp above: the row goes
                elif q % 4 == 2:
                    assert len(ids) == 0 and (want[0][q] == NEG_INF).all()
                else:
                    assert len(ids) == min(100, int(live.sum()))
            for i, mode in enumerate(MODES):                        # the gate is on t whatever the fused score is
                check(w, nq, (10, 100)[i % 2], per_query, mode, boost=random_boosts(rng), transform=tr, gate=gate, what="gate")


# ---- 4. replace over three distinct values: ties across workgroups and across chained passes
@pytest.mark.parametrize("dim", [128, 1024])
def test_replace_over_three_values(worlds, dim):
    w = worlds(4128, dim)
    three = (np.arange(4128) % 3).astype(np.float32)
    for nq in (5, 33):
        want = check(w, nq, 100, three, "replace", what="three levels")
        live_top = np.flatnonzero((w.tags != -1) & (three == 2))[:100]
        assert np.array_equal(want[1][0], live_top) and (want[0][0] == 2).all()
        per_query = np.stack([(np.arange(4128) + q) % 3 for q in range(NQ_MAX)]).astype(np.float32)
        check(w, nq, 100, per_query, "replace", gate=np.zeros(NQ_MAX, dtype=np.float32), what="three levels, gated, per-query")


# ---- 5. cross-checks against code that exists
@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
def test_sum_is_the_boosted_search_and_ones_is_the_plain_search(worlds, oracle, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(1071 + n)
    per_query = (rng.standard_normal((NQ_MAX, n)) * 0.05).astype(np.float32)
    boost = random_boosts(rng)
    for nq, k in ((5, 10), (33, 100)):
        block = w.torch.from_numpy(w.column(per_query[:nq])).cuda()
        for tr in TRANSFORMS:
            a = w.idx.search_scored(w.q_raw[:nq], k, block, boost=boost[:nq], transform=tr, combine="sum")
            b = w.idx.search_boosted(w.q_raw[:nq], k, block, boost=boost[:nq], transform=tr, bonus_rows=n)
            assert_same(a, b, ("sum == boosted", n, dim, nq, k, tr))
        want = check(w, nq, k, np.ones(n, dtype=np.float32), "multiply", what="ones")
        ko = max(1, min(k, ORACLE_MAX_K))
        s_o, i_o = oracle.search(w.xn, w.qn_gpu[:nq], ko, kind=oracle.KIND_F32_MFMA, tags=w.tags)
        assert np.array_equal(i_o[:, :ko], want[1][:, :ko]) and np.array_equal(s_o[:, :ko].astype(np.float32), want[0][:, :ko])


# ---- 6. refusals leave the outputs alone
def test_refusals(gpu, worlds):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    w = worlds(1000, 128)
    L = N.lib()
    q = np.ascontiguousarray(w.q_raw[:5])
    block = w.idx.new_bonus(5)
    stride = int(block.shape[1])

    def ptr(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def native(idx, nq, k, n_fn, boost=None, transform=0, combine=1, gate=None, rows=1000):
        out_s = np.full((max(nq, 1), max(k, 1)), 7.0, dtype=np.float32)
        out_i = np.full((max(nq, 1), max(k, 1)), 7, dtype=np.int64)
        b = None if boost is None else np.ascontiguousarray(boost, dtype=np.float32)
        g = None if gate is None else np.ascontiguousarray(gate, dtype=np.float32)
        rc = L.rass_index_search_scored(idx._h, ptr(q), nq, k, ptr(b), transform, combine, ptr(g), ctypes.c_void_p(block.data_ptr()), n_fn,
                                        rows, stride, None, None, ptr(out_s), ptr(out_i))
        assert (out_s == 7.0).all() and (out_i == 7).all()
        return rc

    assert native(w.idx, 5, 10, 5, rows=999) == ERR_INVALID          # the column is short of the index
    assert native(w.idx, 5, 10, 5, rows=1001) == ERR_INVALID
    assert native(w.idx, 5, 10, 5, rows=0) == ERR_INVALID
    d_q = gpu.from_numpy(q).cuda()
    d_s = gpu.full((5, 10), 7.0, dtype=gpu.float32, device="cuda")
    d_i = gpu.full((5, 10), 7, dtype=gpu.int64, device="cuda")
    gpu.cuda.synchronize()
    with pytest.raises(N.RassError):
        w.idx.search_scored_device(d_q.data_ptr(), 5, 10, block.data_ptr(), 5, 999, stride, d_s.data_ptr(), d_i.data_ptr())
    w.eng.synchronize()
    assert (d_s == 7.0).all() and (d_i == 7).all()
    assert native(w.idx, 5, 10, 3) < 0                # n_fn neither 1 nor nq
    assert native(w.idx, 5, 0, 5) < 0 and native(w.idx, 5, 4097, 5) < 0
    assert native(w.idx, 5, 10, 5, boost=[1, 2, np.inf, 4, 5]) < 0
    assert native(w.idx, 5, 10, 5, gate=[0, 0, np.nan, 0, 0]) == ERR_INVALID
    assert native(w.idx, 5, 10, 5, transform=2) < 0
    assert native(w.idx, 5, 10, 5, combine=6) < 0 and native(w.idx, 5, 10, 5, combine=-1) < 0
    with pytest.raises(ValueError):
        w.idx.search_scored(q, 10, block, combine="product")
    with pytest.raises(ValueError):
        w.idx.search_scored(q, 10, block, min_score=[0, 0, np.nan, 0, 0])
    for dim, dtype in ((1536, "f32"), (256, "bf16")):
        eng = Engine(0, dim)
        try:
            idx = eng.open_index("refuse", dtype=dtype)
            idx.add(np.random.default_rng(9).standard_normal((1000, dim), dtype=np.float32))
            q = np.ascontiguousarray(np.ones((5, dim), dtype=np.float32))
            assert native(idx, 5, 10, 5) == ERR_UNSUPPORTED, (dim, dtype)
            with pytest.raises(ValueError):
                idx.search_scored(q, 10, block)
        finally:
            eng.close()


# ---- 7. the builder against the fp64 restatement
DAY0 = (dt.date(2024, 2, 29) - dt.date(1970, 1, 1)).days
ORIGIN, OFFSET = float(DAY0 - 100), 7.0


def attr_world(w):
    """Attribute columns on a world, once: 0 dates as days (with values at origin +- offset exactly), 3 ints of both signs
    and zero, 7 positive ints; each with missing values.  Column 5 is never set."""
    if not hasattr(w, "fcols"):
        rng = np.random.default_rng(1081 + w.n)
        n = w.n
        days = rng.integers(DAY0 - 700, DAY0 + 1, size=n).astype(np.int64)
        days[:4] = (ORIGIN - OFFSET, ORIGIN + OFFSET, ORIGIN, ORIGIN + OFFSET + 1)
        ints = rng.integers(-50, 50, size=n).astype(np.int64)
        ints[4:7] = (0, -1, 1)
        pos = rng.integers(1, 2000, size=n).astype(np.int64)
        w.fcols = {}
        for c, v in ((0, days), (3, ints), (7, pos)):
            gone = rng.random(n) < 0.1
            gone[:8] = False
            v[gone] = F.ATTR_MISSING
            v[n - 1] = F.ATTR_MISSING
            w.fcols[c] = v
            w.idx.set_attr(c, 0, v.astype(np.int32))
    return w.fcols


EXACT_FNS = [
    {"kind": "linear", "col": 0, "origin": ORIGIN, "scale": 30.0, "offset": OFFSET, "decay": 0.5, "weight": 1.5},
    {"kind": "weight", "weight": 0.75, "filter": 0},
    {"kind": "field_value_factor", "col": 3, "factor": 0.1, "modifier": "none", "weight": -2.0},
    {"kind": "field_value_factor", "col": 3, "factor": 1.7, "modifier": "square", "missing": 3.0, "filter": 1},
    {"kind": "field_value_factor", "col": 7, "factor": 0.37, "modifier": "sqrt"},
    {"kind": "field_value_factor", "col": 3, "factor": 3.0, "modifier": "reciprocal", "weight": 0.3},      # 1 / 0 = inf at value 0
    {"kind": "linear", "col": 3, "origin": 10.0, "scale": 5.0, "offset": 0.0, "decay": 0.9},
    {"kind": "weight", "weight": 4.0, "filter": 2},                                                          # an empty bitmap
    {"kind": "field_value_factor", "col": 5, "factor": 2.0, "missing": None},                               # a column never set
    {"kind": "linear", "col": 7, "origin": 1000.0, "scale": 300.0, "offset": 50.0, "decay": 0.25, "filter": 0},
]
LIBM_FNS = [
    {"kind": "gauss", "col": 0, "origin": ORIGIN, "scale": 30.0, "offset": OFFSET, "decay": 0.5},
    {"kind": "exp", "col": 0, "origin": float(DAY0), "scale": 90.0, "offset": 0.0, "decay": 0.33, "weight": 2.0},
    {"kind": "field_value_factor", "col": 7, "factor": 1.2, "modifier": "log1p", "filter": 1},
    {"kind": "field_value_factor", "col": 3, "factor": 1.0, "modifier": "ln", "weight": 0.5},               # ln of <= 0: -inf / NaN
    {"kind": "field_value_factor", "col": 7, "factor": 0.01, "modifier": "log2p", "missing": 1.0},
    {"kind": "field_value_factor", "col": 7, "factor": 1.0, "modifier": "log"},
    {"kind": "field_value_factor", "col": 7, "factor": 0.5, "modifier": "ln1p"},
    {"kind": "field_value_factor", "col": 7, "factor": 0.5, "modifier": "ln2p"},
    {"kind": "gauss", "col": 3, "origin": 0.0, "scale": 0.5, "offset": 0.0, "decay": 0.01},                 # exp of a large negative
]


def filter_bits(w):
    rng = np.random.default_rng(1082 + w.n)
    bits = np.stack([rng.random(w.n) < 0.5, rng.random(w.n) < 0.2, np.zeros(w.n, dtype=bool)])
    return bits


def build_both(w, fns, n_fn, score_mode, max_boost=None):
    """(device column read back [n_fn, n], restatement [n_fn, n], libm cells) for `fns` given per query."""
    from rassengine_amd.engine import pack_allow
    cols, bits = attr_world(w), filter_bits(w)
    d_bits = w.torch.from_numpy(pack_allow(bits).view(np.int32)).cuda()
    block = w.idx.new_bonus(None if n_fn is None else n_fn)
    block.fill_(123.0)
    w.idx.fn_from_attr(block, fns, score_mode=score_mode, max_boost=max_boost, filters=d_bits)
    w.eng.synchronize()
    got = block.cpu().numpy().reshape(n_fn or 1, -1)
    assert (got[:, w.n:] == 123.0).all()                         # the padding is left alone
    want = F.build_column(fns, cols, w.n, n_fn or 1, score_mode, max_boost, bits)
    return got[:, :w.n], want, F.libm_cells(fns, cols, w.n, n_fn or 1, bits)


def same_cells(got, want):
    """bool: the same float32 word, or NaN on both sides (which NaN an invalid operation yields is the platform's)."""
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def spread(fns, counts, rng):
    """Functions for len(counts) queries: query q gets counts[q] of `fns` (cycled from a random start), interleaved."""
    out = []
    for q, c in enumerate(counts):
        at = int(rng.integers(len(fns)))
        out += [dict(fns[(at + j) % len(fns)], query=q) for j in range(c)]
    return [out[i] for i in rng.permutation(len(out))]


@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
@pytest.mark.parametrize("score_mode", F.SCORE_MODES)
def test_builder_exact_cells_equal_the_restatement(worlds, n, dim, score_mode):
    w = worlds(n, dim)
    rng = np.random.default_rng(1083 + n)
    for n_fn in (None, 1, 5, 33):
        counts = [(0, 1, 3, F.MAX_SCORE_FNS)[(q + 1) % 4] for q in range(n_fn or 1)]
        counts[0] = 3 if n_fn is None else counts[0]
        fns = spread(EXACT_FNS, counts, rng)
        for cap in (None, 1.25):
            got, want, libm = build_both(w, fns, n_fn, score_mode, cap)
            assert not libm.any()
            same = same_cells(got, want)
            assert same.all(), (n_fn, score_mode, cap, np.argwhere(~same)[:5], got[~same][:5], want[~same][:5])
            assert cap is None or not (got > np.float32(cap)).any()
        no_fn = [q for q, c in enumerate(counts) if c == 0]
        assert all((got[q] == 1.0).all() for q in no_fn)        # a row no function applies to gets 1.0


@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
@pytest.mark.parametrize("score_mode", F.SCORE_MODES)
def test_builder_libm_cells_within_one_ulp(worlds, n, dim, score_mode):
    w = worlds(n, dim)
    rng = np.random.default_rng(1084 + n)
    differing = 0
    for n_fn in (None, 5, 33):
        counts = [(3, 1, F.MAX_SCORE_FNS, 0)[q % 4] for q in range(n_fn or 1)]
        fns = spread(LIBM_FNS + EXACT_FNS, counts, rng)
        fns[0] = dict(LIBM_FNS[0], query=fns[0]["query"])
        got, want, libm = build_both(w, fns, n_fn, score_mode, 50.0)
        assert libm.any()
        dist = F.ulp_distance(got, want)
        differing += int((dist != 0).sum())
        same = same_cells(got, want)
        assert same[~libm].all(), (n_fn, score_mode, np.argwhere(~same & ~libm)[:5])
        assert (dist <= 1).all(), (n_fn, score_mode, int(dist.max()), np.argwhere(dist > 1)[:5])
    print("builder %s n=%d: %d cells differ from the fp64 restatement by one fp32 ulp" % (score_mode, n, differing))


def test_builder_hand_values_and_missing(worlds):
    w = worlds(1000, 128)
    cols = attr_world(w)
    got, want, _ = build_both(w, [{"kind": "gauss", "col": 0, "origin": ORIGIN, "scale": 30.0, "offset": OFFSET, "decay": 0.5}], None, "multiply")
    live = cols[0] != F.ATTR_MISSING
    assert (got[0][:3] == 1.0).all()                              # at origin +- offset and at the origin: d = 0
    assert (got[0][~live] == 1.0).all()                           # decay on a missing field: 1.0
    assert got[0][3] < 1.0 and (got[0][live] >= 0).all() and (got[0][live] <= 1).all()
    got, _, _ = build_both(w, [{"kind": "field_value_factor", "col": 0, "factor": 1.0}], None, "first")
    assert np.array_equal(got[0][live], cols[0][live].astype(np.float32)) and (got[0][~live] == 1.0).all()


def test_builder_refusals_leave_the_block_untouched(worlds):
    from rassengine_amd import _native as N
    w = worlds(1000, 128)
    attr_world(w)
    block = w.idx.new_bonus(34)         # two launch groups: a refusal in the second must not leave the first written
    block.fill_(5.0)
    good = {"kind": "gauss", "col": 0, "origin": 0.0, "scale": 1.0, "offset": 0.0, "decay": 0.5}
    bad = [dict(good, scale=0.0), dict(good, scale=-1.0), dict(good, decay=0.0), dict(good, decay=1.0), dict(good, decay=1.5),
           dict(good, decay=-0.5), dict(good, offset=-1.0), dict(good, col=8), dict(good, col=-1), dict(good, query=34),
           dict(good, query=-1), dict(good, filter=0), dict(good, weight=float("nan")), dict(good, origin=float("inf")),
           {"kind": "field_value_factor", "col": 9, "factor": 1.0}, {"kind": "field_value_factor", "col": 0, "factor": float("nan")}]

    def refused(functions, **kw):
        """The call answers RASS_ERR_INVALID and not one cell of the block has changed."""
        with pytest.raises(N.RassError) as err:
            w.idx.fn_from_attr(block, functions, **kw)
        assert err.value.code == ERR_INVALID, (functions[-1], kw)
        w.eng.synchronize()
        assert (block == 5.0).all(), (functions[-1], kw)

    for fn in bad:
        refused([dict(good, query=0), dict(good, query=1), dict({"query": 33}, **fn)])     # good functions in group 0, the bad one in group 1
        refused([dict({"query": 0}, **fn)])
    refused([dict(good, query=33)] * (F.MAX_SCORE_FNS + 1))                                 # too many functions for one query
    refused([good] * F.MAX_SCORE_FNS + [dict(good, query=33)] * (F.MAX_SCORE_FNS + 1))
    refused([good], max_boost=float("nan"))
    with pytest.raises(ValueError):
        w.idx.fn_from_attr(block, [good], score_mode="median")
    w.eng.synchronize()
    assert (block == 5.0).all()
    w.idx.fn_from_attr(block, [good] * F.MAX_SCORE_FNS + [dict(good, query=33)] * F.MAX_SCORE_FNS)   # the limit is per query
    w.eng.synchronize()
    assert not (block[0, :1000] == 5.0).any() and not (block[33, :1000] == 5.0).any() and (block[:, 1000:] == 5.0).all()


# ---- 8. a device-built column, read back, through every mode of the scan
@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
def test_search_over_device_built_columns(worlds, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(1091 + n)
    fns = spread(LIBM_FNS + EXACT_FNS, [3] * 33, rng)
    got, _, _ = build_both(w, fns, 33, "sum", 50.0)              # holds -inf / NaN cells (ln of <= 0) and inf (1 / 0)
    got = np.where(np.isposinf(got), np.float32(3.0), got)       # +inf is out of the search's scope
    boost = random_boosts(rng)
    for i, mode in enumerate(MODES):
        check(w, 33, (10, 100)[i % 2], got, mode, boost=boost, transform=TRANSFORMS[i % 2], gate=np.full(NQ_MAX, 0.4, dtype=np.float32)
              if i % 3 == 0 else None, what="device-built column")
    from rassengine_amd.engine import pack_allow
    bits = rng.random(n) < 0.3                                    # a `where` bitmap composes in every mode through bonus_mask
    block = w.torch.from_numpy(w.column(got[0])).cuda()
    w.idx.bonus_mask(block, w.torch.from_numpy(pack_allow(bits[None, :]).view(np.int32)[0].copy()).cuda())
    w.eng.synchronize()
    masked = block.cpu().numpy()[:n]
    assert (masked[~bits] == NEG_INF).all()
    for mode in MODES:
        want = check(w, 5, 32, masked, mode, what="masked column")
        assert bits[want[1][want[1] >= 0]].all()


# ---- 9. the shim
def test_shim_scored_and_recent(gpu, oracle, monkeypatch):
    from rassengine_amd import config, indexer, ops
    from rassengine_amd.attrfilter import compile_functions, run_plan
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,chunkDate:date,pages:int")
    eng = Engine(0, 128)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: eng.open_index(name))
    try:
        rng = np.random.default_rng(1101)
        name = "rass-idx-fscore"
        docs = _corpus(rng)
        emb = rng.standard_normal((300, 128), dtype=np.float32)
        indexer.add_documents(name, docs[:280], emb[:280])
        over = [dict(docs[i], resourceType="Encounter", pages=int(i % 40), chunkDate="2023-09-09") for i in range(40, 60)]
        for d in over:
            docs[int(d["doc_id"][1:])] = d
        indexer.add_documents(name, docs[280:] + over, np.concatenate([emb[280:], emb[40:60]]))
        st = REGISTRY.get(name)
        st.attrs.clock = lambda: NOW
        rows = st.index.rows
        assert rows == 320 and st.index.count == 300
        hip = indexer.HipIndexer(None, name)
        q = rng.standard_normal(128).astype(np.float32)
        xn = st.index.get_rows(0, rows)
        qn = ops.normalize_rows(gpu.from_numpy(q[None, :]).cuda()).cpu().numpy()
        cos = oracle.scores(np.ascontiguousarray(xn, dtype=np.float32), qn, kind=oracle.KIND_F32_MFMA).astype(np.float32)[0]
        live = np.array([d is not None for d in st.row_doc])
        days = np.array([F.ATTR_MISSING if d is None or "chunkDate" not in d else (dt.date.fromisoformat(d["chunkDate"]) - dt.date(1970, 1, 1)).days
                         for d in st.row_doc], dtype=np.int64)

        def ids(res):
            return [(d["doc_id"], s) for d, s in res]

        def want(k, column, mode, transform, keep, gate=None, boost=1.0):
            s, i = F.search(cos[None, :], k, column, np.array([boost], dtype=np.float32), transform, mode,
                            None if gate is None else np.array([gate], dtype=np.float32), live & keep)
            return [(st.row_doc[r]["doc_id"], float(v)) for v, r in zip(s[0], i[0]) if r >= 0]

        # a gauss decay on the date, worth double for Conditions, under a `where` and a patient
        functions = [{"gauss": {"chunkDate": {"origin": "now-30d/d", "scale": "120d", "offset": "7d", "decay": 0.5}}},
                     {"filter": {"term": {"resourceType": "Condition"}}, "weight": 2.0}]
        where = {"bool": {"must_not": {"term": {"resourceType": "Encounter"}}}}
        keep = np.array([d is not None and AR.doc_matches(where, d, KINDS, NOW) and d["patientId"] == "p1" for d in st.row_doc])
        records, flts = compile_functions(functions, st.attrs, st.patients, st.doc_types)
        assert records[0]["origin"] == float(DAY0 - 30) and records[0]["scale"] == 120.0 and records[0]["offset"] == 7.0
        bitmaps = gpu.stack([run_plan(st.index, plan) for plan in flts])
        column = st.index.fn_from_attr(st.index.new_bonus(), records, score_mode="multiply", filters=bitmaps)
        eng.synchronize()
        column = column.cpu().numpy()[:rows]                       # the device-built column, read back
        cond = np.array([d is not None and d.get("resourceType") == "Condition" for d in st.row_doc])
        ref_col = F.build_column(records, {1: days}, rows, 1, "multiply", None, cond[None, :])[0]
        assert (F.ulp_distance(column, ref_col)[live] <= 1).all()
        for boost_mode, sm, tr in (("multiply", None, "opensearch"), ("sum", "cosine", "raw"), ("max", "cosine", "raw")):
            got = hip.semantic_search_scored(q, k=40, functions=functions, boost_mode=boost_mode, boost=1.5, where=where,
                                             patient_id="p1", knn_score_mode=sm, min_score=0.0 if sm else 0.45)
            assert got and ids(got) == want(40, column, boost_mode, tr, keep, 0.0 if sm else 0.45, 1.5), boost_mode
        assert hip.semantic_search_scored(q, k=5, functions=[{"gauss": {"chunkDate": {"scale": "12h"}}}]) == []
        assert hip.semantic_search_scored(q, k=5, functions=[{"script_score": {}}]) == []
        # the k most recent (earliest) chunks among those at least this similar
        gate = float(np.sort(B.transform(cos, 1)[live])[-120])
        dated = days != F.ATTR_MISSING
        fdays = np.where(dated, days, 0).astype(np.float32)
        for order, sign in (("desc", 1.0), ("asc", -1.0)):
            col = (np.float32(sign) * fdays).astype(np.float32)
            got = hip.semantic_search_recent(q, k=50, field="chunkDate", min_score=gate, order=order)
            exp = want(50, np.where(dated, col, NEG_INF), "replace", 1, np.ones(rows, dtype=bool), gate)
            assert len(got) == 50 and ids(got) == [(d, sign * s) for d, s in exp], order
            vals = [s for _, s in got]
            assert vals == sorted(vals, reverse=order == "desc")
            got = hip.semantic_search_recent(q, k=200, field="chunkDate", min_score=gate, order=order, missing="_last")
            exp = want(200, np.where(dated, col, np.float32(-(1 << 24))), "replace", 1, np.ones(rows, dtype=bool), gate)
            assert len(got) == len(exp) == 120
            assert [d for d, _ in ids(got)] == [d for d, _ in exp], order
            tail = [s for _, s in got if np.isnan(s)]
            assert tail and all(np.isnan(s) for _, s in got[-len(tail):]) and not any(np.isnan(s) for _, s in got[:-len(tail)])
        assert hip.semantic_search_recent(q, k=5, field="resourceType") == []
        assert hip.semantic_search_recent(q, k=5, field="chunkDate", order="sideways") == []
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()


# ---- 9. the loop's steady state: three iterations per workgroup (the boosted tests' deep shape)
@pytest.mark.parametrize("nq", [16, 17])
@pytest.mark.parametrize("dim", [128, 1024])
def test_deep_loop_parks_each_pair_for_its_own_tiles(gpu, worlds, dim, nq):
    n = deep_rows(gpu)
    w = worlds(n, dim)
    rng = np.random.default_rng(1111 + dim)
    # one column per query, every row its own value (replace ranks by it alone; multiply by it times the similarity)
    per_query = ((rng.permutation(NQ_MAX * n).reshape(NQ_MAX, n) + 1) * (2.0 / (NQ_MAX * n))).astype(np.float32)
    assert all(len(np.unique(per_query[q])) == n for q in range(nq))
    boost = random_boosts(rng)
    gate = np.where(np.arange(NQ_MAX) % 2 == 0, np.float32(0.0), NEG_INF).astype(np.float32)     # every other query gated
    check(w, nq, 10, per_query, "multiply", boost=boost, transform="opensearch", what="deep multiply")
    want = check(w, nq, 10, per_query, "replace", boost=boost, transform="raw", gate=gate, what="deep replace, gated")
    cus = gpu.cuda.get_device_properties(0).multi_processor_count
    assert (want[1] >= 0).all() and len(np.unique(want[1] // 32 // cus)) > 1      # hits from more than one round of tiles
