"""Boosted search against the CPU oracle: ``rass_index_search_boosted(_device)`` and the bonus column builders.

The expected answer is always ``boost_ref`` (a numpy fp32 restatement: every operation rounded on its own, ties by id, the
non-finite rule) over ``oracle.scores(KIND_F32_MFMA)`` for the queries as the GPU normalised them; never the engine's own
top-k.  Ids and scores must be EQUAL: no tolerance anywhere in this file.

Shapes: n = 20 (less than a tile), 1 000 (the last tile has 8 rows) and 4 128 (129 tiles) at dims 128 and 1024; every row
stride class 128 .. 1024 at n = 1 000 with nq 5 and 32 (both kernel widths); nq = 1, 5, 32, 33 (a second launch group of one
query) and 70; k = 1, 10, 32 and 100 (four passes chained under the continuation bound on the fused score).  Tombstones as
in the allow-list tests.  Each world (corpus, oracle score matrix, engine, index) is built once for the module.
"""
import ctypes
import datetime as dt

import numpy as np
import pytest

import attr_ref as AR
import boost_ref as B

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
ORACLE_MAX_K = 1024
PATIENT_MASK = 0x00FFFFFF
NQ_MAX = 70
NQS = (1, 5, 32, 33, 70)
KS = (1, 10, 32, 100)
SHAPES = [(20, 128), (1000, 128), (4128, 128), (20, 1024), (1000, 1024), (4128, 1024)]
STRIDE_DIMS = (128, 200, 384, 500, 640, 768, 896, 1024)     # row strides 128, 256, ..., 1024


def stride_of(n):
    return (n + 31) // 32 * 32 + 32


class World:
    """Rows, tags (with tombstones), 70 queries, the oracle's score matrix and a live index holding the rows."""

    def __init__(self, torch, oracle, n, dim, xn=None, name="boost"):
        from rassengine_amd import ops
        from rassengine_amd.engine import Engine
        rng = np.random.default_rng(11000 + n + dim)
        self.torch, self.oracle, self.n, self.dim, self.rng = torch, oracle, n, dim, rng
        self.xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32) if xn is None else xn
        self.q_raw = rng.standard_normal((NQ_MAX, dim), dtype=np.float32) * 3.0     # un-normalised on purpose
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.tags = (rng.integers(0, 5 if n < 100 else 50, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)
        self.dead = sorted({3, n // 2, n - 1, n - 5} if n < 100 else set(rng.choice(n, size=n // 25, replace=False)) | {n - 1, 31, 32})
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.eng = Engine(0, dim)
        self.idx = self.eng.open_index(name)
        self.idx.add(self.xn, tags=self.tags, normalize=False)
        for r in self.dead:
            self.idx.delete(int(r))
        self.tags = self.tags.copy()
        self.tags[self.dead] = -1
        self.stride = stride_of(n)

    def live(self, nq, qfilter=None, qmask=None):
        ok = np.tile(self.tags != -1, (nq, 1))
        if qfilter is not None:
            for q in range(nq):
                if qfilter[q] >= 0:
                    ok[q] &= ((self.tags & qmask[q]) if qmask is not None else self.tags) == qfilter[q]
        return ok

    def column(self, bonus):
        """[n] or [nq, n] values -> the padded block the engine takes ([stride] / [nq, stride]); the padding is poisoned
        with a value that would win every ranking if the kernel read it for a row that does not exist."""
        b = np.asarray(bonus, dtype=np.float32)
        out = np.full(b.shape[:-1] + (self.stride,), 1e9, dtype=np.float32)
        out[..., :self.n] = b
        return out

    def check(self, nq, k, bonus=None, boost=None, mode="raw", qfilter=None, qmask=None, bonus_rows=None, what="", entries=(False, True)):
        """Host and device entry points against the restatement; returns the expected answer."""
        n = self.n
        col = np.zeros(n, dtype=np.float32) if bonus is None else np.asarray(bonus, dtype=np.float32)
        col = col if col.ndim == 1 else col[:nq]
        bst = None if boost is None else np.asarray(boost, dtype=np.float32)[:nq]
        f = None if qfilter is None else qfilter[:nq]
        m = None if qmask is None else qmask[:nq]
        want = B.search(self.scores[:nq], k, bst, col, mode, self.live(nq, f, m), bonus_rows)
        block = self.column(col)
        rows_arg = n if bonus_rows is None else bonus_rows      # (the block's padding past n is poison)
        d_block = self.torch.from_numpy(block).cuda()
        for on_device in entries:
            got = self.idx.search_boosted(self.q_raw[:nq], k, d_block, boost=bst, transform=mode, bonus_rows=rows_arg, q_filter=f,
                                          q_filter_mask=m, on_device=on_device)
            assert_same(got, want, (what, "device" if on_device else "host", n, self.dim, nq, k, mode))
        return want


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids")):
        same = np.array_equal(g, w, equal_nan=False)
        assert same, (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


@pytest.fixture(scope="module")
def worlds(gpu, oracle):
    made = {}

    def get(n, dim):
        if (n, dim) not in made:
            made[(n, dim)] = World(gpu, oracle, n, dim)
        return made[(n, dim)]

    yield get
    for w in made.values():
        w.eng.close()


def filters(w, nq):
    """Per-query filters: exact patient+type, masked patient, none."""
    rng = np.random.default_rng(5 + w.n)
    live_tags = w.tags[w.tags != -1]
    qf = np.full(nq, -1, dtype=np.int32)
    qm = np.full(nq, -1, dtype=np.int32)
    for q in range(nq):
        t = int(live_tags[rng.integers(len(live_tags))])
        if q % 3 == 0:
            qf[q] = t
        elif q % 3 == 1:
            qf[q], qm[q] = t & PATIENT_MASK, PATIENT_MASK
    return qf, qm


# ---- 1. a zero column, boost 1, raw scores: the plain search
@pytest.mark.parametrize("n,dim", SHAPES)
def test_zero_column_is_the_plain_search(worlds, oracle, n, dim):
    w = worlds(n, dim)
    for nq in NQS:
        for k in KS:
            want = w.check(nq, k, what="zero")
            ko = max(1, min(k, n, ORACLE_MAX_K))
            s_o, i_o = oracle.search(w.xn, w.qn_gpu[:nq], ko, kind=oracle.KIND_F32_MFMA, tags=w.tags)
            assert np.array_equal(i_o[:, :ko], want[1][:, :ko]) and np.array_equal(s_o[:, :ko].astype(np.float32), want[0][:, :ko])


# ---- 2. dense random columns: per query and shared, with filters, host and device
@pytest.mark.parametrize("n,dim", SHAPES)
def test_dense_random_column(worlds, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(21 + n + dim)
    per_query = (rng.standard_normal((NQ_MAX, n)) * 0.05).astype(np.float32)
    plain = B.search(w.scores[:5], 10, None, None, 0, w.live(5))
    changed = B.search(w.scores[:5], 10, None, per_query[:5], 0, w.live(5))
    assert n < 100 or not np.array_equal(plain[1], changed[1])      # sigma 0.05 really changes the ranking
    for nq in NQS:
        for k in KS:
            w.check(nq, k, per_query, what="per-query")
            w.check(nq, k, per_query[3], what="shared")
    qf, qm = filters(w, NQ_MAX)
    for nq in (5, 33):
        for k in (10, 100):
            w.check(nq, k, per_query, qfilter=qf, qmask=qm, what="masked filter")
            w.check(nq, k, per_query[0], qfilter=np.where(qm == -1, qf, -1).astype(np.int32), what="exact filter")


@pytest.mark.parametrize("dim", STRIDE_DIMS)
def test_every_stride_class(worlds, dim):
    w = worlds(1000, dim)
    rng = np.random.default_rng(31 + dim)
    per_query = (rng.standard_normal((32, 1000)) * 0.05).astype(np.float32)
    boost = rng.uniform(-2.0, 2.0, size=32).astype(np.float32)
    for nq in (5, 32):
        w.check(nq, 10, per_query, what="stride")
        w.check(nq, 32, per_query, boost=boost, mode="opensearch", what="stride, opensearch")


# ---- 3. boost 0: every live row ties at its bonus
@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
def test_boost_zero_orders_by_id(worlds, n, dim):
    w = worlds(n, dim)
    zero = np.zeros(NQ_MAX, dtype=np.float32)
    for nq in (5, 33):
        for k in (10, 100):
            want = w.check(nq, k, None, boost=zero, what="boost 0")
            live_ids = np.flatnonzero(w.tags != -1)[:k]
            assert np.array_equal(want[1][0, :len(live_ids)], live_ids) and (want[0][0, :len(live_ids)] == 0).all()
            three = (np.arange(n) % 3).astype(np.float32)
            w.check(nq, k, three, boost=zero, what="boost 0, three levels")


# ---- 4. fused ties across workgroups: duplicated rows under a two-valued bonus
def test_fused_ties_across_workgroups(gpu, oracle):
    n, dim = 2000, 128
    rng = np.random.default_rng(41)
    base = oracle.normalize_ref(rng.standard_normal((40, dim), dtype=np.float32)).astype(np.float32)
    w = World(gpu, oracle, n, dim, xn=np.ascontiguousarray(base[np.arange(n) % 40]), name="dups")
    try:
        bonus = np.where(rng.random(n) < 0.5, 0.5, 0.0).astype(np.float32)
        per_query = np.where(rng.random((NQ_MAX, n)) < 0.5, 0.5, 0.0).astype(np.float32)
        for nq in (5, 33):
            for k in (10, 32, 100):
                want = w.check(nq, k, bonus, what="dups shared")
                assert k == 1 or (want[0][:, 0] == want[0][:, 1]).all()      # ties at the very top
                w.check(nq, k, per_query, what="dups per-query")
    finally:
        w.eng.close()


# ---- 5. -inf and NaN bonuses exclude; a NaN vector stays out whatever its bonus
def test_nonfinite_bonus_excludes(worlds):
    w = worlds(1000, 128)
    rng = np.random.default_rng(51)
    per_query = (rng.standard_normal((NQ_MAX, 1000)) * 0.05).astype(np.float32)
    per_query[rng.random((NQ_MAX, 1000)) < 0.3] = NEG_INF
    per_query[rng.random((NQ_MAX, 1000)) < 0.1] = np.nan
    per_query[2] = NEG_INF                      # a query with every row excluded: the empty answer
    per_query[40] = np.nan
    per_query[4, 100:] = NEG_INF                # fewer than k rows left
    for nq in (5, 33, 70):
        for k in (10, 100):
            want = w.check(nq, k, per_query, what="non-finite bonus")
            assert (want[1][2] == -1).all() and (want[0][2] == NEG_INF).all()
            assert nq <= 40 or (want[1][40] == -1).all()
    for mode in ("raw", "opensearch"):
        w.check(33, 32, per_query, boost=np.linspace(-1, 1, NQ_MAX).astype(np.float32), mode=mode, what="non-finite, boosted")


def test_nan_vector_never_ranks(gpu, oracle):
    n, dim = 100, 128
    rng = np.random.default_rng(52)
    xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
    xn[17, :] = np.nan
    xn[70, 5] = np.nan
    w = World(gpu, oracle, n, dim, xn=xn, name="nanrow")
    try:
        assert np.isnan(w.scores[:, 17]).all() and np.isnan(w.scores[:, 70]).all()
        bonus = np.zeros(n, dtype=np.float32)
        bonus[17] = 5.0                          # finite and large: only the cosine rule keeps the row out
        for mode in ("raw", "opensearch"):
            for boost in (None, np.zeros(NQ_MAX, dtype=np.float32)):
                want = w.check(5, 100, bonus, boost=boost, mode=mode, what="nan vector")
                assert 17 not in want[1] and 70 not in want[1]
    finally:
        w.eng.close()


# ---- 6. rows past bonus_rows read 0
@pytest.mark.parametrize("n,dim,rows", [(1000, 128, 517), (4128, 1024, 4001), (1000, 128, 0)])
def test_rows_past_bonus_rows_read_zero(worlds, n, dim, rows):
    w = worlds(n, dim)
    per_query = (np.random.default_rng(61).standard_normal((NQ_MAX, n)) * 0.05 + 1.0).astype(np.float32)
    for nq in (5, 33):
        for k in (10, 100):
            w.check(nq, k, per_query, bonus_rows=rows, what="bonus_rows")
            w.check(nq, k, per_query[1], bonus_rows=rows, what="bonus_rows shared")


# ---- 7. the opensearch transform, bit for bit, under negative and fractional boosts
@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
def test_opensearch_transform_is_bit_exact(worlds, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(71)
    boost = np.array([2.0, 1.5, -1.0, 0.3, -0.7, 1.0, 1e-3, 7.25] * 9, dtype=np.float32)[:NQ_MAX]
    per_query = (rng.standard_normal((NQ_MAX, n)) * 0.05).astype(np.float32)
    t = B.transform(w.scores[0], 1)
    assert np.array_equal(t, np.float32(1) / (np.float32(2) - w.scores[0]))
    for nq in (5, 33):
        for k in (10, 100):
            w.check(nq, k, None, boost=None, mode="opensearch", what="opensearch plain")
            w.check(nq, k, per_query, boost=boost, mode="opensearch", what="opensearch boosted")
            w.check(nq, k, per_query, boost=boost, mode="raw", what="raw boosted")


# ---- 8. the builders, word for word
def bits_of(t):
    return t.cpu().numpy().view(np.uint32)


def test_scatter_equals_restatement_and_refuses_duplicates(worlds):
    from rassengine_amd import _native as N
    w = worlds(1000, 128)
    rng = np.random.default_rng(81)
    for nb in (None, 5, 33):
        bonus = w.idx.new_bonus(nb)
        want = np.zeros(tuple(bonus.shape), dtype=np.float32)
        for _ in range(2):      # the second call adds onto the first
            m = 400
            cells = rng.choice((nb or 1) * 1000, size=m, replace=False)
            q_of, rows = (cells // 1000).astype(np.int32), (cells % 1000).astype(np.int64)
            vals = rng.standard_normal(m).astype(np.float32)
            w.idx.bonus_scatter(bonus, q_of, rows, vals)
            B.scatter(want, q_of, rows, vals)
        w.eng.synchronize()
        assert np.array_equal(bonus.cpu().numpy().view(np.uint32), want.view(np.uint32)), nb
    bonus = w.idx.new_bonus(2)
    before = bonus.clone()
    for q_of, rows in (([0, 1, 0], [5, 5, 5]), ([0], [1000]), ([2], [0]), ([0], [-1])):
        with pytest.raises(N.RassError):
            w.idx.bonus_scatter(bonus, q_of, rows, np.ones(len(rows), dtype=np.float32))
    w.eng.synchronize()
    assert w.torch.equal(bonus, before)


@pytest.mark.parametrize("n,dim", [(20, 128), (1000, 128), (4128, 1024)])
@pytest.mark.parametrize("per_q", [0, 1, 8, 64])
def test_clause_builder_equals_restatement(worlds, n, dim, per_q):
    w = worlds(n, dim)
    rng = np.random.default_rng(82 + n + per_q)
    if not hasattr(w, "cols"):
        w.cols = {}
        for c in (0, 3, 7):
            v = rng.integers(-50, 50, size=n).astype(np.int64)
            v[rng.random(n) < 0.1] = B.ATTR_MISSING
            v[:2] = ((1 << 31) - 1, -(1 << 31) + 1)
            w.cols[c] = v
            w.idx.set_attr(c, 0, v.astype(np.int32))
    for nb in (None, 5, 33):
        clauses, weights = [], []
        for q in range(nb or 1):
            for _ in range(per_q):
                lo = int(rng.integers(-60, 40))
                clauses.append((q, int(rng.choice([0, 3, 5, 7])), lo, lo + int(rng.integers(-2, 40)), int(rng.random() < 0.3)))
                weights.append(np.float32(rng.standard_normal() * (10.0 ** rng.integers(-3, 3))))
        order = rng.permutation(len(clauses))      # queries interleaved: each query's own list order is what counts
        clauses, weights = [clauses[i] for i in order], [weights[i] for i in order]
        bonus = w.idx.new_bonus(nb)
        want = np.zeros(tuple(bonus.shape), dtype=np.float32)
        seedv = rng.standard_normal(want.shape).astype(np.float32)
        for op in ("replace", "add", "replace"):
            if op == "add":
                bonus.copy_(w.torch.from_numpy(seedv))
                want[...] = seedv
            w.idx.bonus_from_attr_clauses(bonus, np.array(clauses, dtype=np.int64).reshape(-1, 5), weights, op=op)
            B.from_attr_clauses(want, w.cols, clauses, weights, n, op)
            w.eng.synchronize()
            assert np.array_equal(bonus.cpu().numpy().view(np.uint32), want.view(np.uint32)), (nb, op, per_q)


def test_mask_equals_restatement_and_composes(worlds):
    from rassengine_amd.engine import pack_allow
    w = worlds(1000, 128)
    rng = np.random.default_rng(83)
    for nb, n_bits in ((None, 1), (5, 5), (5, 1), (33, 33)):
        bits = rng.random((n_bits, 1000)) < 0.4
        allow = w.torch.from_numpy(pack_allow(bits).view(np.int32)).cuda()
        allow = allow[0].contiguous() if n_bits == 1 else allow
        seedv = rng.standard_normal(((nb or 1), w.idx.new_bonus().shape[0])).astype(np.float32)
        bonus = w.torch.from_numpy(seedv if nb else seedv[0]).cuda()
        want = seedv.copy()
        w.idx.bonus_mask(bonus, allow)
        B.mask(want, bits, 1000)
        w.eng.synchronize()
        got = bonus.cpu().numpy().reshape(want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (nb, n_bits)
        if nb == 5 and n_bits == 5:     # and the search behind it: only allowed rows rank
            s, i = w.idx.search_boosted(w.q_raw[:5], 100, bonus)
            ref = B.search(w.scores[:5], 100, None, want[:, :1000], 0, w.live(5))
            assert_same((s, i), ref, "masked search")
            assert all(bits[q][i[q][i[q] >= 0]].all() for q in range(5))


# ---- 9. refusals leave the outputs alone
def test_refusals(gpu, worlds):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    w = worlds(1000, 128)
    L = N.lib()
    q = np.ascontiguousarray(w.q_raw[:5])
    bonus = w.idx.new_bonus(5)
    stride = int(bonus.shape[1])

    def native(idx, nq, k, n_bonus, boost=None, transform=0, rows=stride):
        out_s = np.full((max(nq, 1), max(k, 1)), 7.0, dtype=np.float32)
        out_i = np.full((max(nq, 1), max(k, 1)), 7, dtype=np.int64)
        b = None if boost is None else np.ascontiguousarray(boost, dtype=np.float32)
        rc = L.rass_index_search_boosted(idx._h, q.ctypes.data_as(ctypes.c_void_p), nq, k,
                                         None if b is None else b.ctypes.data_as(ctypes.c_void_p), transform,
                                         ctypes.c_void_p(bonus.data_ptr()), n_bonus, rows, stride, None, None,
                                         out_s.ctypes.data_as(ctypes.c_void_p), out_i.ctypes.data_as(ctypes.c_void_p))
        assert (out_s == 7.0).all() and (out_i == 7).all()
        return rc

    assert native(w.idx, 5, 10, 3) < 0                # n_bonus neither 1 nor nq
    assert native(w.idx, 5, 0, 5) < 0 and native(w.idx, 5, 4097, 5) < 0
    assert native(w.idx, 5, 10, 5, boost=[1, 2, np.inf, 4, 5]) < 0 and native(w.idx, 5, 10, 5, boost=[1, np.nan, 3, 4, 5]) < 0
    assert native(w.idx, 5, 10, 5, transform=2) < 0
    assert native(w.idx, 5, 10, 5, rows=stride + 1) < 0
    with pytest.raises(ValueError):
        w.idx.search_boosted(q, 10, w.idx.new_bonus(3))
    with pytest.raises(ValueError):
        w.idx.search_boosted(q, 10, bonus, boost=[1, 2, np.inf, 4, 5])
    for dim, dtype in ((1536, "f32"), (256, "bf16")):
        eng = Engine(0, dim)
        try:
            idx = eng.open_index("refuse", dtype=dtype)
            idx.add(np.random.default_rng(9).standard_normal((64, dim), dtype=np.float32))
            q = np.ascontiguousarray(np.ones((5, dim), dtype=np.float32))
            assert native(idx, 5, 10, 5) < 0, (dim, dtype)
            with pytest.raises(ValueError):
                idx.search_boosted(q, 10, bonus)
        finally:
            eng.close()


# ---- 10. the shim
NOW = dt.datetime(2024, 2, 29, 15, 30, tzinfo=dt.timezone.utc)
KINDS = {"resourceType": "keyword", "chunkDate": "date", "pages": "int", "patientId": "keyword", "doc_type": "keyword"}


def _corpus(rng, n=300):
    types = ["Observation", "Condition", "Encounter", "Procedure"]
    docs = []
    for i in range(n):
        d = {"doc_id": f"d{i}", "doc_type": "note" if i % 5 == 0 else "unstructured", "patientId": f"p{i % 4}"}
        if rng.random() < 0.9:
            d["resourceType"] = types[int(rng.integers(4))]
        if rng.random() < 0.85:
            stamp = dt.datetime(2022, 6, 1, tzinfo=dt.timezone.utc) + dt.timedelta(hours=int(rng.integers(0, 24 * 700)))
            d["chunkDate"] = stamp.date().isoformat()
        if rng.random() < 0.9:
            d["pages"] = int(rng.integers(0, 40))
        docs.append(d)
    return docs


class TextEngine:
    """Stands where the kept text engine stands: every hybrid builder returns the canned ranked list, cut at k."""

    def __init__(self, hits):
        self.hits, self.calls = hits, []

    def _answer(self, query, query_emb, k=3, filter_clause=None, patient_id=None):
        self.calls.append(k)
        return self.hits[:k]

    hybrid_search = hybrid_structured_search = multi_intent_search = _answer


def test_shim_boosted_search_and_exact_hybrid(gpu, oracle, monkeypatch):
    from rassengine_amd import config, indexer, ops
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,chunkDate:date,pages:int")
    eng = Engine(0, 128)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: eng.open_index(name))
    try:
        rng = np.random.default_rng(101)
        name = "rass-idx-boost"
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
        # the restatement's inputs: the index's own rows, the query as the GPU normalises it, the oracle's scores
        xn = st.index.get_rows(0, rows)
        qn = ops.normalize_rows(gpu.from_numpy(q[None, :]).cuda()).cpu().numpy()
        cos = oracle.scores(np.ascontiguousarray(xn, dtype=np.float32), qn, kind=oracle.KIND_F32_MFMA).astype(np.float32)[0]
        live = np.array([d is not None for d in st.row_doc])
        row_of = {d["doc_id"]: r for r, d in enumerate(st.row_doc) if d is not None}

        def want(k, boost, mode, bonus, keep=None):
            lv = live if keep is None else live & keep
            s, i = B.search(cos[None, :], k, np.array([boost], dtype=np.float32), bonus, mode, lv)
            return [(st.row_doc[r]["doc_id"], float(v)) for v, r in zip(s[0], i[0]) if r >= 0]

        def got(res):
            return [(d["doc_id"], s) for d, s in res]

        # text hits deep outside the cosine top-k, a duplicate, an unknown id and an overwritten doc (found at its current row)
        order = np.argsort(-np.where(live, cos, -np.inf))
        deep = [st.row_doc[r]["doc_id"] for r in order[200:206]]
        text = [(deep[0], 0.9), ({"doc_id": deep[1]}, 0.45), (deep[0], 0.35), ("never-indexed", 3.0), ("d45", 0.8), (deep[2], 0.2)]
        bonus = np.zeros(rows, dtype=np.float32)
        for key, s in ((deep[0], np.float32(0.9) + np.float32(0.35)), (deep[1], 0.45), ("d45", 0.8), (deep[2], 0.2)):
            bonus[row_of[key]] = np.float32(s)
        for mode, sm in ((1, "opensearch"), (0, "cosine")):
            for k in (10, 300):
                assert got(hip.semantic_search_boosted(q, k=k, boost=2.0, text_hits=text, score_mode=sm)) == want(k, 2.0, mode, bonus)
        top = got(hip.semantic_search_boosted(q, k=10, boost=2.0, text_hits=text))
        assert deep[0] in [d for d, _ in top] and row_of["d45"] >= 300
        # should-clauses: a recency range worth 0.5 that matches a large share, a negative term, a terms leaf, exists
        should = [({"range": {"chunkDate": {"gte": "now-1y"}}}, 0.5), ({"term": {"resourceType": "Procedure"}}, -0.25),
                  ({"terms": {"resourceType": ["Observation", "Condition", "Nope"]}}, 0.125), ({"exists": {"field": "pages"}}, 0.0625)]
        b2 = bonus.copy()
        for leaf, wgt in should:
            hit = np.array([d is not None and AR.doc_matches(leaf, d, KINDS, NOW) for d in st.row_doc])
            b2 = np.where(hit, (b2 + np.float32(wgt)).astype(np.float32), b2)
        assert got(hip.semantic_search_boosted(q, k=50, boost=1.5, text_hits=text, should=should)) == want(50, 1.5, 1, b2)
        where = {"bool": {"must_not": {"term": {"resourceType": "Encounter"}}}}
        keep = np.array([d is not None and AR.doc_matches(where, d, KINDS, NOW) for d in st.row_doc])
        assert got(hip.semantic_search_boosted(q, k=300, should=should, where=where, patient_id="p1")) == \
            want(300, 1.0, 1, _only_should(st, should), keep & np.array([d is not None and d["patientId"] == "p1" for d in st.row_doc]))
        # refusals are logged and answered with []
        assert hip.semantic_search_boosted(q, k=5, should=[({"term": {"patientId": "p1"}}, 1.0)]) == []
        assert hip.semantic_search_boosted(q, k=5, should=[({"bool": {"must": []}}, 1.0)]) == []
        assert hip.semantic_search_boosted(np.zeros(0, dtype=np.float32), k=5) == []
        # RASS_HYBRID_EXACT: the text hit at cosine rank ~200 is missed by the 4k over-fetch fusion unless its text score alone wins
        engine = TextEngine([({"doc_id": d}, s) for d, s in ((deep[3], 0.30), (deep[4], 0.28))])
        monkeypatch.setattr(indexer.HipIndexer, "_text_engine", lambda self: engine)
        k = 5
        old = got(hip.hybrid_search("x", q, k=k))
        assert engine.calls == [k * indexer.FUSION_OVERFETCH]
        monkeypatch.setattr(config, "RASS_HYBRID_EXACT", True)
        new = got(hip.hybrid_search("x", q, k=k))
        assert engine.calls == [k * indexer.FUSION_OVERFETCH] * 2
        hb = np.zeros(rows, dtype=np.float32)
        hb[row_of[deep[3]]], hb[row_of[deep[4]]] = np.float32(0.30), np.float32(0.28)
        assert new == want(k, 2.0, 1, hb)
        # the old path gave the deep hits their text score alone (no cosine): they rank below every knn hit and miss the top k
        assert deep[3] not in [d for d, _ in old] and deep[3] in [d for d, _ in new]
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()


def _only_should(st, should):
    b = np.zeros(len(st.row_doc), dtype=np.float32)
    for leaf, wgt in should:
        hit = np.array([d is not None and AR.doc_matches(leaf, d, KINDS, NOW) for d in st.row_doc])
        b = np.where(hit, (b + np.float32(wgt)).astype(np.float32), b)
    return b


# ---- 11. the loop's steady state: three iterations per workgroup
def deep_rows(torch):
    """5 * CUs + 3 tiles and a tail of 7 rows (41 063 rows on 256 CUs).  The scan launches one workgroup per CU, so every
    workgroup runs the pair loop three times, some over 5 tiles and some over 6 (odd and even counts): a column value
    requested in one iteration is parked and ranked in the next, the LDS image pair flips twice, and the run-ahead refill goes
    past the last tile.  At the shapes above (<= 129 tiles) every workgroup runs the loop body once."""
    return (5 * torch.cuda.get_device_properties(0).multi_processor_count + 3) * 32 + 7


@pytest.mark.parametrize("nq", [16, 17])
@pytest.mark.parametrize("dim", [128, 1024])
def test_deep_loop_parks_each_pair_for_its_own_tiles(gpu, worlds, dim, nq):
    n = deep_rows(gpu)
    w = worlds(n, dim)
    rng = np.random.default_rng(111 + dim)
    # one column per query, every row its own value: a value parked for the wrong tile, pair or query changes the answer
    per_query = (rng.permutation(NQ_MAX * n).reshape(NQ_MAX, n) * (0.25 / (NQ_MAX * n))).astype(np.float32)
    assert all(len(np.unique(per_query[q])) == n for q in range(nq))
    boost = rng.uniform(0.5, 2.0, size=NQ_MAX).astype(np.float32)
    for mode in ("raw", "opensearch"):
        w.check(nq, 10, per_query, boost=boost, mode=mode, what="deep")
    # the column ends inside the fourth round of tiles: the late tiles read 0
    w.check(nq, 10, per_query, boost=boost, mode="raw", bonus_rows=(n * 7 // 10) | 1, what="deep, short column")
