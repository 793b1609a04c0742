"""Allow-list search against the CPU oracle: ``rass_index_search_allowed(_device)``, the bitmap builders and the plan.

The expected answer never comes from the engine's own top-k path (one equivalence test excepted, and it says so).  Scores
are the oracle's emulation of the scan's fmaf order (``KIND_F32_MFMA``) for the queries as the GPU normalised them; the rows
that are live, pass the tag filter (through the mask where there is one) and have their bit set are ranked (score desc, id
asc) by numpy and cut at k.  Where no bitmap is involved that ranking is first held to ``oracle.search``.  Ids and scores
must be EQUAL: no tolerance anywhere in this file.

Shapes: dims 128 and 1024 (both ends of the row stride; at 1024 all 8 K-slices carry 8 chunks), n = 20 (less than a tile),
1 000 (the last tile has 8 rows) and 4 128 (129 tiles: more tiles than a small grid's workgroups take one each), nq = 1, 5,
32, 33 (a second launch group with one query) and 70, k = 1, 10, 32 and 100 (four passes under the continuation bound).
Each world (corpus, oracle score matrix, engine, index) is built once for the module.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
ORACLE_MAX_K = 1024
PATIENT_MASK = 0x00FFFFFF
DOCTYPE_MASK = 0x7F000000
NQ_MAX = 70
NQS = (1, 5, 32, 33, 70)
KS = (1, 10, 32, 100)
SHAPES = [(20, 128), (1000, 128), (4128, 128), (20, 1024), (1000, 1024), (4128, 1024)]


class World:
    """Rows, tags (with tombstones), 70 queries, the oracle's score matrix and a live index holding the rows."""

    def __init__(self, torch, oracle, n, dim):
        from rassengine_amd import ops
        from rassengine_amd.engine import Engine
        rng = np.random.default_rng(7000 + n + dim)
        self.torch, self.oracle, self.n, self.dim = torch, oracle, n, dim
        self.xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
        self.q_raw = rng.standard_normal((NQ_MAX, dim), dtype=np.float32) * 3.0     # un-normalised on purpose
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        # patient codes from a few (n = 20) to thousands of distinct values, two doc types
        self.tags = (rng.integers(0, 5 if n < 100 else 5000, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)
        self.dead = sorted({3, n // 2, n - 1, n - 5} if n < 100 else set(rng.choice(n, size=n // 25, replace=False)) | {n - 1, 31, 32})
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.eng = Engine(0, dim)
        self.idx = self.eng.open_index("allow")
        self.idx.add(self.xn, tags=self.tags, normalize=False)
        for r in self.dead:
            self.idx.delete(int(r))
        self.tags = self.tags.copy()
        self.tags[self.dead] = -1
        self.words = (n + 31) // 32

    def matching(self, q, bits, qfilter=None, qmask=None):
        ok = self.tags != -1
        if qfilter is not None and qfilter[q] >= 0:
            ok &= ((self.tags & qmask[q]) if qmask is not None else self.tags) == qfilter[q]
        if bits is not None:
            b = bits[0] if bits.shape[0] == 1 else bits[q]
            ok &= b[:self.n]
        return np.flatnonzero(ok)

    def expect(self, nq, k, bits, qfilter=None, qmask=None):
        """(scores [nq, k], ids [nq, k]): ``bits`` is bool [1 or nq, >= n] or None (no bitmap: held to oracle.search)."""
        es = np.full((nq, k), NEG_INF, dtype=np.float32)
        ei = np.full((nq, k), -1, dtype=np.int64)
        for q in range(nq):
            rows = self.matching(q, bits, qfilter, qmask)
            s = self.scores[q, rows]
            order = np.lexsort((rows, -s))[:k]
            es[q, :len(order)], ei[q, :len(order)] = s[order], rows[order]
        if bits is None:
            ko = max(1, min(k, self.n, ORACLE_MAX_K))
            s_o, i_o = self.oracle.search(self.xn, self.qn_gpu[:nq], ko, kind=self.oracle.KIND_F32_MFMA, tags=self.tags, qfilter=qfilter,
                                          qmask=qmask)
            assert np.array_equal(i_o[:, :ko], ei[:, :ko]) and np.array_equal(s_o[:, :ko].astype(np.float32), es[:, :ko])
        return es, ei

    def run_device(self, nq, k, d_allow, n_bitmaps, words, qfilter=None, qmask=None):
        torch = self.torch
        dq = torch.from_numpy(np.ascontiguousarray(self.q_raw[:nq])).cuda()
        df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter[:nq], dtype=np.int32)).cuda()
        dm = None if qmask is None else torch.from_numpy(np.ascontiguousarray(qmask[:nq], dtype=np.int32)).cuda()
        os_ = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        oi = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                        # the engine works on its own stream
        self.idx.search_allowed_device(dq.data_ptr(), nq, k, d_allow.data_ptr(), n_bitmaps, words, os_.data_ptr(), oi.data_ptr(),
                                       d_q_filter_ptr=0 if df is None else df.data_ptr(),
                                       d_q_filter_mask_ptr=0 if dm is None else dm.data_ptr())
        self.eng.synchronize()
        return os_.cpu().numpy(), oi.cpu().numpy()

    def check(self, nq, k, bits, qfilter=None, qmask=None, what=""):
        """Host and device entry points against the oracle's ranking; returns the host answer."""
        from rassengine_amd.engine import pack_allow
        torch = self.torch
        words = pack_allow(bits if bits.shape[0] == 1 else bits[:nq])
        want = self.expect(nq, k, bits, qfilter, qmask)
        f = None if qfilter is None else qfilter[:nq]
        m = None if qmask is None else qmask[:nq]
        allow = words[0] if bits.shape[0] == 1 and nq != 1 else words           # [words] = shared; nq = 1: [1, words] is both
        got = self.idx.search_allowed(self.q_raw[:nq], k, allow, q_filter=f, q_filter_mask=m)
        assert_same(got, want, (what, "host", self.n, self.dim, nq, k))
        d_allow = torch.from_numpy(words.view(np.int32)).cuda()
        dev = self.run_device(nq, k, d_allow, words.shape[0], words.shape[1], qfilter, qmask)
        assert_same(dev, want, (what, "device", self.n, self.dim, nq, k))
        return got


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids")):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


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


def random_bits(n, density, seed, nb=NQ_MAX):
    return np.random.default_rng(seed).random((nb, n)) < density


@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("density", [0.5, 0.01])
def test_random_bitmap_per_query(worlds, n, dim, density):
    w = worlds(n, dim)
    bits = random_bits(n, density, seed=int(density * 100) + n)
    for nq in NQS:
        for k in KS:
            w.check(nq, k, bits, what=f"density {density}")


@pytest.mark.parametrize("n,dim", SHAPES)
def test_shared_bitmap_equals_the_same_bitmap_per_query(worlds, n, dim):
    w = worlds(n, dim)
    one = random_bits(n, 0.3, seed=11 + n, nb=1)
    for nq in (5, 33, 70):
        for k in (10, 100):
            shared = w.check(nq, k, one, what="shared")
            repeated = w.check(nq, k, np.repeat(one, nq, axis=0), what="repeated")
            assert_same(shared, repeated, ("shared vs repeated", n, dim, nq, k))


@pytest.mark.parametrize("n,dim", SHAPES)
def test_single_row_and_fewer_rows_than_k(worlds, n, dim):
    w = worlds(n, dim)
    live = np.flatnonzero(w.tags != -1)
    bits = np.zeros((NQ_MAX, n), dtype=bool)
    bits[np.arange(NQ_MAX), live[(np.arange(NQ_MAX) * 7) % len(live)]] = True        # one allowed row per query, all different
    for nq, k in ((1, 1), (5, 10), (33, 32), (70, 100)):
        s, i = w.check(nq, k, bits, what="single row")
        assert np.all(i[:, 0] >= 0) and np.all(i[:, 1:] == -1) and np.all(np.isneginf(s[:, 1:]))
    few = np.zeros((1, n), dtype=bool)
    few[0, live[:: max(1, len(live) // 5)][:5]] = True                                # five rows, shared
    for nq, k in ((5, 10), (33, 100)):
        s, i = w.check(nq, k, few, what="five rows")
        assert np.all(i[:, :5] >= 0) and np.all(i[:, 5:] == -1) and np.all(np.isneginf(s[:, 5:]))


@pytest.mark.parametrize("n,dim", SHAPES)
def test_all_zero_bitmap_is_the_empty_answer(worlds, n, dim):
    w = worlds(n, dim)
    for nb in (1, 33):
        s, i = w.check(33, 10, np.zeros((nb, n), dtype=bool), what="all zero")
        assert np.all(i == -1) and np.all(np.isneginf(s))
    s, i = w.check(1, 100, np.zeros((1, n), dtype=bool), what="all zero, passes")
    assert np.all(i == -1)
    zero = w.torch.zeros((32, w.words), dtype=w.torch.int32, device="cuda")
    w.torch.cuda.synchronize()
    tile, rows, mask = w.idx.allow_plan(zero, 32)
    assert len(tile) == 0


@pytest.mark.parametrize("n,dim", SHAPES)
def test_bits_on_tombstones_and_past_the_end_allow_nothing(worlds, n, dim):
    from rassengine_amd.engine import pack_allow
    w = worlds(n, dim)
    only_dead = np.zeros((1, n), dtype=bool)
    only_dead[0, w.dead] = True
    s, i = w.check(5, 10, only_dead, what="tombstones only")
    assert np.all(i == -1)
    # every bit set, in the last word past n_rows and in three surplus words too
    wide = np.ones((1, w.words * 32 + 96), dtype=bool)
    got = w.check(33, 100, wide, what="all ones, surplus words")
    assert not np.isin(got[1], w.dead).any() and got[1].max() < n
    # ONLY bits past n_rows (when the last word has room) and the surplus words
    past = np.zeros((1, w.words * 32 + 96), dtype=bool)
    past[0, n:] = True
    s, i = w.check(5, 10, past, what="only past the end")
    assert np.all(i == -1)
    d_past = w.torch.from_numpy(pack_allow(past).view(np.int32)).cuda()
    w.torch.cuda.synchronize()
    assert len(w.idx.allow_plan(d_past[0].contiguous(), 5)[0]) == 0


@pytest.mark.parametrize("n,dim", SHAPES)
def test_combined_with_tag_filters(worlds, n, dim):
    w = worlds(n, dim)
    rng = np.random.default_rng(5 + n + dim)
    bits = random_bits(n, 0.6, seed=23 + n)
    live = np.flatnonzero(w.tags != -1)
    pick = w.tags[live[rng.integers(0, len(live), size=NQ_MAX)]]
    # plain: the whole tag must equal the filter; every third query unfiltered
    plain = pick.astype(np.int32).copy()
    plain[::3] = -1
    for nq, k in ((5, 10), (33, 32), (70, 100)):
        w.check(nq, k, bits, qfilter=plain, what="plain filter")
    # masked: by patient, by doc type, and unfiltered, mixed over the queries
    qmask = np.where(np.arange(NQ_MAX) % 2 == 0, PATIENT_MASK, DOCTYPE_MASK).astype(np.int32)
    qfilt = (pick & qmask).astype(np.int32)
    qfilt[::5] = -1
    for nq, k in ((1, 1), (32, 10), (33, 100), (70, 32)):
        w.check(nq, k, bits, qfilter=qfilt, qmask=qmask, what="masked filter")


@pytest.mark.parametrize("n,dim", SHAPES)
def test_all_ones_equals_plain_search(worlds, n, dim):
    """The one place the engine's own top-k is the comparison — next to the oracle check of the same case."""
    w = worlds(n, dim)
    ones = np.ones((1, n), dtype=bool)
    for nq, k in ((5, 10), (33, 32), (70, 100)):
        want = w.expect(nq, k, None)                            # no bitmap: held to oracle.search inside
        got = w.check(nq, k, ones, what="all ones")
        assert_same(got, want, ("all ones vs oracle.search", n, dim, nq, k))
        assert_same(got, w.idx.search(w.q_raw[:nq], k), ("all ones vs search", n, dim, nq, k))


def test_prefilter_mode_serves_the_exact_scan(worlds):
    w = worlds(4128, 128)
    bits = random_bits(4128, 0.2, seed=77)
    before = w.check(33, 10, bits, what="mode 0")
    w.idx.set_prefilter("int8")
    try:
        assert w.idx.prefilter_mode == "int8"
        during = w.check(33, 10, bits, what="mode 2")
    finally:
        w.idx.set_prefilter(False)
    assert_same(during, before, "prefilter mode 2 vs 0")


def test_duplicate_rows_tie_by_id(gpu, oracle):
    """40 identical rows spread over 7 tiles: the id-asc rule decides, across workgroups, inside a tile, at the k cut and at
    the continuation bound of a k = 100 search (the 32nd hit is one of the duplicates)."""
    w = World(gpu, oracle, 200, 128)
    try:
        dup = np.arange(2, 200, 5)
        dup = dup[w.tags[dup] != -1]
        xn = w.xn.copy()
        xn[dup] = xn[dup[0]]
        w.eng.drop_index("allow")
        w.idx = w.eng.open_index("allow-dup")
        w.idx.add(xn, tags=np.where(w.tags == -1, 0, w.tags).astype(np.int32), normalize=False)
        for r in w.dead:
            w.idx.delete(int(r))
        w.xn = xn
        w.q_raw[:8] = xn[dup[0]] * 2.5                                   # eight queries whose best rows are the duplicates
        from rassengine_amd import ops
        w.qn_gpu = ops.normalize_rows(gpu.from_numpy(w.q_raw).cuda()).cpu().numpy()
        w.scores = oracle.scores(w.xn, w.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        assert len(np.unique(w.scores[0, dup])) == 1 and w.scores[0, dup[0]] == w.scores[0].max()
        all_on = np.ones((1, 200), dtype=bool)
        some = all_on.copy()
        some[0, dup[1::3]] = False
        for bits, what in ((all_on, "all duplicates allowed"), (some, "some not")):
            allowed_dup = dup[bits[0, dup]]
            for k in (1, 10, 32, 100):
                s, i = w.check(8, k, bits, what=what)
                m = min(k, len(allowed_dup))
                assert np.array_equal(i[0, :m], allowed_dup[:m])
    finally:
        w.eng.close()


def test_rows_appended_after_the_bitmap_was_built(gpu, oracle):
    """An append does not move the layout epoch and may land between building a bitmap and searching with it — here 40 rows
    across a 32-row boundary (200 -> 240), each a copy of a query, so every one would rank first.  The bitmap speaks for the
    rows it was built over: device bitmaps from both builders and a host bitmap of exactly ceil(200 / 32) words all search
    the grown index without an error and never return a new row."""
    from rassengine_amd.engine import pack_allow
    w = World(gpu, oracle, 200, 128)
    try:
        bits = random_bits(200, 0.5, seed=9, nb=1)
        rows = np.flatnonzero(bits[0])
        values = np.unique(w.tags[w.tags != -1] & PATIENT_MASK)[::2].astype(np.int32)
        by_tag = (np.isin(w.tags & PATIENT_MASK, values) & (w.tags != -1))[None, :]
        d_rows = w.idx.allow_from_rows(rows)
        d_tags = w.idx.allow_from_tag_values(values, PATIENT_MASK)
        host = pack_allow(bits[0])
        assert host.shape == (7,)
        want_rows, want_tags = w.expect(33, 10, bits), w.expect(33, 10, by_tag)
        late = oracle.normalize_ref(w.q_raw[:40]).astype(np.float32)
        assert w.idx.add(late, tags=np.full(40, int(values[0]), dtype=np.int32), normalize=False) == 200 and w.idx.rows == 240
        for allow, want, what in ((d_rows, want_rows, "allow_from_rows"), (host, want_rows, "host words"),
                                  (np.repeat(host[None, :], 33, axis=0), want_rows, "host words per query"), (d_tags, want_tags, "allow_from_tag_values")):
            got = w.idx.search_allowed(w.q_raw[:33], 10, allow)
            assert got[1].max() < 200, what
            assert_same(got, want, ("appended after the build", what))
        # a bitmap built now sees them: query j's best row is its own copy
        s, i = w.idx.search_allowed(w.q_raw[:33], 1, w.idx.allow_from_tag_values(values[:1], PATIENT_MASK))
        assert np.array_equal(i[:33, 0], 200 + np.arange(33))
    finally:
        w.eng.close()


@pytest.mark.parametrize("n,dim", [(20, 128), (1000, 1024), (4128, 128)])
def test_allow_from_rows_equals_numpy(worlds, n, dim):
    from rassengine_amd.engine import pack_allow
    w = worlds(n, dim)
    rng = np.random.default_rng(n)
    rows = rng.integers(0, n, size=max(3, n // 3))
    rows = np.concatenate([rows, rows[:5], [-1, -7, n, n + 1, n + 31, 2 ** 40, -2 ** 40, 0, n - 1]]).astype(np.int64)
    want = np.zeros(n, dtype=bool)
    want[rows[(rows >= 0) & (rows < n)]] = True
    d = w.idx.allow_from_rows(rows)
    w.eng.synchronize()
    got = d.cpu().numpy().view(np.uint32)
    assert len(got) >= w.words and np.array_equal(got[:w.words], pack_allow(want)) and not got[w.words:].any()     # slack words: zero
    assert not w.idx.allow_from_rows(np.zeros(0, dtype=np.int64)).cpu().numpy().any()
    # ... and the search over it
    s, i = w.idx.search_allowed(w.q_raw[:5], 10, d)
    assert_same((s, i), w.expect(5, 10, want[None, :]), "search over allow_from_rows")


@pytest.mark.parametrize("n,dim", [(20, 128), (1000, 128), (4128, 1024)])
@pytest.mark.parametrize("n_values", [1, 7, 3000])
def test_allow_from_tag_values_equals_numpy(worlds, n, dim, n_values):
    """3 000 values exceed the builder's LDS tier (2 048): the set is searched in global memory."""
    from rassengine_amd.engine import pack_allow
    w = worlds(n, dim)
    rng = np.random.default_rng(n_values + n)
    present = np.unique(w.tags[w.tags != -1] & PATIENT_MASK)
    values = np.concatenate([rng.choice(present, size=min(len(present), (n_values + 1) // 2), replace=False),
                             rng.integers(0, 1 << 24, size=n_values)])[:n_values].astype(np.int32)
    rng.shuffle(values)                                                     # any order, duplicates possible
    for mask, vals in ((PATIENT_MASK, values), (PATIENT_MASK | DOCTYPE_MASK, values | (1 << 24)), (DOCTYPE_MASK, np.array([2 << 24], np.int32))):
        want = np.isin(w.tags & mask, vals) & (w.tags != -1)
        d = w.idx.allow_from_tag_values(vals, mask)
        w.eng.synchronize()
        got = d.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:w.words], pack_allow(want)) and not got[w.words:].any(), (n, n_values, hex(mask))
    s, i = w.idx.search_allowed(w.q_raw[:33], 10, d)
    assert_same((s, i), w.expect(33, 10, want[None, :]), "search over allow_from_tag_values")


@pytest.mark.parametrize("n,dim", [(1000, 128), (4128, 1024)])
def test_plan_equals_numpy(worlds, n, dim):
    from rassengine_amd.engine import pack_allow
    w = worlds(n, dim)
    single = np.zeros((32, n), dtype=bool)
    single[17, n - 3] = True
    for bits, what in ((random_bits(n, 0.01, seed=3 + n, nb=32), "density 0.01"), (single, "a single bit")):
        words = pack_allow(bits)
        d = w.torch.from_numpy(words.view(np.int32)).cuda()
        w.torch.cuda.synchronize()
        tile, rows, mask = w.idx.allow_plan(d, 32)
        want = set()
        for t in range(w.words):
            m = sum(1 << q for q in range(32) if words[q, t] != 0)
            if m:
                want.add((t, min(32, n - 32 * t), m))
        assert len(tile) == len(want) == int(np.count_nonzero((words != 0).any(axis=0))), what
        assert set(zip(tile.tolist(), rows.tolist(), mask.tolist())) == want, what
    # a shared bitmap: the mask names every query of the group
    one = pack_allow(single[17])
    d = w.torch.from_numpy(one.view(np.int32)).cuda()
    w.torch.cuda.synchronize()
    tile, rows, mask = w.idx.allow_plan(d, 5)
    assert (tile.tolist(), rows.tolist(), mask.tolist()) == ([(n - 3) // 32], [min(32, n - 32 * ((n - 3) // 32))], [0b11111])


def test_error_paths(worlds, gpu):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    L = N.lib()
    w = worlds(1000, 128)
    q = np.ascontiguousarray(w.q_raw[:3])
    out_s, out_i = np.empty((3, 4096), np.float32), np.empty((3, 4096), np.int64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(idx, queries, k, allow, n_bitmaps, words):
        rc = L.rass_index_search_allowed(idx._h, ptr(queries), 3, k, ptr(allow), n_bitmaps, words, None, None, ptr(out_s), ptr(out_i))
        return rc, L.rass_last_error().decode()

    ones = np.full((3, w.words + 2), 0xFFFFFFFF, dtype=np.uint32)
    assert call(w.idx, q, 10, ones, 3, w.words + 2)[0] == 0
    for what, args in (("words too small", (w.idx, q, 10, ones, 3, w.words - 1)),
                       ("n_bitmaps neither 1 nor nq", (w.idx, q, 10, ones, 2, w.words)),
                       ("k = 0", (w.idx, q, 0, ones, 3, w.words)),
                       ("k too large", (w.idx, q, N.RASS_MAX_K_MULTIPASS + 1, ones, 3, w.words))):
        rc, text = call(*args)
        assert rc != 0 and text, what
    # the device entry point refuses the same way
    d = gpu.from_numpy(ones.view(np.int32)).cuda()
    with pytest.raises(N.RassError):
        w.idx.search_allowed_device(d.data_ptr(), 3, 10, d.data_ptr(), 3, w.words - 1, d.data_ptr(), d.data_ptr())
    with pytest.raises(ValueError):
        w.idx.search_allowed(q, 10, ones[:2])                       # a [2, words] bitmap for 3 queries: caught in Python
    for dim, dtype, what in ((256, "bf16", "bf16 index"), (1536, "f32", "dim 1536")):
        eng = Engine(0, dim)
        try:
            idx = eng.open_index("allow-err", dtype=dtype)
            x = np.random.default_rng(1).standard_normal((40, dim), dtype=np.float32)
            idx.add(x)
            rc, text = call(idx, np.ascontiguousarray(x[:3]), 10, ones, 3, 2)
            assert rc != 0 and text, what
        finally:
            eng.close()
