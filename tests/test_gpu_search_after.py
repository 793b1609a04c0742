"""The continuation-bound search ``rass_index_search_device_after`` against the CPU oracle.

The entry point returns, per query, the best k rows that rank strictly behind a caller-supplied (after_score[q],
after_row[q]) under (score desc, row ordinal asc); ``serving.HipServingShard.search_packed(after=...)`` calls it for every
pass of a sharded k > 32 search.  The host ``search(k > 32)`` loop reaches the same kernels, but only with the previous
pass's own last hit as the bound, 32 rows per pass and a tolerance; here the bound is whatever a front or a C caller can
hand over: a value between two scores, +-inf, NaN, a row of -1 or past the row count, a row the query cannot see.

The expected answer never comes from the engine's own top-k path.  As in test_gpu_range_search.py the scores are the oracle's
emulation of the scan's fmaf order (``KIND_F32_MFMA``) for the queries as the GPU normalised them; per query the rows that are
live and pass the filter are ranked with ``np.lexsort((rows, -s))``; the first min(n, 1 024) of that ranking must be
``oracle.search``'s answer before anything is compared with the GPU; and the ranking is cut at the bound in numpy: a row stays
iff ``s < a_s or (s == a_s and row > a_r)``.  The first k of what stays, padded with (-inf, -1), is what the entry point must
return.  Ids and scores must be EQUAL for fp32 indices.  The only tolerance in this file is the bf16 index's (the last section
but two), taken from test_gpu_bf16_corpus.py, where every bound sits in a gap of the fp64 ranking four tolerances wide so
that the side a row falls on does not depend on the kernel's rounding.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
POS_INF = np.float32(np.inf)
I64_MAX = np.iinfo(np.int64).max
ORACLE_MAX_K = 1024
ERR_INVALID = -1                 # RASS_ERR_INVALID
PMASK, DMASK = 0x00FFFFFF, 0x7F000000


class Corpus:
    """Rows, tags and queries of one case with the oracle's score matrix, computed once."""

    def __init__(self, torch, oracle, n, dim, nq, seed, tags=None):
        from rassengine_amd import ops
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.nq = n, dim, nq
        self.xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0     # un-normalised on purpose
        self.tags = tags
        self._torch, self._ops, self._oracle = torch, ops, oracle
        self.refresh()

    def refresh(self):
        """(Re)compute the GPU-normalised queries and the score matrix: after a test edited rows or queries (ties)."""
        self.qn_gpu = self._ops.normalize_rows(self._torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = self._oracle.scores(self.xn, self.qn_gpu, kind=self._oracle.KIND_F32_MFMA).astype(np.float32)

    def ranked(self, tags=None, qfilter=None, qmask=None, check=True):
        """Per query the (scores f32, row ordinals i64) of every row it can see, score desc, row asc."""
        tags = self.tags if tags is None else tags
        out = []
        for q in range(self.nq):
            ok = np.ones(self.n, dtype=bool)
            if tags is not None:
                ok &= tags != -1
                if qfilter is not None and qfilter[q] >= 0:
                    ok &= ((tags & qmask[q]) if qmask is not None else tags) == qfilter[q]
            rows = np.flatnonzero(ok).astype(np.int64)
            s = self.scores[q, rows]
            order = np.lexsort((rows, -s))
            out.append((s[order], rows[order]))
        if check:        # the ranking above IS oracle.search's as far as that reaches
            k = max(1, min(self.n, ORACLE_MAX_K))
            s_o, i_o = self._oracle.search(self.xn, self.qn_gpu, k, kind=self._oracle.KIND_F32_MFMA, tags=tags,
                                           qfilter=qfilter if tags is not None else None, qmask=qmask if tags is not None else None)
            for q, (s, i) in enumerate(out):
                m = min(k, len(i))
                assert np.array_equal(i_o[q, :m], i[:m]) and np.array_equal(s_o[q, :m].astype(np.float32), s[:m])
                assert np.all(i_o[q, m:] == -1)
        return out


def bounds_at(ranked, rank_of):
    """(after_score f32 [nq], after_row i64 [nq]): query q's bound is the row at rank ``rank_of(q, len)`` of its own ranking
    (clipped to the last one); a query that sees no row gets (-inf, INT64_MAX)."""
    a_s = np.full(len(ranked), NEG_INF, dtype=np.float32)
    a_r = np.full(len(ranked), I64_MAX, dtype=np.int64)
    for q, (s, rows) in enumerate(ranked):
        if len(s):
            j = min(int(rank_of(q, len(s))), len(s) - 1)
            a_s[q], a_r[q] = s[j], rows[j]
    return a_s, a_r


def expect(ranked, a_s, a_r, k, ids=None):
    """(scores [nq, k], ids [nq, k]) the entry point must return: the ranking cut at the bound, its first k, padded.
    ``ids``: the id reported for each row ordinal (caller-assigned ids); the cut itself is in ordinals."""
    nq = len(ranked)
    es = np.full((nq, k), NEG_INF, dtype=np.float32)
    ei = np.full((nq, k), -1, dtype=np.int64)
    for q, (s, rows) in enumerate(ranked):
        with np.errstate(invalid="ignore"):
            keep = (s < a_s[q]) | ((s == a_s[q]) & (rows > a_r[q]))
        s, rows = s[keep][:k], rows[keep][:k]
        es[q, :len(s)] = s
        ei[q, :len(s)] = rows if ids is None else np.asarray(ids, dtype=np.int64)[rows]
    return es, ei


class Device:
    """One launch group's queries and filters in device memory, uploaded once; ``after`` runs one bounded pass."""

    def __init__(self, torch, idx, q_raw, qfilter=None, qmask=None):
        self.torch, self.idx, self.nq = torch, idx, q_raw.shape[0]
        self.dq = torch.from_numpy(np.ascontiguousarray(q_raw, dtype=np.float32)).cuda()
        self.df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter, dtype=np.int32)).cuda()
        self.dm = None if qmask is None else torch.from_numpy(np.ascontiguousarray(qmask, dtype=np.int32)).cuda()

    def after(self, a_s, a_r, k):
        torch, nq = self.torch, self.nq
        ds = torch.from_numpy(np.ascontiguousarray(a_s, dtype=np.float32)).cuda()
        dr = torch.from_numpy(np.ascontiguousarray(a_r, dtype=np.int64)).cuda()
        assert ds.shape == (nq,) and dr.shape == (nq,)
        os_ = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        oi = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                        # the engine works on its own stream
        self.idx.search_device_after(self.dq.data_ptr(), nq, k, ds.data_ptr(), dr.data_ptr(), os_.data_ptr(), oi.data_ptr(),
                                     d_q_filter_ptr=0 if self.df is None else self.df.data_ptr(),
                                     d_q_filter_mask_ptr=0 if self.dm is None else self.dm.data_ptr())
        self.idx.engine.synchronize()
        return os_.cpu().numpy(), oi.cpu().numpy()


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids")):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def tagged(n, seed):
    """patient | doc_type tags as the range test's ``small`` fixture has them."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 6, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)


def mixed_filters(nq):
    """(plain filter, masked filter, mask) per query: exact tags, -1 (no filter), a value no row carries; patient-only,
    doc-type-only and whole-tag masks."""
    plain = np.array([[-1, 0 | (1 << 24), 1 | (2 << 24), 5 | (1 << 24), 99, 3 | (2 << 24)][q % 6] for q in range(nq)], dtype=np.int32)
    filt = np.array([[3, 2 << 24, -1, 0, 77, 1 << 24, 1 | (1 << 24)][q % 7] for q in range(nq)], dtype=np.int32)
    mask = np.array([[PMASK, DMASK, -1, PMASK, PMASK, DMASK, -1][q % 7] for q in range(nq)], dtype=np.int32)
    return plain, filt, mask


# ---- 1. paging equals the ranking

@pytest.mark.parametrize("nq", [1, 16, 17, 32])
@pytest.mark.parametrize("dim", [100, 256, 1024])
def test_after_paging_equals_the_ranking(gpu, oracle, dim, nq):
    """3 000 rows (94 tiles of 32: up to the CU count one tile per workgroup, beyond it several) paged with k = 1, 7 (the first
    40 pages) and 32 (all 94 pages, the last one short, and one page past the end).  Page p's bound is the oracle's row at rank
    p k - 1, never the GPU's output, and every page must equal the oracle's slice."""
    from rassengine_amd.engine import Engine
    n = 3000
    case = Corpus(gpu, oracle, n, dim, nq, seed=7000 + dim + nq)
    ranked = case.ranked()
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("after-paging")
        idx.add(case.xn, normalize=False)
        dev = Device(gpu, idx, case.q_raw)
        for k, pages in ((1, 40), (7, 40), (32, (n + 31) // 32 + 1)):
            whole = []
            for p in range(pages):
                if p == 0:
                    a_s, a_r = np.full(nq, POS_INF), np.full(nq, -1, dtype=np.int64)
                else:
                    a_s, a_r = bounds_at(ranked, lambda q, m: p * k - 1)
                got = dev.after(a_s, a_r, k)
                want_s = np.full((nq, k), NEG_INF, dtype=np.float32)
                want_i = np.full((nq, k), -1, dtype=np.int64)
                for q, (s, rows) in enumerate(ranked):      # the oracle's slice, by position
                    m = len(s[p * k:(p + 1) * k])
                    want_s[q, :m], want_i[q, :m] = s[p * k:(p + 1) * k], rows[p * k:(p + 1) * k]
                assert_same(expect(ranked, a_s, a_r, k), (want_s, want_i), f"the numpy cut, k {k} page {p}")
                assert_same(got, (want_s, want_i), f"k {k} page {p}")
                whole.append(got)
            if k == 32:     # every page was run: the concatenation is the whole ranking, then padding
                assert n % 32 != 0 and np.all(whole[-2][1][:, n % 32:] == -1) and np.all(whole[-1][1] == -1)
                cs, ci = np.concatenate([w[0] for w in whole], axis=1), np.concatenate([w[1] for w in whole], axis=1)
                for q, (s, rows) in enumerate(ranked):
                    assert np.array_equal(ci[q, :n], rows) and np.array_equal(cs[q, :n], s)
                    assert np.all(ci[q, n:] == -1) and np.all(np.isneginf(cs[q, n:]))
    finally:
        eng.close()


# ---- 2. bounds that are no row's score

def test_after_bounds_that_are_no_rows_score(gpu, oracle):
    """A midpoint between two neighbouring scores (``after_row`` 0, -1 and INT64_MAX must not matter), +inf (the plain
    top-k, whatever the row), -inf and NaN (nothing: every comparison of the kernels with NaN is false)."""
    from rassengine_amd.engine import Engine
    n, nq = 3000, 32
    case = Corpus(gpu, oracle, n, 256, nq, seed=7100)
    ranked = case.ranked()
    mid = np.empty(nq, dtype=np.float32)
    rank = np.empty(nq, dtype=np.int64)
    for q, (s, _) in enumerate(ranked):
        j = 37 * q + 5                                   # a different rank per query; the next gap a float32 fits into
        while not s[j] > np.float32((np.float64(s[j]) + np.float64(s[j + 1])) / 2) > s[j + 1]:
            j += 1
        mid[q], rank[q] = np.float32((np.float64(s[j]) + np.float64(s[j + 1])) / 2), j
        assert j < 37 * q + 5 + 20 and not np.any(s == mid[q])
    eng = Engine(0, 256)
    try:
        idx = eng.open_index("after-odd-bounds")
        idx.add(case.xn, normalize=False)
        dev = Device(gpu, idx, case.q_raw)
        for k in (7, 32):
            want = expect(ranked, mid, np.zeros(nq, dtype=np.int64), k)
            for q, (s, rows) in enumerate(ranked):       # by construction: what follows rank j
                assert np.array_equal(want[1][q], rows[rank[q] + 1:rank[q] + 1 + k])
            for row in (0, -1, I64_MAX):
                assert_same(dev.after(mid, np.full(nq, row, dtype=np.int64), k), want, f"midpoint, row {row}, k {k}")
            top = (np.stack([s[:k] for s, _ in ranked]), np.stack([r[:k] for _, r in ranked]))
            s_o, i_o = oracle.search(case.xn, case.qn_gpu, k, kind=oracle.KIND_F32_MFMA)
            assert_same((s_o.astype(np.float32), i_o), top, "the oracle's plain top-k")
            for row in (-1, I64_MAX):
                assert_same(dev.after(np.full(nq, POS_INF), np.full(nq, row, dtype=np.int64), k), top, f"+inf, row {row}, k {k}")
            nothing = (np.full((nq, k), NEG_INF, dtype=np.float32), np.full((nq, k), -1, dtype=np.int64))
            for bound in (NEG_INF, np.float32(np.nan)):
                for row in (-1, 0, I64_MAX):
                    assert_same(dev.after(np.full(nq, bound), np.full(nq, row, dtype=np.int64), k), nothing, f"{bound}, row {row}, k {k}")
            # one call with every kind side by side: the bound is per query
            a_s, a_r = mid.copy(), np.full(nq, -1, dtype=np.int64)
            a_s[1::4], a_s[2::4], a_s[3::4] = POS_INF, NEG_INF, np.nan
            a_r[3::4] = I64_MAX
            want = expect(ranked, a_s, a_r, k)
            assert np.all(want[1][2::4] == -1) and np.all(want[1][3::4] == -1) and np.array_equal(want[1][1::4], top[1][1::4])
            assert_same(dev.after(a_s, a_r, k), want, f"mixed bounds, k {k}")
    finally:
        eng.close()


# ---- 3. ties

def test_after_ties_by_row(gpu, oracle):
    """64 copies of one vector: at the tie score ``after_row`` alone decides which copies are left."""
    from rassengine_amd.engine import Engine
    n = 500
    case = Corpus(gpu, oracle, n, 256, 2, seed=63)
    copies = np.sort(np.random.default_rng(3).choice(n, 64, replace=False)).astype(np.int64)
    case.xn[copies] = case.xn[copies[0]]
    case.q_raw[0] = case.xn[copies[0]] * 2.0
    case.refresh()
    ranked = case.ranked()
    tie = ranked[0][0][0]
    assert np.array_equal(ranked[0][1][:64], copies) and np.all(ranked[0][0][:64] == tie) and ranked[0][0][64] < tie
    between = next(int(r) for a, b in zip(copies, copies[1:]) for r in range(a + 1, b))      # no copy, between two copies
    assert between not in copies and copies[0] < between < copies[-1]
    other_s, other_r = bounds_at(ranked, lambda q, m: 9)                                      # query 1: an ordinary bound
    eng = Engine(0, 256)
    try:
        idx = eng.open_index("after-ties")
        idx.add(case.xn, normalize=False)
        dev = Device(gpu, idx, case.q_raw)
        for k in (7, 32):
            for row, left in ((-1, 64), (int(copies[9]), 54), (between, int(np.count_nonzero(copies > between))),
                              (n - 1, 0), (n + 1000, 0)):
                a_s = np.array([tie, other_s[1]], dtype=np.float32)
                a_r = np.array([row, other_r[1]], dtype=np.int64)
                want = expect(ranked, a_s, a_r, k)
                m = min(left, k)
                assert np.array_equal(want[1][0, :m], copies[64 - left:][:m]) and np.all(want[0][0, :m] == tie)
                assert np.all(want[0][0, m:] < tie) and np.all(want[1][0, m:] >= 0)
                assert np.array_equal(want[1][1], ranked[1][1][10:10 + k])
                assert_same(dev.after(a_s, a_r, k), want, f"tie, after_row {row}, k {k}")
    finally:
        eng.close()


# ---- 4. a bound naming a row the query cannot see

def test_after_bound_on_an_invisible_row(gpu, oracle):
    """A front hands a shard a bound translated from another shard's hit: the (score, row) of a tombstoned row, of a row the
    query's plain filter excludes, of a row its masked filter excludes.  Expected: the cut over the rows the query sees."""
    from rassengine_amd.engine import Engine
    n, nq, k = 2000, 14, 10
    tags = tagged(n, 99)
    case = Corpus(gpu, oracle, n, 128, nq, seed=7300, tags=tags)
    dead = np.unique(np.random.default_rng(5).choice(n, 150, replace=False))
    live_tags = tags.copy()
    live_tags[dead] = -1
    plain, filt, mask = mixed_filters(nq)

    def bound_on(hidden_of):
        """Query q's bound: among the rows ``hidden_of(q)`` the one with the (2 q + 1)-th best score for it."""
        a_s, a_r = np.empty(nq, dtype=np.float32), np.empty(nq, dtype=np.int64)
        for q in range(nq):
            rows = np.flatnonzero(hidden_of(q))
            assert len(rows) > 2 * q + 1
            r = rows[np.lexsort((rows, -case.scores[q, rows]))[2 * q + 1]]
            a_s[q], a_r[q] = case.scores[q, r], r
        return a_s, a_r

    eng = Engine(0, 128)
    try:
        idx = eng.open_index("after-invisible")
        idx.add(case.xn, tags=tags, normalize=False)
        for r in dead:
            idx.delete(int(r))
        is_dead = live_tags == -1
        for what, f, m in (("no filter", None, None), ("plain filter", plain, None), ("masked filter", filt, mask)):
            ranked = case.ranked(tags=live_tags, qfilter=f, qmask=m)
            if f is not None:
                assert any(len(r) == 0 for _, r in ranked) and any(len(r) == n - len(dead) for _, r in ranked)
            dev = Device(gpu, idx, case.q_raw, f, m)
            hidden = [("a tombstoned row", lambda q: is_dead)]
            if f is not None:
                # live rows the filter excludes; an unfiltered query (-1) hides nothing but the tombstones
                def excluded(q, f=f, m=m):
                    if f[q] < 0:
                        return is_dead
                    return ~is_dead & (((tags & m[q]) if m is not None else tags) != f[q])
                hidden.append(("a filtered-out row", excluded))
            for name, hidden_of in hidden:
                a_s, a_r = bound_on(hidden_of)
                for q in range(nq):
                    assert a_r[q] not in ranked[q][1]
                want = expect(ranked, a_s, a_r, k)
                assert np.count_nonzero(want[1] >= 0) > 0
                assert_same(dev.after(a_s, a_r, k), want, f"{what}, bound on {name}")
    finally:
        eng.close()


# ---- 5. a deep bound, with and without the sample floor

def test_after_deep_bound_under_the_sample_floor(gpu, oracle, monkeypatch):
    """40 000 rows x 128 columns, 32 queries: 1 250 tiles, so the grid is one workgroup per CU (256 on MI355X), and with more
    than 16 queries ``RASS_SCAN_SAMPLE_FLOOR=force`` samples whenever n_rows >= 2 * 64 * grid = 32 768: the sample pass runs
    UNDER the bound and the big scan drops rows below the floor it yields.  (Unset, the rule is 32 * 64 * grid rows: no sample;
    ``0``: never.)  The bound at rank n - 1 - (q % 12) leaves 0..11 rows, fewer than k = 10 for most queries and none for
    some, and the floor may drop none of them; the second run's bounds are at rank 37 q + 5.  All three settings must equal
    the oracle."""
    from rassengine_amd.engine import Engine
    n, nq, k = 40000, 32, 10
    case = Corpus(gpu, oracle, n, 128, nq, seed=7500)
    ranked = case.ranked()
    deep = bounds_at(ranked, lambda q, m: m - 1 - (q % 12))
    want_deep = expect(ranked, *deep, k)
    for q in range(nq):
        assert np.count_nonzero(want_deep[1][q] >= 0) == min(q % 12, k)
        assert np.array_equal(want_deep[1][q, :q % 12][:k], ranked[q][1][n - (q % 12):][:k])
    shallow = bounds_at(ranked, lambda q, m: 37 * q + 5)
    want_shallow = expect(ranked, *shallow, k)
    for q in range(nq):
        assert np.array_equal(want_shallow[1][q], ranked[q][1][37 * q + 6:37 * q + 6 + k])
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("after-deep")
        idx.add(case.xn, normalize=False)
        dev = Device(gpu, idx, case.q_raw)
        for setting in ("0", "force", None):           # read per call
            if setting is None:
                monkeypatch.delenv("RASS_SCAN_SAMPLE_FLOOR", raising=False)
            else:
                monkeypatch.setenv("RASS_SCAN_SAMPLE_FLOOR", setting)
            assert_same(dev.after(*deep, k), want_deep, f"deep bound, floor {setting}")
            assert_same(dev.after(*shallow, k), want_shallow, f"bound at rank 37 q + 5, floor {setting}")
    finally:
        eng.close()


# ---- 6. wide rows

@pytest.mark.parametrize("nq", [17, 32])
@pytest.mark.parametrize("dim", [1536, 2048])
def test_after_wide_rows_split(gpu, oracle, dim, nq):
    """A row stride above 1 024 takes the wide-row kernel, which answers 16 queries per launch: more than 16 queries run as
    16 + (nq - 16) in two launches, and the launch layer moves the queries, filters, masks, outputs AND the two bound arrays
    on by 16 for the second.  The bounds differ per query (rank 5 q + 3 of the query's own ranking), every second query has a
    masked filter, so queries 16.. answer visibly wrong if they get the bounds, filters or masks of queries 0..15."""
    from rassengine_amd.engine import Engine
    n, k = 1500, 10
    tags = tagged(n, 17)
    case = Corpus(gpu, oracle, n, dim, nq, seed=7600 + dim + nq, tags=tags)
    filt = np.array([[3, 2 << 24, 0, 1 << 24, 5][(q // 2) % 5] if q % 2 == 0 else -1 for q in range(nq)], dtype=np.int32)
    mask = np.array([[PMASK, DMASK, PMASK, DMASK, PMASK][(q // 2) % 5] if q % 2 == 0 else -1 for q in range(nq)], dtype=np.int32)
    ranked = case.ranked(qfilter=filt, qmask=mask)
    a_s, a_r = bounds_at(ranked, lambda q, m: 5 * q + 3)
    want = expect(ranked, a_s, a_r, k)
    for q in range(nq):
        assert len(ranked[q][1]) > 5 * q + 3 + k and np.array_equal(want[1][q], ranked[q][1][5 * q + 4:5 * q + 4 + k])
    for q in range(16, nq):     # the off-by-16 answer is a different one
        assert not np.array_equal(expect(ranked[q:q + 1], a_s[q - 16:], a_r[q - 16:], k)[1], want[1][q:q + 1])
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("after-wide")
        idx.add(case.xn, tags=tags, normalize=False)
        assert_same(Device(gpu, idx, case.q_raw, filt, mask).after(a_s, a_r, k), want, "wide rows, masked filters")
        plain_ranked = case.ranked(check=False)
        p_s, p_r = bounds_at(plain_ranked, lambda q, m: 5 * q + 3)
        assert_same(Device(gpu, idx, case.q_raw).after(p_s, p_r, k), expect(plain_ranked, p_s, p_r, k), "wide rows, no filter")
    finally:
        eng.close()


# ---- 7. index states

@pytest.fixture(scope="module")
def states(gpu, oracle):
    """3 000 rows x 256 columns with patient | doc_type tags, 32 queries, one engine: the index-state tests share it."""
    from rassengine_amd.engine import Engine
    n = 3000
    tags = tagged(n, 99)
    case = Corpus(gpu, oracle, n, 256, 32, seed=7700, tags=tags)
    eng = Engine(0, 256)
    idx = eng.open_index("after-states")
    idx.add(case.xn, tags=tags, normalize=False)
    yield eng, idx, case
    eng.close()


def test_after_ignores_the_prefilter_mode(gpu, states):
    """A bounded request goes to the exact scan whatever the prefilter mode: int8, bf16 and the certified int8 mode answer as
    the oracle says and with the bits of the mode off — at k = 10, where an unbounded request would take the candidate scan,
    and at k = 32, which only the certified mode serves."""
    eng, idx, case = states
    nq = case.nq
    _, filt, mask = mixed_filters(nq)
    runs = []
    for f, m in ((None, None), (filt, mask)):
        ranked = case.ranked(qfilter=f, qmask=m)
        a_s, a_r = bounds_at(ranked, lambda q, n: (37 * q + 5) % max(n - 40, 1))
        runs.append((Device(gpu, idx, case.q_raw, f, m), ranked, a_s, a_r))
    assert idx.prefilter_mode == "off"
    off = {}
    for r, (dev, ranked, a_s, a_r) in enumerate(runs):
        for k in (10, 32):
            off[r, k] = dev.after(a_s, a_r, k)
            assert_same(off[r, k], expect(ranked, a_s, a_r, k), f"mode off, run {r}, k {k}")
    try:
        for mode in ("int8", "bf16", "int8_exact"):
            idx.set_prefilter(mode)
            assert idx.prefilter_mode == mode
            for r, (dev, ranked, a_s, a_r) in enumerate(runs):
                for k in (10, 32):
                    got = dev.after(a_s, a_r, k)
                    assert_same(got, expect(ranked, a_s, a_r, k), f"mode {mode} vs the oracle, run {r}, k {k}")
                    assert np.array_equal(got[0].view(np.uint32), off[r, k][0].view(np.uint32)) and np.array_equal(got[1], off[r, k][1])
    finally:
        idx.set_prefilter(False)


def test_after_tombstones_and_compaction(gpu, states):
    """Tombstoned rows never rank, as bound or not; after ``compact()`` the bound and the expected rows are the old ones
    mapped through ``new_row``."""
    eng, _, case = states
    n, nq, k = case.n, case.nq, 10
    idx = eng.open_index("after-compact")
    idx.add(case.xn, tags=case.tags, normalize=False)
    best = case.ranked(check=False)
    dead = np.unique(np.concatenate([np.random.default_rng(5).choice(n, 200, replace=False),
                                     best[0][1][:3], best[1][1][4:6]]))          # some of the best rows die too
    for r in dead:
        idx.delete(int(r))
    tags = case.tags.copy()
    tags[dead] = -1
    _, filt, mask = mixed_filters(nq)
    for f, m in ((None, None), (filt, mask)):
        ranked = case.ranked(tags=tags, qfilter=f, qmask=m)
        a_s, a_r = bounds_at(ranked, lambda q, n_: (37 * q + 5) % max(n_ - 40, 1))
        assert_same(Device(gpu, idx, case.q_raw, f, m).after(a_s, a_r, k), expect(ranked, a_s, a_r, k), "tombstones")
    new_row = idx.compact()
    assert idx.rows == n - len(dead)
    for f, m in ((None, None), (filt, mask)):
        ranked = case.ranked(tags=tags, qfilter=f, qmask=m, check=False)
        a_s, a_r = bounds_at(ranked, lambda q, n_: (37 * q + 5) % max(n_ - 40, 1))
        moved = [(s, new_row[rows]) for s, rows in ranked]      # the live rows keep their order: new ordinals ascend with the old
        assert all(np.all(rows >= 0) for _, rows in moved)
        new_r = np.where(a_r == I64_MAX, I64_MAX, new_row[np.clip(a_r, 0, n - 1)])
        assert np.all(new_r >= 0)
        assert_same(Device(gpu, idx, case.q_raw, f, m).after(a_s, new_r, k), expect(moved, a_s, new_r, k), "compacted")


def test_after_reports_caller_assigned_ids(gpu, states):
    """An ``add_ex`` index (a shard of a multi-GPU index): the bound is in row ORDINALS, the reported ids are the caller's."""
    eng, _, case = states
    n, nq = case.n, case.nq
    idx = eng.open_index("after-gid")
    idx.add(case.xn[:1200], normalize=False, first_global_id=1000)
    idx.add(case.xn[1200:], normalize=False, first_global_id=50_000)
    gids = np.concatenate([1000 + np.arange(1200), 50_000 + np.arange(n - 1200)]).astype(np.int64)
    ranked = case.ranked(tags=np.zeros(n, dtype=np.int32), check=False)
    dev = Device(gpu, idx, case.q_raw)
    for k in (10, 32):
        a_s, a_r = bounds_at(ranked, lambda q, m: 37 * q + 5)
        want = expect(ranked, a_s, a_r, k, ids=gids)
        assert np.all(want[1] >= 1000) and np.any(want[1] >= 50_000)
        assert_same(dev.after(a_s, a_r, k), want, f"global ids, k {k}")


def test_after_tie_order_is_by_ordinal(gpu, oracle):
    """Caller-assigned ids that do NOT ascend with the insertion order: ties are broken by row ordinal, as the header says,
    and the bound's row is an ordinal too."""
    from rassengine_amd.engine import Engine
    n, half = 600, 300
    case = Corpus(gpu, oracle, n, 256, 2, seed=7800)
    copies = np.array([5, 140, 299, 300, 421, 598], dtype=np.int64)      # on both sides of the batch boundary
    case.xn[copies] = case.xn[copies[0]]
    case.q_raw[0] = case.xn[copies[0]] * 2.0
    case.refresh()
    ranked = case.ranked()
    tie = ranked[0][0][0]
    assert np.array_equal(ranked[0][1][:6], copies) and np.all(ranked[0][0][:6] == tie) and ranked[0][0][6] < tie
    gids = np.concatenate([50_000 + np.arange(half), 1000 + np.arange(n - half)]).astype(np.int64)
    eng = Engine(0, 256)
    try:
        idx = eng.open_index("after-gid-order")
        idx.add(case.xn[:half], normalize=False, first_global_id=50_000)
        idx.add(case.xn[half:], normalize=False, first_global_id=1000)
        dev = Device(gpu, idx, case.q_raw)
        other_s, other_r = bounds_at(ranked, lambda q, m: 9)
        for row, left in ((-1, 6), (140, 4), (299, 3), (300, 2), (n, 0)):
            a_s, a_r = np.array([tie, other_s[1]], dtype=np.float32), np.array([row, other_r[1]], dtype=np.int64)
            want = expect(ranked, a_s, a_r, 7, ids=gids)
            assert np.array_equal(want[1][0, :left], gids[copies[6 - left:]])
            if left == 6:
                assert want[1][0, 2] > want[1][0, 3]                     # ordinal order is not id order here
            assert_same(dev.after(a_s, a_r, 7), want, f"ordinal tie order, after_row {row}")
    finally:
        eng.close()


# ---- 8. the bf16 index

TOL = 2e-6      # test_gpu_bf16_corpus.py: the bf16 scan's scores against the fp64 oracle on the bf16-rounded operands


def _bf16_round(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _swaps_are_ties(i_gpu, i_ref, all64):
    for q in range(i_ref.shape[0]):
        for a, b in zip(i_gpu[q], i_ref[q]):
            if a != b and (a < 0 or b < 0 or abs(all64[q, a] - all64[q, b]) > 2 * TOL):
                return False
    return True


@pytest.fixture(scope="module")
def bf16_case(gpu, oracle):
    from rassengine_amd import ops
    from rassengine_amd.engine import Engine
    n, dim, nq = 3000, 256, 32
    rng = np.random.default_rng(7900)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    tags = tagged(n, 79)
    q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0
    eng = Engine(0, dim)
    idx = eng.open_index("after-bf16", dtype="bf16")
    idx.add(x, tags=tags)
    stored = idx.get_rows(0, n)                              # the bf16-rounded unit rows the scan reads
    qb = _bf16_round(ops.normalize_rows(gpu.from_numpy(q_raw).cuda()).cpu().numpy())
    all64 = oracle.scores(stored, qb)                        # KIND_F64
    yield eng, idx, q_raw, tags, stored, qb, all64
    eng.close()


def test_after_bf16_index_matches_oracle_in_gaps(gpu, oracle, bf16_case):
    """The EXT branch of the bf16 scan.  No bit-exact oracle exists for it, so the yardstick is test_gpu_bf16_corpus.py's: fp64
    scores of the stored rows and the bf16-rounded queries, scores within TOL, swaps only between ties.  Every bound is the
    midpoint of a gap of the fp64 ranking at least 4 TOL wide (searched forward from rank 11 q + 3, found within 50 ranks):
    a row's kernel score is within TOL of its fp64 score, so it lies on the same side of the bound."""
    eng, idx, q_raw, tags, stored, qb, all64 = bf16_case
    n, nq = all64.shape[1], all64.shape[0]
    _, filt, mask = mixed_filters(nq)
    for f, m, k in ((None, None, 10), (None, None, 32), (filt, mask, 10)):
        a_s = np.full(nq, NEG_INF, dtype=np.float32)
        want_i = np.full((nq, k), -1, dtype=np.int64)
        for q in range(nq):
            ok = np.ones(n, dtype=bool)
            if f is not None and f[q] >= 0:
                ok &= (tags & m[q]) == f[q]
            rows = np.flatnonzero(ok).astype(np.int64)
            if len(rows) == 0:
                continue                                     # a filter value no row carries: nothing, whatever the bound
            s = all64[q, rows]
            order = np.lexsort((rows, -s))
            s, rows = s[order], rows[order]
            j0 = (11 * q + 3) % (len(rows) - 60)
            j = next((j for j in range(j0, j0 + 50) if s[j] - s[j + 1] >= 4 * TOL), None)
            assert j is not None, (q, j0)                    # the precondition, checked on the CPU
            a_s[q] = np.float32((s[j] + s[j + 1]) / 2)
            assert s[j] - a_s[q] >= 1.9 * TOL and a_s[q] - s[j + 1] >= 1.9 * TOL
            want_i[q] = rows[j + 1:j + 1 + k]
        rs, ri = oracle.search(stored, qb, min(n, ORACLE_MAX_K), tags=tags, qfilter=f, qmask=m, kind=oracle.KIND_F64)
        for q in range(nq):      # the fp64 ranking above is oracle.search's
            w = want_i[q][want_i[q] >= 0]
            if len(w):
                at = int(np.flatnonzero(ri[q] == w[0])[0])
                assert np.array_equal(ri[q, at:at + len(w)], w[:len(ri[q]) - at])
        for row in (-1, I64_MAX):                            # no score equals a midpoint: the row cannot matter
            s, i = Device(gpu, idx, q_raw, f, m).after(a_s, np.full(nq, row, dtype=np.int64), k)
            assert _swaps_are_ties(i, want_i, all64), (k, row, i[:2], want_i[:2])
            valid = want_i >= 0
            assert np.array_equal(i >= 0, valid) and np.all(np.isneginf(s[~valid]))
            got = np.take_along_axis(all64, np.clip(i, 0, None), 1)
            assert np.all(np.abs(s[valid].astype(np.float64) - got[valid]) <= TOL)
            assert np.all(s[valid] < np.repeat(a_s[:, None], k, axis=1)[valid])


def test_after_bf16_pages_chain_to_the_k70_search(gpu, bf16_case):
    """Needs no oracle: ten pages of 7, each bounded by the GPU's own previous last hit, are the bf16 index's own
    ``search(q, 70)``, id for id and bit for bit, without a repeated id and with non-increasing scores."""
    eng, idx, q_raw, tags, stored, qb, all64 = bf16_case
    nq = q_raw.shape[0]
    _, filt, mask = mixed_filters(nq)
    for f, m in ((None, None), (filt, mask)):
        dev = Device(gpu, idx, q_raw, f, m)
        a_s, a_r = np.full(nq, POS_INF), np.full(nq, -1, dtype=np.int64)
        pages = []
        for _ in range(10):
            s, i = dev.after(a_s, a_r, 7)
            pages.append((s, i))
            short = i[:, -1] < 0                              # ran out of rows: nothing ranks behind -inf
            a_s, a_r = np.where(short, NEG_INF, s[:, -1]), np.where(short, I64_MAX, i[:, -1])
        cs, ci = np.concatenate([p[0] for p in pages], axis=1), np.concatenate([p[1] for p in pages], axis=1)
        ks, ki = idx.search(q_raw, 70, q_filter=f, q_filter_mask=m)
        assert np.array_equal(ci, ki) and np.array_equal(cs.view(np.uint32), ks.view(np.uint32))
        for q in range(nq):
            live = ci[q][ci[q] >= 0]
            assert len(set(live.tolist())) == len(live) and np.all(np.diff(cs[q][:len(live)]) <= 0)
            assert np.all(ci[q][len(live):] == -1)
        assert np.count_nonzero(ci >= 0) > 0


# ---- 9. refusals

def test_after_refusals(gpu, states):
    import rassengine_amd._native as N
    eng, idx, case = states
    L = idx._L
    nq = 33
    dq = gpu.from_numpy(np.ascontiguousarray(np.resize(case.q_raw, (nq, case.dim)))).cuda()
    da_s = gpu.full((nq,), np.inf, dtype=gpu.float32, device="cuda")
    da_r = gpu.full((nq,), -1, dtype=gpu.int64, device="cuda")
    df = gpu.zeros((nq,), dtype=gpu.int32, device="cuda")
    dm = gpu.full((nq,), PMASK, dtype=gpu.int32, device="cuda")
    os_ = gpu.full((nq, 33), 7.0, dtype=gpu.float32, device="cuda")
    oi = gpu.full((nq, 33), 7, dtype=gpu.int64, device="cuda")
    gpu.cuda.synchronize()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(handle, n, k, flt=None, msk=None, a_s=da_s, a_r=da_r):
        rc = L.rass_index_search_device_after(handle, p(dq), n, k, p(flt), p(msk), p(a_s), p(a_r), p(os_), p(oi))
        eng.synchronize()
        return rc

    assert call(idx._h, 2, 5) == N.RASS_OK
    assert call(idx._h, 2, 5, a_s=None) == ERR_INVALID and call(idx._h, 2, 5, a_r=None) == ERR_INVALID
    assert call(idx._h, 0, 5) == ERR_INVALID and call(idx._h, 33, 5) == ERR_INVALID
    assert call(idx._h, 2, 0) == ERR_INVALID and call(idx._h, 2, 33) == ERR_INVALID
    assert call(idx._h, 2, 5, None, dm) == ERR_INVALID
    assert call(idx._h, 2, 5, df, dm) == N.RASS_OK
    assert call(idx._h, 32, 32) == N.RASS_OK
    # an empty index: nothing, for every query
    for dtype in ("f32", "bf16"):
        empty = eng.open_index("after-empty-" + dtype, dtype=dtype)
        assert empty.rows == 0
        os_.fill_(7.0)
        oi.fill_(7)
        gpu.cuda.synchronize()
        assert call(empty._h, 32, 32) == N.RASS_OK
        s, i = os_.cpu().numpy().reshape(-1)[:32 * 32], oi.cpu().numpy().reshape(-1)[:32 * 32]
        assert np.all(np.isneginf(s)) and np.all(i == -1), dtype


# ---- 10. the serving shard

def test_after_through_the_serving_shard(gpu, oracle):
    """``serving.HipServingShard.search_packed(after=...)`` on one GPU, no process group: the packed record (scores at offset 0,
    ids at ``record_bytes(nq, k)[0]``) holds exactly the oracle's cut; ``after=None`` holds the oracle's top-k."""
    from rassengine_amd.engine import Engine
    from rassengine_amd.serving import HipServingShard
    n, nq, k = 2000, 12, 10
    tags = tagged(n, 31)
    case = Corpus(gpu, oracle, n, 128, nq, seed=8000, tags=tags)
    plain, filt, mask = mixed_filters(nq)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("after-shard")
        idx.add(case.xn, tags=tags, normalize=False)
        shard = HipServingShard(idx)                      # the engine now works on torch's current stream
        dq = gpu.from_numpy(case.q_raw).cuda()
        ids_off, size = shard.record_bytes(nq, k)
        assert ids_off == nq * k * 4 and size == ids_off + nq * k * 8

        def unpack(rec):
            gpu.cuda.synchronize()
            assert rec.dtype == gpu.uint8 and rec.numel() >= size
            raw = rec.cpu().numpy()
            return (raw[:nq * k * 4].view(np.float32).reshape(nq, k).copy(),
                    raw[ids_off:ids_off + nq * k * 8].view(np.int64).reshape(nq, k).copy())

        for what, f, m in (("plain filter", plain, None), ("masked filter", filt, mask)):
            ranked = case.ranked(qfilter=f, qmask=m)
            df = gpu.from_numpy(f).cuda()
            dm = None if m is None else gpu.from_numpy(m).cuda()
            a_s, a_r = bounds_at(ranked, lambda q, n_: (37 * q + 5) % max(n_ - 40, 1))
            want = expect(ranked, a_s, a_r, k)
            assert np.count_nonzero(want[1] >= 0) > 0 and np.any(want[1] == -1)
            rec = shard.search_packed(dq, k, df, dm, after=(gpu.from_numpy(a_s), gpu.from_numpy(a_r)))   # host tensors, as the server passes them
            assert_same(unpack(rec), want, f"search_packed(after), {what}")
            out = gpu.zeros((size + 8,), dtype=gpu.uint8, device="cuda")                                  # a record with a tail
            assert shard.search_packed(dq, k, df, dm, after=(gpu.from_numpy(a_s).cuda(), gpu.from_numpy(a_r).cuda()), out=out) is out
            assert_same(unpack(out), want, f"search_packed(after, out=), {what}")
            assert np.all(out.cpu().numpy()[size:] == 0)
            top = expect(ranked, np.full(nq, POS_INF), np.full(nq, -1, dtype=np.int64), k)
            assert_same(unpack(shard.search_packed(dq, k, df, dm)), top, f"search_packed(after=None), {what}")
    finally:
        eng.reset_stream()
        eng.close()
