"""Score-threshold (range) search against the CPU oracle: ``rass_index_search_range`` and ``rass_index_search_range_device``.

The expected answer never comes from the engine's own top-k path.  The scores are the oracle's emulation of the scan's fmaf
order (``KIND_F32_MFMA``, the kind ``test_scan_matches_oracle`` holds the top-k scan to) for the queries as the GPU normalised
them, ranked (score desc, id asc) under the oracle's row rules (a tombstone never matches; a filter compares the tag, through
the mask where there is one) and cut at ``float32(score) >= threshold``.  ``oracle.search`` itself takes k <= 1 024
(``RASS_ORACLE_MAX_K``), fewer than most corpora here have rows, so the full ranking is ``oracle.scores`` of the same kind
sorted by numpy, and its first min(n, 1 024) entries must be ``oracle.search``'s answer, ids and scores, before anything is
compared with the GPU.  Ids, scores and totals must then be EQUAL: no tolerance anywhere in this file.

Thresholds are taken from the oracle's own sorted scores (rank j differs per query), so every count is known by construction
and the boundary row itself must be in (``>=``); plus one threshold above the maximum (0 hits) and ``-inf`` (every live row
the filter lets through).  Where a total exceeds ``max_hits`` the host variant must return the oracle's prefix and the device
variant the empty list, both with the exact total.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
ORACLE_MAX_K = 1024


class Corpus:
    """Rows, tags and queries of one case with the oracle's score matrix, computed once."""

    def __init__(self, torch, oracle, n, dim, nq, seed, tags=None):
        from rassengine_amd import ops
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.nq = n, dim, nq
        self.xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0     # un-normalised on purpose
        self.tags = tags
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self._oracle = oracle
        self.refresh()

    def refresh(self):
        """(Re)compute the score matrix: after the rows were edited by a test (ties)."""
        self.scores = self._oracle.scores(self.xn, self.qn_gpu, kind=self._oracle.KIND_F32_MFMA).astype(np.float32)

    def ranked(self, tags=None, qfilter=None, qmask=None, ids=None, check=True):
        """Per query the (scores f32, ids i64) of every matching row, score desc, id asc.  ``ids``: reported id per row."""
        tags = self.tags if tags is None else tags
        row_id = np.arange(self.n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
        out = []
        for q in range(self.nq):
            ok = np.ones(self.n, dtype=bool)
            if tags is not None:
                ok &= tags != -1
                if qfilter is not None and qfilter[q] >= 0:
                    ok &= ((tags & qmask[q]) if qmask is not None else tags) == qfilter[q]
            rows = np.flatnonzero(ok)
            s = self.scores[q, rows]
            order = np.lexsort((row_id[rows], -s))
            out.append((s[order], row_id[rows][order]))
        if check and ids is None:        # the ranking above IS oracle.search's as far as that reaches
            k = max(1, min(self.n, ORACLE_MAX_K))
            s_o, i_o = self._oracle.search(self.xn, self.qn_gpu, k, kind=self._oracle.KIND_F32_MFMA, tags=tags,
                                           qfilter=qfilter if tags is not None else None, qmask=qmask if tags is not None else None)
            for q, (s, i) in enumerate(out):
                m = min(k, len(i))
                assert np.array_equal(i_o[q, :m], i[:m]) and np.array_equal(s_o[q, :m].astype(np.float32), s[:m])
                assert np.all(i_o[q, m:] == -1)
        return out


def boundary_thresholds(ranked, span):
    """Query q's threshold = its own rank-j score, j different per query (0 hits' worth of rows: +inf)."""
    thr = np.empty(len(ranked), dtype=np.float32)
    for q, (s, _) in enumerate(ranked):
        thr[q] = s[(37 * q + 5) % min(len(s), span)] if len(s) else np.float32(np.inf)
    return thr


def expect(ranked, thr, max_hits, device):
    """(scores [nq, max_hits], ids, totals) the entry point must return."""
    nq = len(ranked)
    es = np.full((nq, max_hits), NEG_INF, dtype=np.float32)
    ei = np.full((nq, max_hits), -1, dtype=np.int64)
    et = np.zeros(nq, dtype=np.int64)
    for q, (s, i) in enumerate(ranked):
        m = int(np.count_nonzero(s >= thr[q]))      # the list is sorted: a prefix
        et[q] = m
        if device and m > max_hits:
            continue                                # the device variant: the empty list, the total says why
        m = min(m, max_hits)
        es[q, :m], ei[q, :m] = s[:m], i[:m]
    return es, ei, et


def run_device(torch, idx, q_raw, thr, max_hits, qfilter=None, qmask=None, id_base=0):
    nq = q_raw.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(q_raw)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)).cuda()
    df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter, dtype=np.int32)).cuda()
    dm = None if qmask is None else torch.from_numpy(np.ascontiguousarray(qmask, dtype=np.int32)).cuda()
    os_ = torch.full((nq, max_hits), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, max_hits), 7, dtype=torch.int64, device="cuda")
    ot = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                        # the engine works on its own stream
    idx.search_range_device(dq.data_ptr(), nq, dt.data_ptr(), max_hits, os_.data_ptr(), oi.data_ptr(), ot.data_ptr(),
                            id_base=id_base, d_q_filter_ptr=0 if df is None else df.data_ptr(),
                            d_q_filter_mask_ptr=0 if dm is None else dm.data_ptr())
    idx.engine.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy(), ot.cpu().numpy()


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids", "totals")):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check_both(torch, idx, case, ranked, thr, max_hits, qfilter=None, qmask=None, what=""):
    """Host variant (any nq) and device variant (groups of <= 32) against the oracle's cut."""
    got = idx.search_range(case.q_raw, thr, max_hits=max_hits, q_filter=qfilter, q_filter_mask=qmask)
    assert_same(got, expect(ranked, thr, max_hits, device=False), what + " host")
    for q0 in range(0, case.nq, 32):
        sl = slice(q0, min(q0 + 32, case.nq))
        got = run_device(torch, idx, case.q_raw[sl], thr[sl], max_hits, None if qfilter is None else qfilter[sl],
                         None if qmask is None else qmask[sl])
        assert_same(got, expect(ranked[sl], thr[sl], max_hits, device=True), what + " device")


@pytest.fixture(scope="module")
def small(gpu, oracle):
    """3 000 rows x 256 columns (a bf16 index needs whole 256-column units) with patient | doc_type tags, 9 queries, one
    engine: the index-state tests share it."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(99)
    n = 3000
    tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)
    case = Corpus(gpu, oracle, n, 256, 9, seed=4242, tags=tags)
    eng = Engine(0, 256)
    idx = eng.open_index("range-small")
    idx.add(case.xn, tags=tags, normalize=False)
    yield eng, idx, case
    eng.close()


@pytest.mark.parametrize("n,dim,nq", [
    (1, 100, 1), (33, 100, 17), (3000, 384, 32), (3000, 1024, 33), (3000, 1536, 16), (3000, 2048, 32),
    (40000, 1024, 32),      # a full grid with a ragged last tile: every workgroup adds to the same 32 counters
])
def test_range_matches_oracle(gpu, oracle, n, dim, nq):
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, n, dim, nq, seed=5000 + n + dim + nq)
    ranked = case.ranked()
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("range")
        idx.add(case.xn, normalize=False)
        max_hits = 256
        # ranks up to 299: most queries fit max_hits, those at rank >= 256 overflow it
        thr = boundary_thresholds(ranked, 300)
        for q, (s, _) in enumerate(ranked):
            assert s[(37 * q + 5) % min(len(s), 300)] == thr[q]          # the boundary row itself must be reported
        check_both(gpu, idx, case, ranked, thr, max_hits, what="boundary")
        above = np.array([np.nextafter(s[0], np.float32(np.inf)) for s, _ in ranked], dtype=np.float32)
        check_both(gpu, idx, case, ranked, above, max_hits, what="above the maximum")
        mixed = thr.copy()
        mixed[0::3] = NEG_INF                                             # every row matches
        if nq > 1:
            mixed[1::3] = above[1::3]                                     # none does
        check_both(gpu, idx, case, ranked, mixed, max_hits, what="-inf / boundary / above")
        got = idx.search_range(case.q_raw, np.full(nq, NEG_INF), max_hits=max_hits)
        assert np.all(got[2] == n)
    finally:
        eng.close()


@pytest.mark.parametrize("max_hits", [8, 4095, 4096])
def test_range_overflow(gpu, oracle, max_hits):
    """n = 5 000 with -inf thresholds: host = the best max_hits rows (the oracle's prefix), device = the empty list, and
    total = the live row count either way."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 5000, 128, 3, seed=61)
    ranked = case.ranked()
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("over")
        idx.add(case.xn, normalize=False)
        thr = np.full(case.nq, NEG_INF)
        s, i, t = idx.search_range(case.q_raw, thr, max_hits=max_hits)
        assert np.all(t == 5000) and np.all(i >= 0)
        check_both(gpu, idx, case, ranked, thr, max_hits)
        ds, di, dt = run_device(gpu, idx, case.q_raw, thr, max_hits)
        assert np.all(dt == 5000) and np.all(di == -1) and np.all(np.isneginf(ds))
    finally:
        eng.close()


def test_range_exactly_max_hits_live_rows(gpu, oracle):
    """4 097 live rows overflow max_hits = 4 096; with one of them tombstoned the 4 096 fit exactly."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 4097, 128, 2, seed=62)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("edge")
        idx.add(case.xn, normalize=False)
        thr = np.full(case.nq, NEG_INF)
        ranked = case.ranked()
        check_both(gpu, idx, case, ranked, thr, 4096, what="4097 live")
        assert np.all(idx.search_range(case.q_raw, thr, max_hits=4096)[2] == 4097)
        dead = int(ranked[0][1][100])                # a row inside query 0's list
        idx.delete(dead)
        tags = np.zeros(4097, dtype=np.int32)
        tags[dead] = -1
        ranked = case.ranked(tags=tags)
        check_both(gpu, idx, case, ranked, thr, 4096, what="4096 live")
        ds, di, dt = run_device(gpu, idx, case.q_raw, thr, 4096)
        assert np.all(dt == 4096) and np.all(di >= 0) and dead not in di
    finally:
        eng.close()


def test_range_ties_by_id(gpu, oracle):
    """64 copies of one vector: every copy is counted, the order among them is id ascending, and an overflowing host
    list keeps the lowest ids."""
    from rassengine_amd import ops
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 500, 256, 2, seed=63)
    copies = np.sort(np.random.default_rng(3).choice(500, 64, replace=False))
    case.xn[copies] = case.xn[copies[0]]
    case.q_raw[0] = case.xn[copies[0]] * 2.0
    case.qn_gpu = ops.normalize_rows(gpu.from_numpy(case.q_raw).cuda()).cpu().numpy()
    case.refresh()
    ranked = case.ranked()
    assert np.array_equal(ranked[0][1][:64], copies) and np.all(ranked[0][0][:64] == ranked[0][0][0])
    eng = Engine(0, 256)
    try:
        idx = eng.open_index("ties")
        idx.add(case.xn, normalize=False)
        thr = np.array([ranked[0][0][0], ranked[1][0][9]], dtype=np.float32)
        s, i, t = idx.search_range(case.q_raw, thr, max_hits=100)
        assert t[0] == 64 and np.array_equal(i[0, :64], copies) and t[1] == 10
        check_both(gpu, idx, case, ranked, thr, 100, what="ties")
        check_both(gpu, idx, case, ranked, thr, 40, what="ties, overflow")    # host: the 40 lowest ids of the 64
    finally:
        eng.close()


def test_range_filters(gpu, small):
    """Plain and masked filters, a filter value no row carries, unfiltered queries next to filtered ones."""
    eng, idx, case = small
    nq = case.nq
    plain = np.array([-1, 0 | (1 << 24), 1 | (2 << 24), 5 | (1 << 24), 99, -1, 3 | (2 << 24), 2 | (1 << 24), 4 | (2 << 24)], dtype=np.int32)
    ranked = case.ranked(qfilter=plain)
    assert len(ranked[4][1]) == 0
    for thr in (boundary_thresholds(ranked, 200), np.full(nq, NEG_INF)):
        check_both(gpu, idx, case, ranked, thr, 256, qfilter=plain, what="plain filter")
    got = idx.search_range(case.q_raw, np.full(nq, NEG_INF), max_hits=8, q_filter=plain)
    for q in range(nq):      # -inf with a patient filter: total = that patient's live row count
        assert got[2][q] == (case.n if plain[q] < 0 else np.count_nonzero(case.tags == plain[q]))
    pmask, dmask = 0x00FFFFFF, 0x7F000000
    filt = np.array([3, 2 << 24, -1, 0, 77, 1 << 24, 5, 4, 1 | (1 << 24)], dtype=np.int32)
    mask = np.array([pmask, dmask, -1, pmask, pmask, dmask, pmask, pmask, -1], dtype=np.int32)
    ranked = case.ranked(qfilter=filt, qmask=mask)
    assert len(ranked[4][1]) == 0 and len(ranked[1][1]) > 1024
    for thr in (boundary_thresholds(ranked, 300), np.full(nq, NEG_INF)):
        check_both(gpu, idx, case, ranked, thr, 256, qfilter=filt, qmask=mask, what="masked filter")


def test_range_consistent_with_search_ex(gpu, small):
    """The listed scores are search_ex(k = max_hits)'s scores for the same rows, bit for bit."""
    eng, idx, case = small
    ranked = case.ranked(check=False)
    thr = boundary_thresholds(ranked, 60)
    s, i, t = idx.search_range(case.q_raw, thr, max_hits=64)
    ks, ki = idx.search(case.q_raw, 64)
    for q in range(case.nq):
        m = int(t[q])
        assert 0 < m <= 64
        assert np.array_equal(i[q, :m], ki[q, :m]) and np.array_equal(s[q, :m].view(np.uint32), ks[q, :m].view(np.uint32))
        assert ks[q, m] < thr[q]


def test_range_ignores_the_prefilter_mode(gpu, small):
    """An int8-prefilter index answers as with the mode off, overflowing queries (the top-k fallback) included."""
    eng, idx, case = small
    ranked = case.ranked(check=False)
    thr = boundary_thresholds(ranked, 40)
    off = [idx.search_range(case.q_raw, thr, max_hits=m) for m in (8, 64)]
    idx.set_prefilter("int8")
    try:
        for m, want in zip((8, 64), off):
            assert_same(idx.search_range(case.q_raw, thr, max_hits=m), want, f"int8 prefilter, max_hits {m}")
            check_both(gpu, idx, case, ranked, thr, m, what=f"int8 prefilter vs oracle, max_hits {m}")
    finally:
        idx.set_prefilter(False)


def test_range_id_base_on_the_device_variant(gpu, small):
    eng, idx, case = small
    ranked = case.ranked(check=False)
    thr = boundary_thresholds(ranked, 50)
    es, ei, et = expect(ranked, thr, 64, device=True)
    ei = np.where(ei >= 0, ei + 7_000_000_000, -1)
    assert_same(run_device(gpu, idx, case.q_raw, thr, 64, id_base=7_000_000_000), (es, ei, et), "id_base")


def test_range_tombstones_and_compaction(gpu, oracle):
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 2000, 128, 5, seed=64)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("tomb")
        idx.add(case.xn, normalize=False)
        best = case.ranked()
        dead = np.unique(np.concatenate([np.random.default_rng(5).choice(2000, 150, replace=False),
                                         best[0][1][:3], best[1][1][4:6]]))          # some of the best rows die too
        for r in dead:
            idx.delete(int(r))
        tags = np.zeros(2000, dtype=np.int32)
        tags[dead] = -1
        ranked = case.ranked(tags=tags)
        for thr in (boundary_thresholds(ranked, 200), np.full(case.nq, NEG_INF)):
            check_both(gpu, idx, case, ranked, thr, 256, what="tombstones")
        assert np.all(idx.search_range(case.q_raw, np.full(case.nq, NEG_INF), max_hits=1)[2] == 2000 - len(dead))
        new_row = idx.compact()
        after = [(s, new_row[i]) for s, i in ranked]           # the live rows keep their order: new ordinals ascend with the old
        assert all(np.all(i >= 0) for _, i in after)
        for thr in (boundary_thresholds(ranked, 200), np.full(case.nq, NEG_INF)):
            check_both(gpu, idx, case, after, thr, 256, what="compacted")
    finally:
        eng.close()


def test_range_reports_caller_assigned_ids(gpu, oracle):
    """An add_ex index (a shard of a multi-GPU index) reports its global ids, on both variants; id_base is ignored."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 700, 128, 4, seed=65)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(400)]).astype(np.int64)
        ranked = case.ranked(ids=gids)
        thr = boundary_thresholds(ranked, 30)
        check_both(gpu, idx, case, ranked, thr, 32, what="global ids")
        assert_same(run_device(gpu, idx, case.q_raw, thr, 32, id_base=123), expect(ranked, thr, 32, device=True), "id_base ignored")
    finally:
        eng.close()


def test_range_refusals(gpu, small):
    import rassengine_amd._native as N
    eng, idx, case = small
    L = idx._L
    q = np.ascontiguousarray(case.q_raw[:2])
    s = np.empty((2, 4097), dtype=np.float32)
    i = np.empty((2, 4097), dtype=np.int64)
    t = np.empty(2, dtype=np.int64)
    f = np.zeros(2, dtype=np.int32)
    m = np.full(2, 0x00FFFFFF, dtype=np.int32)

    def call(handle, thr, max_hits, flt=None, msk=None):
        thr = np.asarray(thr, dtype=np.float32)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        return L.rass_index_search_range(handle, p(q), 2, p(thr), max_hits, p(flt), p(msk), p(s), p(i), p(t))

    ok = [0.0, 0.0]
    assert call(idx._h, ok, 16) == N.RASS_OK
    assert call(idx._h, ok, 0) == -1 and call(idx._h, ok, 4097) == -1                # RASS_ERR_INVALID
    assert call(idx._h, [0.0, np.nan], 16) == -1
    assert call(idx._h, ok, 16, None, m) == -1
    assert call(idx._h, ok, 16, f, m) == N.RASS_OK
    assert call(idx._h, [-np.inf, np.inf], 16) == N.RASS_OK and t[0] == case.n and t[1] == 0
    # the device variant: the same bounds; a NaN threshold cannot be refused without a read-back and matches nothing
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, q, ok, 0)
    assert e.value.code == -1
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, q, ok, 4097)
    assert e.value.code == -1
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, q, ok, 16, qfilter=None, qmask=m)
    assert e.value.code == -1
    ds, di, dt = run_device(gpu, idx, q, [np.nan, -np.inf], 16)
    assert dt[0] == 0 and np.all(di[0] == -1) and dt[1] == case.n
    bf = eng.open_index("range-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    assert call(bf._h, ok, 16) == -5                                                 # RASS_ERR_UNSUPPORTED
    with pytest.raises(N.RassError) as e:
        run_device(gpu, bf, q, ok, 16)
    assert e.value.code == -5
