"""Grouped (collapsed) search against the CPU oracle: ``rass_index_search_grouped`` and ``rass_index_search_grouped_device``.

The expected answer never comes from the engine.  The scores are the oracle's emulation of the scan's fmaf order
(``KIND_F32_MFMA``, the kind ``test_scan_matches_oracle`` holds the top-k scan to) for the queries as the GPU normalised
them.  Per query the live, filter-passing rows are ranked by ``np.lexsort((rows, -s))`` (score desc, row asc); a group's
representative is its first row in that order, and the groups are listed in the order of their representatives.  The group
of a row is ``(tag & group_mask) >> ctz(group_mask)``; a row whose key is ``>= n_groups`` is left out.  Scores, ids, groups
and totals must be EQUAL: no tolerance anywhere in this file.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24


class Corpus:
    """Rows and queries of one case with the oracle's score matrix, computed once and never changed by a test."""

    def __init__(self, torch, oracle, n, dim, nq, seed, edit=None):
        from rassengine_amd import ops
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.nq = n, dim, nq
        self.xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0     # un-normalised on purpose
        if edit is not None:
            edit(self)
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)


def group_keys(tags, group_mask):
    shift = (group_mask & -group_mask).bit_length() - 1
    return (tags.astype(np.int64) & group_mask) >> shift


def expect(case, tags, group_mask, n_groups, k, qfilter=None, qmask=None, ids=None, qsel=None):
    """(scores [nq, k], ids, groups, totals, status) the entry points must return.  ``ids``: reported id per row."""
    qsel = range(case.nq) if qsel is None else qsel
    nq = len(qsel)
    row_id = np.arange(case.n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    keys = group_keys(tags, group_mask)
    es = np.full((nq, k), NEG_INF, dtype=np.float32)
    ei = np.full((nq, k), -1, dtype=np.int64)
    eg = np.full((nq, k), -1, dtype=np.int32)
    et = np.zeros(nq, dtype=np.int64)
    status = 0
    for j, q in enumerate(qsel):
        ok = tags != -1
        if qfilter is not None and qfilter[q] >= 0:
            ok &= ((tags & qmask[q]) if qmask is not None else tags) == qfilter[q]
        if np.any(ok & (keys >= n_groups)):
            status = 1
        rows = np.flatnonzero(ok & (keys < n_groups))
        s = case.scores[q, rows]
        order = np.lexsort((rows, -s))
        rows, s = rows[order], s[order]
        _, first = np.unique(keys[rows], return_index=True)     # a group's best row = its first in the ranking
        first = np.sort(first)                                   # ... and the groups in the order of those rows
        et[j] = len(first)
        m = min(len(first), k)
        es[j, :m], ei[j, :m], eg[j, :m] = s[first[:m]], row_id[rows[first[:m]]], keys[rows[first[:m]]]
    return es, ei, eg, et, status


def run_device(torch, idx, q_raw, k, group_mask, n_groups, qfilter=None, qmask=None, id_base=0):
    nq = q_raw.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(q_raw)).cuda()
    df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter, dtype=np.int32)).cuda()
    dm = None if qmask is None else torch.from_numpy(np.ascontiguousarray(qmask, dtype=np.int32)).cuda()
    os_ = torch.full((nq, max(k, 1)), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, max(k, 1)), 7, dtype=torch.int64, device="cuda")
    og = torch.full((nq, max(k, 1)), 7, dtype=torch.int32, device="cuda")
    ot = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                        # the engine works on its own stream
    idx.search_grouped_device(dq.data_ptr(), nq, k, group_mask, n_groups, os_.data_ptr(), oi.data_ptr(), og.data_ptr(),
                              ot.data_ptr(), st.data_ptr(), id_base=id_base,
                              d_q_filter_ptr=0 if df is None else df.data_ptr(),
                              d_q_filter_mask_ptr=0 if dm is None else dm.data_ptr())
    idx.engine.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy(), og.cpu().numpy(), ot.cpu().numpy(), int(st.item())


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids", "groups", "totals")):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check_both(torch, idx, case, tags, group_mask, n_groups, k, qfilter=None, qmask=None, ids=None, what=""):
    """Host variant (any nq) and device variant (groups of <= 32) against the oracle's collapse."""
    want = expect(case, tags, group_mask, n_groups, k, qfilter, qmask, ids)
    assert want[4] == 0
    got = idx.search_grouped(case.q_raw, k, group_mask, n_groups, q_filter=qfilter, q_filter_mask=qmask)
    assert_same(got, want, what + " host")
    for q0 in range(0, case.nq, 32):
        sl = slice(q0, min(q0 + 32, case.nq))
        got = run_device(torch, idx, case.q_raw[sl], k, group_mask, n_groups, None if qfilter is None else qfilter[sl],
                         None if qmask is None else qmask[sl])
        assert got[4] == 0
        assert_same(got, tuple(w[sl] for w in want[:4]), what + " device")
    return want


def patient_tags(rng, n, n_groups, runs):
    """A patient code < n_groups per row — random, or dealt in runs of 32 adjacent rows (one document's chunks) — under a
    doc_type byte the patient mask must not see."""
    g = (np.arange(n) // 32) % n_groups if runs else rng.integers(0, n_groups, size=n)
    return (g | (rng.integers(1, 3, size=n) << DSHIFT)).astype(np.int32)


@pytest.mark.parametrize("n,dim,nq", [(1000, 100, 1), (3000, 256, 16), (3000, 1024, 17), (2500, 1024, 33), (2000, 1536, 32),
                                      (1500, 2048, 5)])
def test_grouped_matches_oracle(gpu, oracle, n, dim, nq):
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, n, dim, nq, seed=7000 + n + dim + nq)
    rng = np.random.default_rng(n + nq)
    eng = Engine(0, dim)
    try:
        for n_groups in (1, 7, 300):
            for runs in (False, True):
                tags = patient_tags(rng, n, n_groups, runs)
                idx = eng.open_index(f"grouped-{n_groups}-{int(runs)}")
                idx.add(case.xn, tags=tags, normalize=False)
                for k in (1, 10, 32, 33, 300):
                    want = check_both(gpu, idx, case, tags, PMASK, n_groups, k, what=f"groups {n_groups} runs {runs} k {k}")
                    assert np.all(want[3] == min(n_groups, len(np.unique(tags & PMASK))))
                eng.drop_index(idx.name)
    finally:
        eng.close()


@pytest.mark.parametrize("k", [4096, 4095])
def test_grouped_radix_select_at_the_cap(gpu, oracle, k):
    """5 000 distinct groups over 6 000 rows: more groups than k, so the k-th largest key is found by the radix select, and
    the total says 5 000."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 6000, 128, 3, seed=71)
    rng = np.random.default_rng(72)
    tags = np.concatenate([rng.permutation(5000), rng.integers(0, 5000, size=1000)]).astype(np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("radix")
        idx.add(case.xn, tags=tags, normalize=False)
        want = check_both(gpu, idx, case, tags, PMASK, 5000, k, what=f"k {k}")
        assert np.all(want[3] == 5000) and np.all(want[1] >= 0)
    finally:
        eng.close()


def test_grouped_full_grid_under_contention(gpu, oracle):
    """65 536 x 128, 32 queries: a workgroup on every CU.  8 groups, then ONE group — every workgroup races on the 32 slots,
    and the answer is search_ex(k = 1)."""
    from rassengine_amd.engine import Engine
    n = 65536
    case = Corpus(gpu, oracle, n, 128, 32, seed=73)
    eng = Engine(0, 128)
    try:
        tags8 = (np.random.default_rng(74).integers(0, 8, size=n)).astype(np.int32)
        idx = eng.open_index("grid8")
        idx.add(case.xn, tags=tags8, normalize=False)
        for k in (1, 8, 10):
            check_both(gpu, idx, case, tags8, PMASK, 8, k, what=f"8 groups k {k}")
        one = eng.open_index("grid1")
        one.add(case.xn, tags=np.zeros(n, dtype=np.int32), normalize=False)
        want = check_both(gpu, one, case, np.zeros(n, dtype=np.int32), PMASK, 1, 3, what="1 group")
        ks, ki = one.search(case.q_raw, 1)
        assert np.array_equal(want[1][:, 0], ki[:, 0]) and np.array_equal(want[0][:, 0].view(np.uint32), ks[:, 0].view(np.uint32))
        assert np.all(want[3] == 1) and np.all(want[1][:, 1:] == -1)
    finally:
        eng.close()


def test_grouped_every_row_its_own_group_is_search_ex(gpu, oracle):
    from rassengine_amd.engine import Engine
    n = 4096
    case = Corpus(gpu, oracle, n, 256, 6, seed=75)
    tags = np.arange(n, dtype=np.int32)
    eng = Engine(0, 256)
    try:
        idx = eng.open_index("own")
        idx.add(case.xn, tags=tags, normalize=False)
        for k in (10, 300):
            want = check_both(gpu, idx, case, tags, PMASK, n, k, what=f"k {k}")
            ks, ki = idx.search(case.q_raw, k)
            assert np.array_equal(want[1], ki) and np.array_equal(want[0].view(np.uint32), ks.view(np.uint32))
            assert np.array_equal(want[2], ki) and np.all(want[3] == n)
    finally:
        eng.close()


def test_grouped_ties(gpu, oracle):
    """Identical rows in different groups rank by id; identical rows inside one group elect the lowest row."""
    from rassengine_amd.engine import Engine
    copies = np.sort(np.random.default_rng(3).choice(500, 48, replace=False))

    def edit(c):
        c.xn[copies] = c.xn[copies[0]]
        c.q_raw[0] = c.xn[copies[0]] * 2.0

    case = Corpus(gpu, oracle, 500, 256, 2, seed=76, edit=edit)
    assert np.all(case.scores[0, copies] == case.scores[0, copies[0]]) and case.scores[0, copies[0]] == case.scores[0].max()
    eng = Engine(0, 256)
    try:
        across = np.arange(500, dtype=np.int32)[::-1].copy()             # every copy its own group, group ids descending
        idx = eng.open_index("ties-across")
        idx.add(case.xn, tags=across, normalize=False)
        want = check_both(gpu, idx, case, across, PMASK, 500, 64, what="across groups")
        assert np.array_equal(want[1][0, :48], copies)
        inside = np.full(500, 1, dtype=np.int32)
        inside[copies[:24]] = 5                                          # two groups of 24 identical rows each
        inside[copies[24:]] = 3
        idx = eng.open_index("ties-inside")
        idx.add(case.xn, tags=inside, normalize=False)
        want = check_both(gpu, idx, case, inside, PMASK, 6, 10, what="inside a group")
        assert list(want[1][0, :2]) == [copies[0], copies[24]] and list(want[2][0, :3]) == [5, 3, 1] and want[3][0] == 3
    finally:
        eng.close()


def test_grouped_tombstones_and_compaction(gpu, oracle):
    from rassengine_amd.engine import Engine
    n = 2000
    case = Corpus(gpu, oracle, n, 128, 5, seed=77)
    tags = np.random.default_rng(78).integers(0, 40, size=n).astype(np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("tomb")
        idx.add(case.xn, tags=tags, normalize=False)
        before = check_both(gpu, idx, case, tags, PMASK, 40, 50, what="live")
        assert np.all(before[3] == 40)
        # the best row of query 0's three best groups dies, and so does the whole of group 7
        dead = np.unique(np.concatenate([before[1][0, :3], np.flatnonzero(tags == 7)]))
        for r in dead:
            idx.delete(int(r))
        live = tags.copy()
        live[dead] = -1
        after = check_both(gpu, idx, case, live, PMASK, 40, 50, what="tombstones")
        assert np.all(after[3] == 39) and 7 not in after[2]
        for j in range(3):                            # the runner-up represents the group now
            g = tags[before[1][0, j]]
            if g == 7:
                continue
            rows = np.flatnonzero((live != -1) & (tags == g))
            runner = rows[np.lexsort((rows, -case.scores[0, rows]))][0]
            assert after[1][0][list(after[2][0]).index(g)] == runner
        new_row = idx.compact()
        want = expect(case, live, PMASK, 40, 50)
        moved = (want[0], np.where(want[1] >= 0, new_row[np.maximum(want[1], 0)], -1), want[2], want[3])
        assert np.all(moved[1][want[1] >= 0] >= 0)
        assert_same(idx.search_grouped(case.q_raw, 50, PMASK, 40), moved, "compacted host")
        got = run_device(gpu, idx, case.q_raw, 50, PMASK, 40)
        assert got[4] == 0
        assert_same(got, moved, "compacted device")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def small(gpu, oracle):
    """3 000 rows x 256 columns (a bf16 index needs whole 256-column units) with patient | doc_type tags, 9 queries, one
    engine: the filter, id, prefilter and refusal tests share it."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(99)
    n = 3000
    tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 4, size=n) << DSHIFT)).astype(np.int32)
    case = Corpus(gpu, oracle, n, 256, 9, seed=4243)
    eng = Engine(0, 256)
    idx = eng.open_index("grouped-small")
    idx.add(case.xn, tags=tags, normalize=False)
    yield eng, idx, case, tags
    eng.close()


def test_grouped_filters(gpu, small):
    eng, idx, case, tags = small
    nq = case.nq
    # collapse by patient under a doc_type masked filter (and two unfiltered queries, one value no row carries)
    filt = np.array([1 << DSHIFT, 2 << DSHIFT, -1, 3 << DSHIFT, 9 << DSHIFT, 1 << DSHIFT, -1, 2 << DSHIFT, 3 << DSHIFT], dtype=np.int32)
    mask = np.full(nq, DMASK, dtype=np.int32)
    want = check_both(gpu, idx, case, tags, PMASK, 6, 10, qfilter=filt, qmask=mask, what="patients under a doc_type filter")
    assert want[3][4] == 0 and np.all(want[1][4] == -1) and np.all(np.isneginf(want[0][4])) and np.all(want[3][[0, 2]] == 6)
    # collapse by doc type under a patient masked filter
    filt = np.array([0, 1, 2, 3, 4, 5, -1, 77, 2], dtype=np.int32)
    mask = np.full(nq, PMASK, dtype=np.int32)
    want = check_both(gpu, idx, case, tags, DMASK, 4, 4, qfilter=filt, qmask=mask, what="doc types under a patient filter")
    assert np.all(want[3][:7] == 3) and want[3][7] == 0 and 0 not in want[2][0, :3]
    # a plain (whole-tag) patient filter: one group
    plain = np.array([0 | (1 << DSHIFT), 3 | (2 << DSHIFT), -1, 5 | (3 << DSHIFT), 99, 1 | (1 << DSHIFT), -1, 2 | (2 << DSHIFT),
                      4 | (3 << DSHIFT)], dtype=np.int32)
    want = check_both(gpu, idx, case, tags, PMASK, 6, 5, qfilter=plain, what="plain filter")
    assert list(want[3]) == [1, 1, 6, 1, 0, 1, 6, 1, 1]
    # a filter matching nothing for every query: empty lists, totals 0
    none = np.full(nq, 1234, dtype=np.int32)
    want = check_both(gpu, idx, case, tags, PMASK, 6, 5, qfilter=none, what="nothing matches")
    assert np.all(want[3] == 0) and np.all(want[1] == -1) and np.all(want[2] == -1)


def test_grouped_ignores_the_prefilter_mode(gpu, small):
    eng, idx, case, tags = small
    off = idx.search_grouped(case.q_raw, 4, PMASK, 6)
    idx.set_prefilter("int8")
    try:
        assert_same(idx.search_grouped(case.q_raw, 4, PMASK, 6), off, "int8 prefilter")
        check_both(gpu, idx, case, tags, PMASK, 6, 4, what="int8 prefilter vs oracle")
    finally:
        idx.set_prefilter(False)


def test_grouped_id_base_on_the_device_variant(gpu, small):
    eng, idx, case, tags = small
    es, ei, eg, et, _ = expect(case, tags, PMASK, 6, 8)
    ei = np.where(ei >= 0, ei + 7_000_000_000, -1)
    got = run_device(gpu, idx, case.q_raw, 8, PMASK, 6, id_base=7_000_000_000)
    assert got[4] == 0
    assert_same(got, (es, ei, eg, et), "id_base")


def test_grouped_reports_caller_assigned_ids(gpu, oracle):
    """An add_ex index (a shard of a multi-GPU index) reports its global ids, on both variants; id_base is ignored."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 700, 128, 4, seed=79)
    tags = np.random.default_rng(80).integers(0, 25, size=700).astype(np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], tags=tags[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], tags=tags[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(400)]).astype(np.int64)
        want = check_both(gpu, idx, case, tags, PMASK, 25, 30, ids=gids, what="global ids")
        got = run_device(gpu, idx, case.q_raw, 30, PMASK, 25, id_base=123)
        assert_same(got, want, "id_base ignored")
    finally:
        eng.close()


def test_grouped_refusals(gpu, small):
    import rassengine_amd._native as N
    eng, idx, case, tags = small
    L = idx._L
    q = np.ascontiguousarray(case.q_raw[:2])
    s = np.empty((2, 4097), dtype=np.float32)
    i = np.empty((2, 4097), dtype=np.int64)
    g = np.empty((2, 4097), dtype=np.int32)
    t = np.empty(2, dtype=np.int64)
    f = np.zeros(2, dtype=np.int32)
    m = np.full(2, PMASK, dtype=np.int32)

    def call(handle, k, group_mask, n_groups, flt=None, msk=None):
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        return L.rass_index_search_grouped(handle, p(q), 2, k, group_mask, n_groups, p(flt), p(msk), p(s), p(i), p(g), p(t))

    assert call(idx._h, 16, PMASK, 6) == N.RASS_OK
    assert call(idx._h, 0, PMASK, 6) == -1 and call(idx._h, 4097, PMASK, 6) == -1          # RASS_ERR_INVALID
    assert call(idx._h, 16, 0, 6) == -1 and call(idx._h, 16, -0x80000000, 6) == -1 and call(idx._h, 16, -1, 6) == -1
    assert call(idx._h, 16, PMASK, 0) == -1 and call(idx._h, 16, PMASK, (1 << 20) + 1) == -1
    assert call(idx._h, 16, PMASK, 1 << 20) == N.RASS_OK and list(t) == [6, 6]
    assert call(idx._h, 16, PMASK, 6, None, m) == -1
    assert call(idx._h, 16, PMASK, 6, f, m) == N.RASS_OK
    # a matching row's group key >= n_groups: the host call fails and says why ...
    assert call(idx._h, 16, PMASK, 4) == -1 and b"n_groups" in L.rass_last_error()
    assert call(idx._h, 16, PMASK, 4, np.array([2, 3], dtype=np.int32), m) == N.RASS_OK and list(t) == [1, 1]   # ... none matches: fine
    # ... the device variant flags it and answers for the other rows
    want = expect(case, tags, PMASK, 4, 10)
    assert want[4] == 1 and np.all(want[3] == 4)
    got = run_device(gpu, idx, case.q_raw, 10, PMASK, 4)
    assert got[4] == 1
    assert_same(got, want, "key out of range, device")
    with pytest.raises(N.RassError) as e:
        idx.search_grouped(case.q_raw, 10, PMASK, 4)
    assert e.value.code == -1
    # the device entry point refuses the same ranges itself (FlatIndex.search_grouped_device checks them first: go below it)
    dq = gpu.from_numpy(q).cuda()
    ds = gpu.empty((2, 16), dtype=gpu.float32, device="cuda")
    di = gpu.empty((2, 16), dtype=gpu.int64, device="cuda")
    dg = gpu.empty((2, 16), dtype=gpu.int32, device="cuda")
    dt = gpu.empty((2,), dtype=gpu.int64, device="cuda")
    dst = gpu.empty((1,), dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()

    def dcall(k, group_mask, n_groups):
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        return L.rass_index_search_grouped_device(idx._h, vp(dq), 2, k, group_mask, n_groups, None, None, 0, vp(ds), vp(di), vp(dg),
                                                  vp(dt), vp(dst))

    assert dcall(16, PMASK, 6) == N.RASS_OK
    idx.engine.synchronize()
    assert dst.item() == 0 and dt.tolist() == [6, 6]
    for bad in (dict(k=0), dict(k=4097), dict(group_mask=0), dict(group_mask=-1), dict(n_groups=0), dict(n_groups=(1 << 20) + 1)):
        kw = dict(dict(k=4, group_mask=PMASK, n_groups=6), **bad)
        assert dcall(kw["k"], kw["group_mask"], kw["n_groups"]) == -1, bad
        with pytest.raises(ValueError):
            run_device(gpu, idx, q, kw["k"], kw["group_mask"], kw["n_groups"])
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, q, 4, PMASK, 6, qfilter=None, qmask=m)
    assert e.value.code == -1
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, case.q_raw[np.zeros(33, dtype=np.int64)], 4, PMASK, 6)      # nq > 32 on the device variant
    assert e.value.code == -1
    bf = eng.open_index("grouped-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    assert call(bf._h, 16, PMASK, 6) == -5                                                  # RASS_ERR_UNSUPPORTED
    with pytest.raises(N.RassError) as e:
        run_device(gpu, bf, q, 4, PMASK, 6)
    assert e.value.code == -5
