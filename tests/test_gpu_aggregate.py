"""Semantic terms aggregation against the CPU oracle: ``rass_index_aggregate`` and ``rass_index_aggregate_device``.

The expected answer never comes from the engine.  The scores are the oracle's emulation of the scan's fmaf order
(``KIND_F32_MFMA``) for the queries as the GPU normalised them.  Per query the HITS are the live, filter-passing rows with
``s >= thr`` whose group key ``(tag & group_mask) >> ctz(group_mask)`` is ``< n_groups``; they are counted per key with
numpy, the buckets are ordered by ``np.lexsort((key, -count))`` and a bucket's best row is its first under
``np.lexsort((rows, -s))``.  Groups, counts, scores, ids, n_buckets and total_hits must be EQUAL: no tolerance anywhere in
this file.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
NAMES = ("groups", "counts", "scores", "ids", "n_buckets", "total_hits")


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
        self.ranked = -np.sort(-self.scores, axis=1)                            # per query, best first

    def at_rank(self, r):
        """One threshold per query: the score of its rank-r row (1-based).  That row itself must count: the test is >=."""
        return self.ranked[:, r - 1].copy()


def group_keys(tags, group_mask):
    shift = (group_mask & -group_mask).bit_length() - 1
    return (tags.astype(np.int64) & group_mask) >> shift


def expect(case, tags, group_mask, n_groups, size, thr, qfilter=None, qmask=None, ids=None, qsel=None):
    """(groups [nq, size], counts, scores, ids, n_buckets [nq], total_hits [nq], status) the entry points must return."""
    qsel = range(case.nq) if qsel is None else qsel
    nq = len(qsel)
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (case.nq,))
    row_id = np.arange(case.n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    keys = group_keys(tags, group_mask)
    eg = np.full((nq, size), -1, dtype=np.int32)
    ec = np.zeros((nq, size), dtype=np.int64)
    es = np.full((nq, size), NEG_INF, dtype=np.float32)
    ei = np.full((nq, size), -1, dtype=np.int64)
    eb = np.zeros(nq, dtype=np.int64)
    et = np.zeros(nq, dtype=np.int64)
    status = 0
    for j, q in enumerate(qsel):
        ok = tags != -1
        if qfilter is not None and qfilter[q] >= 0:
            ok &= ((tags & qmask[q]) if qmask is not None else tags) == qfilter[q]
        hit = ok & (case.scores[q] >= thr[q])
        if np.any(hit & (keys >= n_groups)):
            status = 1
        rows = np.flatnonzero(hit & (keys < n_groups))
        et[j] = len(rows)
        if len(rows) == 0:
            continue
        count = np.bincount(keys[rows], minlength=n_groups)
        key = np.flatnonzero(count)
        key = key[np.lexsort((key, -count[key]))]                # doc_count desc, then key asc
        eb[j] = len(key)
        s = case.scores[q, rows]
        order = np.lexsort((rows, -s))
        rows, s = rows[order], s[order]
        uk, first = np.unique(keys[rows], return_index=True)     # a bucket's best row = its first in the ranking
        best = dict(zip(uk.tolist(), first.tolist()))
        m = min(len(key), size)
        f = np.array([best[g] for g in key[:m].tolist()], dtype=np.int64)
        eg[j, :m], ec[j, :m], es[j, :m], ei[j, :m] = key[:m], count[key[:m]], s[f], row_id[rows[f]]
    return eg, ec, es, ei, eb, et, status


def run_device(torch, idx, q_raw, thr, size, group_mask, n_groups, qfilter=None, qmask=None, id_base=0):
    nq = q_raw.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(q_raw)).cuda()
    dt = torch.from_numpy(np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,)).copy()).cuda()
    df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter, dtype=np.int32)).cuda()
    dm = None if qmask is None else torch.from_numpy(np.ascontiguousarray(qmask, dtype=np.int32)).cuda()
    cols = max(size, 1)
    og = torch.full((nq, cols), 7, dtype=torch.int32, device="cuda")
    oc = torch.full((nq, cols), 7, dtype=torch.int64, device="cuda")
    os_ = torch.full((nq, cols), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, cols), 7, dtype=torch.int64, device="cuda")
    ob = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    ot = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                        # the engine works on its own stream
    idx.search_counts_device(dq.data_ptr(), nq, dt.data_ptr(), size, group_mask, n_groups, og.data_ptr(), oc.data_ptr(),
                             os_.data_ptr(), oi.data_ptr(), ob.data_ptr(), ot.data_ptr(), st.data_ptr(), id_base=id_base,
                             d_q_filter_ptr=0 if df is None else df.data_ptr(),
                             d_q_filter_mask_ptr=0 if dm is None else dm.data_ptr())
    idx.engine.synchronize()
    return (og.cpu().numpy(), oc.cpu().numpy(), os_.cpu().numpy(), oi.cpu().numpy(), ob.cpu().numpy(), ot.cpu().numpy(),
            int(st.item()))


def assert_same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check_both(torch, idx, case, tags, group_mask, n_groups, size, thr, qfilter=None, qmask=None, ids=None, what=""):
    """Host variant (any nq) and device variant (groups of <= 32) against the oracle's counts."""
    want = expect(case, tags, group_mask, n_groups, size, thr, qfilter, qmask, ids)
    assert want[6] == 0
    got = idx.search_counts(case.q_raw, thr, size, group_mask, n_groups, q_filter=qfilter, q_filter_mask=qmask)
    assert_same(got, want, what + " host")
    thr_q = np.broadcast_to(np.asarray(thr, dtype=np.float32), (case.nq,))
    for q0 in range(0, case.nq, 32):
        sl = slice(q0, min(q0 + 32, case.nq))
        got = run_device(torch, idx, case.q_raw[sl], thr_q[sl], size, group_mask, n_groups,
                         None if qfilter is None else qfilter[sl], None if qmask is None else qmask[sl])
        assert got[6] == 0
        assert_same(got, tuple(w[sl] for w in want[:6]), what + " device")
    return want


def patient_tags(rng, n, n_groups, runs):
    """A patient code < n_groups per row — random, or dealt in runs of 32 adjacent rows (one document's chunks: the hits of
    a half-wave share one group, the one-add-per-half path) — under a doc_type byte the patient mask must not see."""
    g = (np.arange(n) // 32) % n_groups if runs else rng.integers(0, n_groups, size=n)
    return (g | (rng.integers(1, 3, size=n) << DSHIFT)).astype(np.int32)


@pytest.mark.parametrize("n,dim,nq", [(1000, 100, 1), (3000, 256, 16), (3000, 1024, 17), (2500, 1024, 33), (2000, 1536, 32),
                                      (1500, 2048, 5)])
def test_aggregate_matches_oracle(gpu, oracle, n, dim, nq):
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, n, dim, nq, seed=9000 + n + dim + nq)
    rng = np.random.default_rng(n + nq)
    above = np.nextafter(case.ranked[:, 0], np.float32(np.inf))
    mixed = np.stack([case.at_rank(1), case.at_rank(10), case.at_rank(n // 2), above, np.full(nq, NEG_INF)])[
        np.arange(nq) % 5, np.arange(nq)]                                  # a different threshold per query within one call
    thresholds = {"rank 1": case.at_rank(1), "rank 10": case.at_rank(10), "rank n/2": case.at_rank(n // 2), "above the max": above,
                  "-inf": NEG_INF, "mixed": mixed}
    eng = Engine(0, dim)
    try:
        for n_groups in (1, 7, 300):
            for runs in (False, True):
                tags = patient_tags(rng, n, n_groups, runs)
                idx = eng.open_index(f"agg-{n_groups}-{int(runs)}")
                idx.add(case.xn, tags=tags, normalize=False)
                for name, thr in thresholds.items():
                    for size in (1, 5, 32, 33, 300):
                        want = check_both(gpu, idx, case, tags, PMASK, n_groups, size, thr,
                                          what=f"groups {n_groups} runs {runs} size {size} thr {name}")
                    g, c, _, _, nb, tot, _ = want                            # of size 300: every bucket is listed
                    assert np.all(c.sum(axis=1) == tot)
                    if name.startswith("rank"):                              # the boundary row itself counts
                        rank = {"rank 1": 1, "rank 10": 10, "rank n/2": n // 2}[name]
                        assert np.all(tot >= rank) and np.all(tot < rank + 3)
                    elif name == "above the max":
                        assert not tot.any() and not nb.any() and np.all(g == -1) and not c.any()
                    elif name == "-inf":
                        assert np.all(tot == n) and np.all(nb == min(n_groups, len(np.unique(tags & PMASK))))
                        if n_groups == 300:
                            # ties in doc_count are certain with 300 groups over these rows: they come out by key ascending
                            tie = (c[0, :-1] == c[0, 1:]) & (g[0, 1:] >= 0)
                            assert tie.any() and np.all(g[0, :-1][tie] < g[0, 1:][tie])
                eng.drop_index(idx.name)
    finally:
        eng.close()


def test_aggregate_full_grid_under_contention(gpu, oracle):
    """65 536 x 128, 32 queries, -inf: a workgroup on every CU, every (row, query) a hit.  ONE slot per query, then 8: the
    count must equal the number of live rows, whichever lanes and workgroups added it."""
    from rassengine_amd.engine import Engine
    n = 65536
    case = Corpus(gpu, oracle, n, 128, 32, seed=173)
    eng = Engine(0, 128)
    try:
        one = eng.open_index("grid1")
        zeros = np.zeros(n, dtype=np.int32)
        one.add(case.xn, tags=zeros, normalize=False)
        want = check_both(gpu, one, case, zeros, PMASK, 1, 3, NEG_INF, what="1 slot")
        assert np.all(want[1][:, 0] == n) and np.all(want[5] == n) and np.all(want[4] == 1) and np.all(want[0][:, 1:] == -1)
        ks, ki = one.search(case.q_raw, 1)
        assert np.array_equal(want[3][:, 0], ki[:, 0]) and np.array_equal(want[2][:, 0].view(np.uint32), ks[:, 0].view(np.uint32))
        for r in (5, 40000, 65535):
            one.delete(r)
            zeros[r] = -1
        want = check_both(gpu, one, case, zeros, PMASK, 1, 1, NEG_INF, what="1 slot, tombstones")
        assert np.all(want[1][:, 0] == n - 3)
        tags8 = (np.random.default_rng(174).integers(0, 8, size=n)).astype(np.int32)
        idx = eng.open_index("grid8")
        idx.add(case.xn, tags=tags8, normalize=False)
        for size in (1, 10):
            want = check_both(gpu, idx, case, tags8, PMASK, 8, size, NEG_INF, what=f"8 slots size {size}")
        assert np.all(want[1].sum(axis=1) == n)
        check_both(gpu, idx, case, tags8, PMASK, 8, 8, case.at_rank(1000), what="8 slots, rank 1000")
    finally:
        eng.close()


def test_aggregate_tie_straddles_the_size_cut(gpu, oracle):
    """Groups 0..5 hold 10, 7, 7, 7, 3 and 1 rows: the cut of size 2 and of size 3 falls inside the tie of three, which the
    group key decides."""
    from rassengine_amd.engine import Engine
    sizes = [10, 7, 7, 7, 3, 1]
    tags = np.random.default_rng(5).permutation(np.repeat(np.arange(6), sizes)).astype(np.int32)
    case = Corpus(gpu, oracle, len(tags), 128, 3, seed=175)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("ties")
        idx.add(case.xn, tags=tags, normalize=False)
        for size, listed in ((1, [0]), (2, [0, 1]), (3, [0, 1, 2]), (4, [0, 1, 2, 3]), (5, [0, 1, 2, 3, 4])):
            want = check_both(gpu, idx, case, tags, PMASK, 6, size, NEG_INF, what=f"size {size}")
            assert np.all(want[0] == np.array(listed)) and np.all(want[1] == np.array(sizes)[listed]) and np.all(want[4] == 6)
        # the same with the keys reversed: the tie is still cut by key, not by arrival or by score
        rev = (5 - tags).astype(np.int32)
        idx = eng.open_index("ties-rev")
        idx.add(case.xn, tags=rev, normalize=False)
        want = check_both(gpu, idx, case, rev, PMASK, 6, 3, NEG_INF, what="reversed")
        assert np.all(want[0] == np.array([5, 2, 3])) and np.all(want[1] == np.array([10, 7, 7]))
    finally:
        eng.close()


@pytest.mark.parametrize("size", [4096, 4095])
def test_aggregate_radix_select_at_the_cap(gpu, oracle, size):
    """5 000 non-empty groups over 6 000 rows: more buckets than ``size``, so the size-th largest key is found by the radix
    select, and n_buckets says 5 000."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 6000, 128, 3, seed=171)
    rng = np.random.default_rng(172)
    tags = np.concatenate([rng.permutation(5000), rng.integers(0, 5000, size=1000)]).astype(np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("radix")
        idx.add(case.xn, tags=tags, normalize=False)
        want = check_both(gpu, idx, case, tags, PMASK, 5000, size, NEG_INF, what=f"size {size}")
        assert np.all(want[4] == 5000) and np.all(want[5] == 6000) and np.all(want[0] >= 0)
        check_both(gpu, idx, case, tags, PMASK, 5000, size, case.at_rank(5500), what=f"size {size}, rank 5500")
    finally:
        eng.close()


def test_aggregate_all_counts_equal(gpu, oracle):
    """Every group holds one row: the high word of every sort key is 1 and all eight radix passes are decided by the low
    word, the group key.  The listed buckets are the lowest keys, ascending."""
    from rassengine_amd.engine import Engine
    n = 5000
    case = Corpus(gpu, oracle, n, 128, 2, seed=176)
    tags = np.random.default_rng(177).permutation(n).astype(np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("equal")
        idx.add(case.xn, tags=tags, normalize=False)
        for size in (1, 100, 4095, 4096):
            want = check_both(gpu, idx, case, tags, PMASK, n, size, NEG_INF, what=f"size {size}")
            assert np.all(want[0] == np.arange(size)) and np.all(want[1] == 1) and np.all(want[4] == n)
            assert np.array_equal(want[3][0], np.argsort(tags)[:size])
    finally:
        eng.close()


def test_aggregate_tombstones_and_compaction(gpu, oracle):
    from rassengine_amd.engine import Engine
    n = 2000
    case = Corpus(gpu, oracle, n, 128, 5, seed=177)
    tags = np.random.default_rng(178).integers(0, 40, size=n).astype(np.int32)
    thr = case.at_rank(1200)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("tomb")
        idx.add(case.xn, tags=tags, normalize=False)
        before = check_both(gpu, idx, case, tags, PMASK, 40, 50, thr, what="live")
        assert np.all(before[4] == 40)
        # the best row of query 0's three largest buckets dies, and so does the whole of group 7
        dead = np.unique(np.concatenate([before[3][0, :3], np.flatnonzero(tags == 7)]))
        for r in dead:
            idx.delete(int(r))
        live = tags.copy()
        live[dead] = -1
        after = check_both(gpu, idx, case, live, PMASK, 40, 50, thr, what="tombstones")
        assert np.all(after[4] == 39) and 7 not in after[0]
        for j in range(3):                            # the count dropped, and the runner-up is the bucket's best row now
            g = before[0][0, j]
            if g == 7:
                continue
            at = list(after[0][0]).index(g)
            assert after[1][0, at] == before[1][0, j] - 1
            rows = np.flatnonzero((live != -1) & (tags == g) & (case.scores[0] >= thr[0]))
            assert after[3][0, at] == rows[np.lexsort((rows, -case.scores[0, rows]))][0]
        new_row = idx.compact()
        want = expect(case, live, PMASK, 40, 50, thr)
        moved = (want[0], want[1], want[2], np.where(want[3] >= 0, new_row[np.maximum(want[3], 0)], -1), want[4], want[5])
        assert np.all(moved[3][want[3] >= 0] >= 0)
        assert_same(idx.search_counts(case.q_raw, thr, 50, PMASK, 40), moved, "compacted host")
        got = run_device(gpu, idx, case.q_raw, thr, 50, PMASK, 40)
        assert got[6] == 0
        assert_same(got, moved, "compacted device")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def small(gpu, oracle):
    """3 000 rows x 256 columns (a bf16 index needs whole 256-column units) with patient | doc_type tags, 9 queries, one
    engine: the filter, cross-check, id, prefilter, status and refusal tests share it."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(199)
    n = 3000
    tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 4, size=n) << DSHIFT)).astype(np.int32)
    case = Corpus(gpu, oracle, n, 256, 9, seed=5243)
    eng = Engine(0, 256)
    idx = eng.open_index("agg-small")
    idx.add(case.xn, tags=tags, normalize=False)
    yield eng, idx, case, tags
    eng.close()


def small_filters(nq):
    masked_dt = (np.array([1 << DSHIFT, 2 << DSHIFT, -1, 3 << DSHIFT, 9 << DSHIFT, 1 << DSHIFT, -1, 2 << DSHIFT, 3 << DSHIFT],
                          dtype=np.int32), np.full(nq, DMASK, dtype=np.int32))
    masked_p = (np.array([0, 1, 2, 3, 4, 5, -1, 77, 2], dtype=np.int32), np.full(nq, PMASK, dtype=np.int32))
    plain = (np.array([0 | (1 << DSHIFT), 3 | (2 << DSHIFT), -1, 5 | (3 << DSHIFT), 99, 1 | (1 << DSHIFT), -1, 2 | (2 << DSHIFT),
                       4 | (3 << DSHIFT)], dtype=np.int32), None)
    return masked_dt, masked_p, plain


def test_aggregate_filters(gpu, small):
    eng, idx, case, tags = small
    nq = case.nq
    masked_dt, masked_p, plain = small_filters(nq)
    for thr, name in ((NEG_INF, "-inf"), (case.at_rank(700), "rank 700")):
        # patients under a doc_type masked filter (and two unfiltered queries, one value no row carries)
        want = check_both(gpu, idx, case, tags, PMASK, 6, 10, thr, qfilter=masked_dt[0], qmask=masked_dt[1],
                          what=f"patients under a doc_type filter, {name}")
        assert want[4][4] == 0 and want[5][4] == 0 and np.all(want[0][4] == -1) and np.all(np.isneginf(want[2][4]))
        # doc types (the mask with its shift of 24) under a patient masked filter
        want = check_both(gpu, idx, case, tags, DMASK, 4, 4, thr, qfilter=masked_p[0], qmask=masked_p[1],
                          what=f"doc types under a patient filter, {name}")
        assert want[4][7] == 0 and 0 not in want[0][0, :3] and set(want[0][6, :3]) == {1, 2, 3}
        # a plain (whole-tag) filter: one bucket
        want = check_both(gpu, idx, case, tags, PMASK, 6, 5, thr, qfilter=plain[0], what=f"plain filter, {name}")
        assert np.all(want[4][[0, 1, 3, 5, 7, 8]] <= 1) and want[4][4] == 0
    assert list(want[4][[2, 6]]) == [6, 6]
    want = check_both(gpu, idx, case, tags, DMASK, 4, 4, NEG_INF, what="doc types, no filter")
    assert np.all(want[4] == 3) and np.all(want[5] == case.n) and np.all(want[0][:, 3] == -1)
    none = np.full(nq, 1234, dtype=np.int32)
    want = check_both(gpu, idx, case, tags, PMASK, 6, 5, NEG_INF, qfilter=none, what="nothing matches")
    assert not want[4].any() and not want[5].any() and np.all(want[0] == -1) and np.all(want[3] == -1)


def test_aggregate_agrees_with_range_and_grouped_search(gpu, small):
    """Cross-checks against the existing entry points on the same index: the hit total is the range search's, and with
    -inf every bucket's (score, id) is the grouped search's entry of that group."""
    eng, idx, case, tags = small
    nq = case.nq
    for flt in small_filters(nq) + ((None, None),):
        kw = {} if flt[0] is None else dict(q_filter=flt[0]) if flt[1] is None else dict(q_filter=flt[0], q_filter_mask=flt[1])
        for thr in (case.at_rank(1), case.at_rank(300), case.at_rank(2999), np.full(nq, NEG_INF)):
            got = idx.search_counts(case.q_raw, thr, 6, PMASK, 6, **kw)
            _, _, totals = idx.search_range(case.q_raw, thr, max_hits=16, **kw)
            assert np.array_equal(got[5], totals)
        g, c, s, i, nb, _ = idx.search_counts(case.q_raw, NEG_INF, 6, PMASK, 6, **kw)
        gs, gi, gg, gt = idx.search_grouped(case.q_raw, 6, PMASK, 6, **kw)
        assert np.array_equal(nb, gt)
        for q in range(nq):
            by_group = {int(k): (sc, ii) for k, sc, ii in zip(gg[q], gs[q], gi[q]) if k >= 0}
            assert {int(k) for k in g[q] if k >= 0} == set(by_group)
            for k, sc, ii in zip(g[q], s[q], i[q]):
                if k >= 0:
                    assert by_group[int(k)] == (sc, ii)


def test_aggregate_ignores_the_prefilter_mode(gpu, small):
    eng, idx, case, tags = small
    thr = case.at_rank(500)
    off = idx.search_counts(case.q_raw, thr, 4, PMASK, 6)
    idx.set_prefilter("int8")
    try:
        assert idx.prefilter_mode == "int8"                              # mode 2
        assert_same(idx.search_counts(case.q_raw, thr, 4, PMASK, 6), off, "int8 prefilter")
        check_both(gpu, idx, case, tags, PMASK, 6, 4, thr, what="int8 prefilter vs oracle")
    finally:
        idx.set_prefilter(False)


def test_aggregate_id_base_on_the_device_variant(gpu, small):
    eng, idx, case, tags = small
    thr = case.at_rank(900)
    eg, ec, es, ei, eb, et, _ = expect(case, tags, PMASK, 6, 8, thr)
    ei = np.where(ei >= 0, ei + 7_000_000_000, -1)
    got = run_device(gpu, idx, case.q_raw, thr, 8, PMASK, 6, id_base=7_000_000_000)
    assert got[6] == 0
    assert_same(got, (eg, ec, es, ei, eb, et), "id_base")


def test_aggregate_reports_caller_assigned_ids(gpu, oracle):
    """An add_ex index (a shard of a multi-GPU index) reports its global ids, on both variants; id_base is ignored."""
    from rassengine_amd.engine import Engine
    case = Corpus(gpu, oracle, 700, 128, 4, seed=179)
    tags = np.random.default_rng(180).integers(0, 25, size=700).astype(np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], tags=tags[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], tags=tags[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(400)]).astype(np.int64)
        thr = case.at_rank(400)
        want = check_both(gpu, idx, case, tags, PMASK, 25, 30, thr, ids=gids, what="global ids")
        got = run_device(gpu, idx, case.q_raw, thr, 30, PMASK, 25, id_base=123)
        assert_same(got, want, "id_base ignored")
    finally:
        eng.close()


def test_aggregate_status_word(gpu, small):
    """A HIT whose group key is >= n_groups is left out and flagged; a row with such a key BELOW the threshold is not."""
    import rassengine_amd._native as N
    eng, idx, case, tags = small
    outside = (tags & PMASK) >= 4                                     # patients 4 and 5 of 0..5
    want = expect(case, tags, PMASK, 4, 10, NEG_INF)
    assert want[6] == 1 and np.all(want[4] == 4) and np.all(want[5] == np.count_nonzero(~outside))
    got = run_device(gpu, idx, case.q_raw, NEG_INF, 10, PMASK, 4)
    assert got[6] == 1
    assert_same(got, want, "key out of range, device")
    with pytest.raises(N.RassError) as e:
        idx.search_counts(case.q_raw, NEG_INF, 10, PMASK, 4)
    assert e.value.code == -1 and "n_groups" in str(e.value)
    # just above the best row that carries such a key: those rows are no hits, nothing is flagged, the host call answers
    thr = np.nextafter(case.scores[:, outside].max(axis=1), np.float32(np.inf))
    want = check_both(gpu, idx, case, tags, PMASK, 4, 10, thr, what="out-of-range keys below the threshold")
    assert want[5].sum() > 0
    # at that row's own score it is a hit again
    thr = case.scores[:, outside].max(axis=1)
    assert expect(case, tags, PMASK, 4, 10, thr)[6] == 1 and run_device(gpu, idx, case.q_raw, thr, 10, PMASK, 4)[6] == 1
    # a filter that keeps them out: fine as well
    flt, msk = np.full(case.nq, 2, dtype=np.int32), np.full(case.nq, PMASK, dtype=np.int32)
    check_both(gpu, idx, case, tags, PMASK, 4, 10, NEG_INF, qfilter=flt, qmask=msk, what="out-of-range keys filtered out")


def test_aggregate_refusals(gpu, small):
    import rassengine_amd._native as N
    eng, idx, case, tags = small
    L = idx._L
    q = np.ascontiguousarray(case.q_raw[:2])
    g = np.empty((2, 4097), dtype=np.int32)
    c = np.empty((2, 4097), dtype=np.int64)
    s = np.empty((2, 4097), dtype=np.float32)
    i = np.empty((2, 4097), dtype=np.int64)
    b = np.empty(2, dtype=np.int64)
    t = np.empty(2, dtype=np.int64)
    f = np.zeros(2, dtype=np.int32)
    m = np.full(2, PMASK, dtype=np.int32)
    minus_inf = np.full(2, NEG_INF)

    def call(handle, size, group_mask, n_groups, flt=None, msk=None, thr=minus_inf):
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        return L.rass_index_aggregate(handle, p(q), 2, p(thr), size, group_mask, n_groups, p(flt), p(msk), p(g), p(c), p(s), p(i),
                                      p(b), p(t))

    assert call(idx._h, 16, PMASK, 6) == N.RASS_OK and list(b) == [6, 6] and list(t) == [case.n, case.n]
    assert call(idx._h, 0, PMASK, 6) == -1 and call(idx._h, 4097, PMASK, 6) == -1          # RASS_ERR_INVALID
    assert call(idx._h, 4096, PMASK, 6) == N.RASS_OK
    assert call(idx._h, 16, 0, 6) == -1 and call(idx._h, 16, -0x80000000, 6) == -1 and call(idx._h, 16, -1, 6) == -1
    assert call(idx._h, 16, PMASK, 0) == -1 and call(idx._h, 16, PMASK, (1 << 20) + 1) == -1
    assert call(idx._h, 16, PMASK, 1 << 20) == N.RASS_OK and list(b) == [6, 6]
    assert call(idx._h, 16, PMASK, 6, None, m) == -1
    assert call(idx._h, 16, PMASK, 6, f, m) == N.RASS_OK
    assert call(idx._h, 16, PMASK, 6, thr=np.array([0.5, np.nan], dtype=np.float32)) == -1 and b"NaN" in L.rass_last_error()
    assert call(idx._h, 16, PMASK, 6, thr=None) == -1
    assert call(idx._h, 16, PMASK, 4) == -1 and b"n_groups" in L.rass_last_error()
    with pytest.raises(ValueError, match="NaN"):
        idx.search_counts(q, np.array([0.5, np.nan]), 16, PMASK, 6)
    # the device entry point refuses the same ranges itself (FlatIndex.search_counts_device checks them first: go below it)
    dq = gpu.from_numpy(q).cuda()
    dthr = gpu.from_numpy(minus_inf).cuda()
    dg = gpu.empty((2, 16), dtype=gpu.int32, device="cuda")
    dc = gpu.empty((2, 16), dtype=gpu.int64, device="cuda")
    ds = gpu.empty((2, 16), dtype=gpu.float32, device="cuda")
    di = gpu.empty((2, 16), dtype=gpu.int64, device="cuda")
    db = gpu.empty((2,), dtype=gpu.int64, device="cuda")
    dt = gpu.empty((2,), dtype=gpu.int64, device="cuda")
    dst = gpu.empty((1,), dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()

    def dcall(size, group_mask, n_groups):
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        return L.rass_index_aggregate_device(idx._h, vp(dq), 2, vp(dthr), size, group_mask, n_groups, None, None, 0, vp(dg), vp(dc),
                                             vp(ds), vp(di), vp(db), vp(dt), vp(dst))

    assert dcall(16, PMASK, 6) == N.RASS_OK
    idx.engine.synchronize()
    assert dst.item() == 0 and db.tolist() == [6, 6] and dt.tolist() == [case.n, case.n]
    for bad in (dict(size=0), dict(size=4097), dict(group_mask=0), dict(group_mask=-1), dict(n_groups=0),
                dict(n_groups=(1 << 20) + 1)):
        kw = dict(dict(size=4, group_mask=PMASK, n_groups=6), **bad)
        assert dcall(kw["size"], kw["group_mask"], kw["n_groups"]) == -1, bad
        with pytest.raises(ValueError):
            run_device(gpu, idx, q, NEG_INF, kw["size"], kw["group_mask"], kw["n_groups"])
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, q, NEG_INF, 4, PMASK, 6, qfilter=None, qmask=m)
    assert e.value.code == -1
    with pytest.raises(N.RassError) as e:
        run_device(gpu, idx, case.q_raw[np.zeros(33, dtype=np.int64)], NEG_INF, 4, PMASK, 6)    # nq > 32 on the device variant
    assert e.value.code == -1
    # a NaN threshold on the device variant, which reads nothing back, matches nothing
    got = run_device(gpu, idx, q, np.array([np.nan, NEG_INF], dtype=np.float32), 4, PMASK, 6)
    assert got[6] == 0 and list(got[5]) == [0, case.n] and list(got[4]) == [0, 6] and np.all(got[0][0] == -1)
    bf = eng.open_index("agg-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    assert call(bf._h, 16, PMASK, 6) == -5                                                  # RASS_ERR_UNSUPPORTED
    with pytest.raises(N.RassError) as e:
        run_device(gpu, bf, q, NEG_INF, 4, PMASK, 6)
    assert e.value.code == -5
