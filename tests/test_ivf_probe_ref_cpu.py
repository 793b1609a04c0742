"""The conditions tests/test_gpu_ivf_probe.py rests on, checked on the reference alone (tests/ivf_probe_ref.py, no GPU): every
case finds its queries in the pool; the chosen queries have the coarse gap at their nprobe boundary and restricted answers
free of near-ties; in the limit world every far list scores below every near one; the duplicate-centroid queries put the pair
where their case needs it; and the inputs can tell three wrong engines from the right one — one that drops the list at rank
nprobe, one that adds the list at rank nprobe + 1, one that resolves a tie the other way — by the rows scanned or the top-k
of the query searched alone.  (Inside a full group of 32 the union of the probed lists can hide one query's list: that is
why the GPU cases run nq 1 and the short last groups of nq 33 and 70 as well.)  A GPU failure can then only be the engine's."""
import numpy as np
import pytest

import ivf_probe_ref as R
from nonfinite_ref import TOL_F64, no_near_ties


def test_the_rules_on_a_hand_made_ranking():
    cent = np.eye(6, dtype=np.float32)
    cent[4] = cent[1]                                                   # list 4 is a bit copy of list 1
    qn = np.array([[0.5, 0.7, 0.1, 0.3, 0.0, 0.4]], dtype=np.float32)
    s, order = R.ranking(cent, qn)
    assert order[0].tolist() == [1, 4, 0, 5, 3, 2] and s[0, 1] == s[0, 4]
    assert R.probed_topn(order[0], 1).tolist() == [1] and R.probed_topn(order[0], 9).tolist() == [1, 4, 0, 5, 3, 2]
    assert R.probed_threshold(s[0], order[0], 1).tolist() == [1, 4]     # the tie is probed whole
    assert R.probed_threshold(s[0], order[0], 3).tolist() == [0, 1, 4]
    assert R.probed_threshold(s[0], order[0], 100).tolist() == [0, 1, 2, 3, 4, 5]
    # the work list of two queries over lists of 0, 33, 64 and 70 rows
    tile0, lens = [0, 0, 2, 4], [0, 33, 64, 70]
    items, scanned = R.work_list([[1, 0], [3, 1, -1]], tile0, lens, 32)
    assert items == [(0, 32, 3), (1, 1, 3), (4, 32, 2), (5, 32, 2), (6, 6, 2)] and scanned == 103
    items, scanned = R.work_list([[2], [2], [3]], [0, 0, 1, 2], lens, 64)
    assert items == [(1, 64, 3), (2, 64, 4), (3, 6, 4)] and scanned == 134


def test_the_plan_fits_a_cu_where_the_host_says_so():
    assert R.plan_lds_bytes(32768, 0, 0) == 135168 <= R.CU_LDS_BYTES == 163840
    assert R.batch_coarse_lists(32768, 32) == 8 and R.plan_lds_bytes(32768, 8, 32) == 200704 > R.CU_LDS_BYTES
    assert R.batched_plan_fits(23552, 32) and not R.batched_plan_fits(23553, 32)
    assert R.batched_plan_fits(R.WIDE_NLIST, 32) and not R.batched_plan_fits(R.WIDE_NLIST, 33)
    assert R.batched_plan_fits(R.LIMIT_NLIST, 1) and not R.batched_plan_fits(R.LIMIT_NLIST, 32)   # the two limit-world batch cases
    assert [R.batch_coarse_lists(R.WIDE_NLIST, p) * p for p in R.BATCH_NPROBES] == [8, 64, 136, 256]


def _vetted(w, qs, nprobe, slabs, flts=(None,), delta=False, boundary=True):
    """The gap and the near-tie conditions of a chosen set, asserted directly."""
    p = min(nprobe, w.nlist)
    for j, q in enumerate(qs):
        if p < w.nlist:
            assert w.gap[q, p - 1] > R.COARSE_GAP
        if boundary:
            assert w.slab_len[w.order[q, p - 1]] > 0 and (p == w.nlist or w.slab_len[w.order[q, p]] > 0)
        for flt in flts:
            f, m = (None, None) if flt is None else flt(j)
            assert no_near_ties(w.top("f32", q, R.K + 1, nprobe, f, m, delta)[0][None], TOL_F64)
            if "bf16" in slabs:
                assert no_near_ties(w.top("bf16", q, R.K + 1, nprobe, f, m, delta)[0][None], TOL_F64)


@pytest.mark.parametrize("dim", R.WIDE_DIMS)
def test_wide_world(dim):
    w = R.Wide(dim)
    slabs = R.wide_slabs(dim)
    assert w.nlist == 1100 and w.covered % 32 == 0 and 3500 <= w.covered <= 4500 and w.delta == 45
    assert all(w.slab_len[l] == n for l, n in R.WIDE_FIXED.items())
    plain = np.ones(w.nlist, dtype=bool)
    plain[list(R.WIDE_FIXED)] = False
    assert w.slab_len[plain].min() == 0 and w.slab_len[plain].max() <= 6
    plan = R.wide_plan(w)
    for case, nqs in (("deep", R.DEEP_NQS), ("batch", R.BATCH_NQS)):
        for nprobe, qs in plan[case].items():
            assert len(qs) == max(nqs) == len(set(qs.tolist()))
            _vetted(w, qs, nprobe, slabs, (None, R.plain_filter))
            for j, q in enumerate(qs):                                  # the wrong engines
                right = w.lists(q, nprobe)
                wrong = R.perturbed(w, q, nprobe)
                assert set(wrong) == ({"drop", "add"} if min(nprobe, w.nlist) < w.nlist else {"drop"})
                for name, lists in wrong.items():
                    assert R.tells_apart(w, "f32", q, R.K, right, lists), (case, nprobe, j, name)
    # the probe sets are what the rules say: nprobe lists, or all of them
    q = int(plan["deep"][500][0])
    assert len(w.lists(q, 500)) == 500 and len(w.lists(q, 100000)) == 1100 and len(w.lists(q, 8)) == 8
    # a deep group's work list: its rows are the rows scanned, tiles ascend, and the masks name the probing queries
    qs = plan["deep"][64][:32]
    tile0 = np.concatenate([[0], np.cumsum(-(-w.slab_len // 32))[:-1]])
    items, scanned = R.work_list([w.lists(q, 64) for q in qs], tile0, w.slab_len, 32)
    assert scanned == sum(r for _, r, _ in items) == w.scanned_groups(qs, 64)[0]
    assert [t for t, _, _ in items] == sorted(t for t, _, _ in items) and all(0 < m < 1 << 32 for _, _, m in items)
    _vetted(w, plan["delta"], R.DELTA_NPROBE, slabs, (R.masked_filter,), delta=True)
    for j, q in enumerate(plan["allow"]):
        rs = w.top_of("f32", q, R.K + 1, w.lists(q, R.DELTA_NPROBE), delta=True, allow=R.allow_bits(w, j))[0]
        assert no_near_ties(rs[None], TOL_F64) and w.gap[q, R.DELTA_NPROBE - 1] > R.COARSE_GAP
    if dim != R.TIE_DIM:
        assert not plan["ties"]
        return
    # the duplicate centroids: every pair has queries that put it at ranks r, r + 1 on both sides of the 32-list rule change
    rank = np.argsort(w.order, axis=1)
    for pair in R.TIE_PAIRS:
        rs = [r for p, _, r in plan["ties"] if p == pair]
        assert any(r + 1 <= 32 for r in rs) and any(r >= 33 for r in rs), (pair, rs)
    assert any(r == 1 for _, _, r in plan["ties"])
    for (lo, hi), q, r in plan["ties"]:
        assert w.slab_len[lo] != w.slab_len[hi] and min(w.slab_len[lo], w.slab_len[hi]) > 0
        assert rank[q, lo] == r - 1 and rank[q, hi] == r and w.scores[q, lo] == w.scores[q, hi]
        assert r == 1 or w.gap[q, r - 2] > R.COARSE_GAP
        assert w.gap[q, r] > R.COARSE_GAP and w.gap[q, r - 1] == 0
        right = w.lists(q, r)
        if r + 1 <= 32:
            assert lo in right and hi not in right and len(right) == r
            wrong = np.array([hi if l == lo else l for l in right])     # the tie resolved the other way
        else:
            assert lo in right and hi in right and len(right) == r + 1
            wrong = np.setdiff1d(right, [hi])                            # a strict top-nprobe: the tie cut
        assert R.tells_apart(w, "f32", q, R.K, right, wrong)
        if r == 1:                                                       # ... and here by the answer as well as by the rows scanned
            assert not np.array_equal(w.top_of("f32", q, R.K, right)[1], w.top_of("f32", q, R.K, wrong)[1])
        group = plan["tie_groups"][(q, r)]
        assert len(group) == 32 and group[5] == q and len(set(group.tolist())) == 32
        _vetted(w, np.delete(group, 5), r, slabs)
        assert no_near_ties(w.top("f32", q, R.K + 1, r)[0][None], TOL_F64)


def test_limit_world():
    w = R.Limit()
    assert w.nlist == 32768 and w.is_near.sum() == 96 and all(w.is_near[l] for l in R.LIMIT_NEAR_FIXED)
    assert 2500 <= w.covered <= 4000 and np.count_nonzero(w.slab_len) == 96 + len(R.LIMIT_FAR_WITH_ROWS)
    assert not any(w.is_near[l] for l in R.LIMIT_FAR_WITH_ROWS)
    # every pool query scores every far list below every near list, by the gap and more
    assert np.all(w.scores[:, w.is_near].min(axis=1) - w.scores[:, ~w.is_near].max(axis=1) > R.COARSE_GAP)
    plan = R.limit_plan(w)
    for nprobe, qs in plan["probe"].items():
        assert len(qs) == R.LIMIT_BATCH_NQ
        _vetted(w, qs, nprobe, ("f32",))
        for q in qs:
            right = w.lists(q, nprobe)
            assert np.all(w.is_near[right]) and len(right) == nprobe
            for name, lists in R.perturbed(w, q, nprobe).items():
                assert R.tells_apart(w, "f32", q, R.K, right, lists), (nprobe, name)
    _vetted(w, plan["full"], R.LIMIT_NLIST, ("f32",), boundary=False)
    assert w.scanned(plan["full"][:1], R.LIMIT_NLIST) == int(w.slab_len.sum())
