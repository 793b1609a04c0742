"""The grouped search with inner hits over a key column: ``rass_index_search_group_hits_keys`` and its ``_device`` form.

The expected answer never comes from the engine: scores are the oracle's emulation of the scan's fmaf order
(``KIND_F32_MFMA``) for the queries as the GPU normalised them, grouping is ``tests/grouphits_ref.py``.  Everything is compared
bit for bit (scores as ``uint32``, ids, groups, totals); the HIP-against-HIP tests (``group_size = 1`` against the grouped
search of the existing kernel, one group / a cap no group reaches against ``search``) say so."""
import ctypes

import numpy as np
import pytest

import grouphits_ref as H
import groupkeys_ref as R
import nonfinite_ref as NF

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5          # RASS_ERR_INVALID, RASS_ERR_UNSUPPORTED
NEG_INF = R.NEG_INF
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
NAMES = ("scores", "ids", "groups", "totals", "capped scores", "capped ids")
N_ROWS = 1500                           # 46 tiles and a tail of 28 rows
# one dim per row-stride class (CH = 1 .. 8), 16 queries (NT = 1) and 17 (NT = 2): all 16 instantiations; two launch groups
SWEEP = [(N_ROWS, dim, nq) for dim in (100, 256, 384, 500, 640, 768, 872, 1024) for nq in (16, 17)] + [(N_ROWS, 1024, 33)]


class Corpus:
    """Rows, queries and tags of one shape with the oracle's score matrix, computed once and never changed by a test.  Rows 2,
    7, 40 and n - 1 are one vector: every query's scores tie there, and query 0's best rows ARE the tie."""

    def __init__(self, torch, oracle, n, dim, nq, seed=0):
        from rassengine_amd import ops
        rng = np.random.default_rng(9000 + n + dim + nq + seed)
        self.n, self.dim, self.nq = n, dim, nq
        x = rng.standard_normal((n, dim), dtype=np.float32)
        x[7] = x[40] = x[n - 1] = x[2]
        self.xn = oracle.normalize_ref(x).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0
        self.q_raw[0] = x[2] * 2.0
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 4, size=n) << DSHIFT)).astype(np.int32)
        self.dead = rng.permutation(n)[:max(1, n // 40)]
        self.live_tags = self.tags.copy()
        self.live_tags[self.dead] = -1


_CORPORA = {}


def corpus(gpu, oracle, shape):
    return _CORPORA.setdefault(shape, Corpus(gpu, oracle, *shape))


@pytest.fixture(scope="module")
def world(gpu, oracle):
    """shape -> (engine, index with tombstones, corpus); built on first use, shared by the tests of this file."""
    from rassengine_amd.engine import Engine
    made = {}

    def get(shape):
        if shape not in made:
            case = corpus(gpu, oracle, shape)
            eng = Engine(0, case.dim)
            idx = eng.open_index("hits")
            idx.add(case.xn, tags=case.tags, normalize=False)
            for r in case.dead:
                idx.delete(int(r))
            made[shape] = (eng, idx, case)
        return made[shape]

    yield get
    for eng, _, _ in made.values():
        eng.close()


def dev(torch, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def ptr(t):
    return 0 if t is None else t.data_ptr()


def words_of(torch, allow):
    return None if allow is None else dev(torch, R.pack_bits(allow).view(np.int32))


def run_device(torch, idx, q_raw, k, d_keys, n_groups, gs, capped, allow=None, qfilter=None, qmask=None, id_base=0):
    """The device variant on poisoned output arrays -> (scores, ids, groups, totals, capped scores, capped ids, status)."""
    nq = q_raw.shape[0]
    dq, df, dm = dev(torch, q_raw), dev(torch, qfilter, np.int32), dev(torch, qmask, np.int32)
    da = words_of(torch, allow)
    n_bitmaps, words = (0, 0) if da is None else ((1 if da.dim() == 1 else da.shape[0]), da.shape[-1])
    os_ = torch.full((nq, k, gs), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, k, gs), 7, dtype=torch.int64, device="cuda")
    og = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    ot = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    cs = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda") if capped else None
    ci = torch.full((nq, k), 7, dtype=torch.int64, device="cuda") if capped else None
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_group_hits_device(dq.data_ptr(), nq, k, d_keys.data_ptr(), d_keys.shape[0], n_groups, gs, os_.data_ptr(), oi.data_ptr(),
                                 og.data_ptr(), ot.data_ptr(), st.data_ptr(), d_out_capped_scores_ptr=ptr(cs), d_out_capped_ids_ptr=ptr(ci),
                                 d_allow_ptr=ptr(da), n_bitmaps=n_bitmaps, words_per_bitmap=words, id_base=id_base,
                                 d_q_filter_ptr=ptr(df), d_q_filter_mask_ptr=ptr(dm))
    idx.engine.synchronize()
    out = [os_.cpu().numpy(), oi.cpu().numpy(), og.cpu().numpy(), ot.cpu().numpy()]
    out += [cs.cpu().numpy(), ci.cpu().numpy()] if capped else []
    return tuple(out) + (int(st.item()),)


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        gb, wb = NF.bits(g), NF.bits(w)
        assert np.array_equal(gb, wb), (what, name, np.argwhere(gb != wb)[:5].tolist(), g[gb != wb][:5], w[gb != wb][:5])


def cut(full, k, gs, capped_from=None):
    """The answer at (k, gs) out of the restatement at (K >= k, GS >= gs): lists are prefixes.  The capped list depends on
    both and comes from a restatement of its own (``capped_from`` at exactly (k, gs))."""
    out = (full[0][:, :k, :gs].copy(), full[1][:, :k, :gs].copy(), full[2][:, :k].copy(), full[3])
    return out + (capped_from[4], capped_from[5]) if capped_from is not None else out


def check(torch, idx, case, tags, keys, n_groups, k, gs, full=None, allow=None, qfilter=None, qmask=None, ids=None, what=""):
    """Host and device variants at (k, gs) against the numpy answer, with the capped list where k * gs <= 4096."""
    capped = k * gs <= 4096
    exact = H.expect_group_hits(case.scores, tags, keys, n_groups, k, gs, allow, qfilter, qmask, ids) if capped or full is None else None
    want = cut(full, k, gs, exact) if full is not None else (exact[:6] if capped else exact[:4])
    assert (exact if exact is not None else full)[6] == 0
    d_keys = dev(torch, keys, np.int32)
    got = idx.search_group_hits(case.q_raw, k, d_keys, n_groups, gs, allow=words_of(torch, allow), q_filter=qfilter, q_filter_mask=qmask,
                                capped=capped)
    assert_same(got, want, what + " host")
    got = run_device(torch, idx, case.q_raw, k, d_keys, n_groups, gs, capped, allow, qfilter, qmask)
    assert got[-1] == 0
    assert_same(got[:-1], want, what + " device")
    return want


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_stride_sweep(gpu, world, shape):
    eng, idx, case = world(shape)
    n, dim, nq = shape
    rng = np.random.default_rng(n + dim + nq)
    styles = {"7 random": (rng.integers(0, 7, size=n), 7), "300 random": (rng.integers(0, 300, size=n), 300),
              "7 runs": ((np.arange(n) // 32) % 7, 7), "300 runs": ((np.arange(n) // 32) % 300, 300)}
    for name, (keys, n_groups) in styles.items():
        full = H.expect_group_hits(case.scores, case.live_tags, keys, n_groups, 300, 16)
        assert full[6] == 0
        for gs, k in ((1, 300), (2, 7), (3, 1), (3, 10), (8, 10), (16, 1), (16, 300)):
            check(gpu, idx, case, case.live_tags, keys, n_groups, k, gs, full=full, what=f"{name} gs {gs} k {k}")
        # group_size = 1 IS the grouped search of the existing kernel, on every output (HIP against HIP)
        d_keys = dev(gpu, keys, np.int32)
        for k in (1, 10, 300):
            hs, hi, hg, ht = idx.search_group_hits(case.q_raw, k, d_keys, n_groups, 1)
            assert_same((hs[:, :, 0], hi[:, :, 0], hg, ht), idx.search_grouped_by_keys(case.q_raw, k, d_keys, n_groups), f"{name} gs 1 k {k}")
    assert case.scores[0, 2] == case.scores[0, 7] == case.scores[0, 40] == case.scores[0, n - 1] == case.scores[0].max()


def test_full_grid_under_contention(gpu, oracle):
    """65 536 x 128, 32 queries: a workgroup on every CU.  8 groups, then ONE group with group_size 16 — every workgroup
    races on the 32 chains, and the answer is search(k = 16) (HIP against HIP, next to the restatement)."""
    from rassengine_amd.engine import Engine
    n = 65536
    case = Corpus(gpu, oracle, n, 128, 32, seed=73)
    tags = np.zeros(n, dtype=np.int32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("grid")
        idx.add(case.xn, tags=tags, normalize=False)
        keys8 = np.random.default_rng(74).integers(0, 8, size=n)
        for gs, k in ((16, 8), (3, 5)):
            check(gpu, idx, case, tags, keys8, 8, k, gs, what=f"8 groups gs {gs} k {k}")
        want = check(gpu, idx, case, tags, np.zeros(n, dtype=np.int64), 1, 3, 16, what="1 group")
        ks, ki = idx.search(case.q_raw, 16)
        assert np.array_equal(want[1][:, 0, :], ki) and np.array_equal(NF.bits(want[0][:, 0, :]), NF.bits(ks))
        assert np.all(want[3] == 1) and np.all(want[1][:, 1:] == -1) and np.all(want[2][:, 1:] == -1)
        assert np.array_equal(want[5], ki[:, :3])           # the cap of 16 binds nothing among the best 3
    finally:
        eng.close()


@pytest.mark.parametrize("nq", [16, 17])
@pytest.mark.parametrize("dim", [128, 1024])
def test_deep_loop_three_iterations_per_workgroup(gpu, world, dim, nq):
    """5 * CUs + 3 tiles and a tail of 7 rows (41 063 rows on 256 CUs): the scan launches one workgroup per CU, so every
    workgroup runs the pair loop three times, some over 5 tiles and some over 6.  A tile's keys requested in one iteration are
    parked and read in the next, the LDS image pair flips twice, and the run-ahead refill goes past the last tile."""
    n = (5 * gpu.cuda.get_device_properties(0).multi_processor_count + 3) * 32 + 7
    eng, idx, case = world((n, dim, nq))
    rng = np.random.default_rng(n + dim + nq)
    keys = rng.integers(0, 64, size=n)          # a row's group says nothing about its tile: keys parked for the wrong tile show
    keys[rng.random(n) < 0.05] = -1
    check(gpu, idx, case, case.live_tags, keys, 64, 10, 3, what="deep")
    check(gpu, idx, case, case.live_tags, keys, 64, 10, 3, allow=rng.random((nq, n)) < 0.3, what="deep, per-query bitmap")


def test_every_row_its_own_group_and_small_groups(gpu, world):
    eng, idx, case = world(SWEEP[2])
    n = case.n
    for k in (10, 300):
        want = check(gpu, idx, case, case.live_tags, np.arange(n), n, k, 4, what=f"own group k {k}")
        assert np.all(want[1][:, :, 1:] == -1) and np.all(np.isneginf(want[0][:, :, 1:])) and np.all(want[1][:, :, 0] >= 0)
        assert np.all(want[3] == n - len(case.dead))
        ks, ki = idx.search(case.q_raw, k)                   # one hit per group: the top-k, and so is the capped list
        assert np.array_equal(want[1][:, :, 0], ki) and np.array_equal(NF.bits(want[0][:, :, 0]), NF.bits(ks))
        assert np.array_equal(want[5], ki)
    # groups of 1, 2, 3, ... rows next to group_size 3 and 16: shorter lists, padded
    sizes = np.repeat(np.arange(60), np.arange(1, 61))[:n]
    keys = np.concatenate([sizes, np.full(n - len(sizes), -1)])
    for gs in (3, 16):
        want = check(gpu, idx, case, case.live_tags, keys, 60, 60, gs, what=f"small groups gs {gs}")
        filled = (want[1] >= 0).sum(axis=2)
        live = np.array([np.count_nonzero((keys == g) & (case.live_tags != -1)) for g in range(60)])
        listed = want[2] >= 0
        assert np.array_equal(filled[listed], np.minimum(live, gs)[want[2][listed]]) and not filled[~listed].any()


def test_ties_inside_a_group_and_across_groups(gpu, world):
    """Rows 2, 7, 40 and n - 1 hold one vector: score descending, then row ascending, within a chain and between groups."""
    eng, idx, case = world(SWEEP[0])
    n = case.n
    tags = case.tags.copy()                                  # an index of its own without tombstones: the tied rows all live
    ix = eng.open_index("ties")
    ix.add(case.xn, tags=tags, normalize=False)
    inside = np.arange(n) % 5
    inside[[2, 7, 40, n - 1]] = 3                            # all four in one group
    across = np.arange(n) % 5
    across[[2, 7, 40, n - 1]] = (4, 1, 1, 0)                 # three groups, two of the rows together
    for name, keys in (("inside", inside), ("across", across)):
        for gs in (1, 2, 3, 16):
            want = check(gpu, ix, case, tags, keys, 5, 5, gs, what=f"ties {name} gs {gs}")
            if name == "inside":
                assert want[2][0, 0] == 3 and want[1][0, 0, :min(gs, 4)].tolist() == [2, 7, 40, n - 1][:gs]
            else:
                assert want[2][0, :3].tolist() == [4, 1, 0] and want[1][0, :3, 0].tolist() == [2, 7, n - 1]
                assert gs == 1 or want[1][0, 1, 1] == 40
            tied = [2, 7, 40, n - 1]                         # the capped list: at most gs rows of a group, ties by row
            assert want[5][0, :4].tolist()[:min(gs, 4)] == tied[:min(gs, 4)] if name == "inside" else \
                want[5][0, :4].tolist() == ([2, 7, n - 1, int(want[5][0, 3])] if gs == 1 else tied)
    eng.drop_index("ties")


def test_tombstones_and_compaction(gpu, oracle):
    """A deleted best row: the runner-ups move up; a group whose rows are all deleted disappears; the same answer, in the new
    ordinals, after a compaction."""
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SWEEP[2])
    n = case.n
    keys = np.arange(n) % 11
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("tomb")
        idx.add(case.xn, tags=case.tags, normalize=False)
        tags = case.tags.copy()
        before = check(gpu, idx, case, tags, keys, 11, 11, 3, what="before")
        gone = [int(before[1][0, 0, 0]), int(before[1][0, 1, 1])] + np.flatnonzero(keys == 4).tolist()
        for r in gone:
            idx.delete(r)
        tags[gone] = -1
        after = check(gpu, idx, case, tags, keys, 11, 11, 3, what="after deletes")
        assert np.all(after[3] == 10) and not np.any(after[2] == 4) and before[1][0, 0, 1] in after[1][0]
        new_row = idx.compact()
        keep = np.flatnonzero(tags != -1)
        assert np.array_equal(new_row[keep], np.arange(len(keep)))
        small = Corpus.__new__(Corpus)
        small.scores, small.q_raw, small.nq, small.n = np.ascontiguousarray(case.scores[:, keep]), case.q_raw, case.nq, len(keep)
        packed = check(gpu, idx, small, tags[keep], keys[keep], 11, 11, 3, what="after compaction")
        assert np.array_equal(NF.bits(packed[0]), NF.bits(after[0])) and np.array_equal(packed[2], after[2])
        assert np.array_equal(packed[1], np.where(after[1] >= 0, new_row[np.maximum(after[1], 0)], -1))
    finally:
        eng.close()


def test_filters_and_bitmaps(gpu, world):
    eng, idx, case = world(SWEEP[15])                        # 1024 x 17
    n, nq = case.n, case.nq
    rng = np.random.default_rng(5)
    tags = case.live_tags
    keys = rng.integers(0, 37, size=n)
    keys[rng.random(n) < 0.1] = -1
    exact = np.where(np.arange(nq) % 3 == 2, -1, case.tags[np.arange(nq) % n]).astype(np.int32)
    by_dt = np.where(np.arange(nq) % 4 == 3, 9 << DSHIFT, ((np.arange(nq) % 3) + 1) << DSHIFT).astype(np.int32)
    by_p = (np.arange(nq) % 7 - 1).astype(np.int32)
    for what, f, m in (("exact", exact, None), ("doc type", by_dt, np.full(nq, DMASK, np.int32)), ("patient", by_p, np.full(nq, PMASK, np.int32))):
        for gs, k in ((3, 10), (16, 37)):
            check(gpu, idx, case, tags, keys, 37, k, gs, qfilter=f, qmask=m, what=f"filter {what} gs {gs}")
    per_q = rng.random((nq, n)) < 0.3
    for what, allow in (("per query", per_q), ("shared", per_q[0]), ("none", np.zeros(n, dtype=bool)), ("all", np.ones(n, dtype=bool))):
        want = check(gpu, idx, case, tags, keys, 37, 10, 3, allow=allow, what=f"bitmap {what}")
        assert what != "none" or not want[3].any()
        check(gpu, idx, case, tags, keys, 37, 37, 8, allow=allow, qfilter=by_p, qmask=np.full(nq, PMASK, np.int32),
              what=f"bitmap {what} with a filter")
    assert_same(check(gpu, idx, case, tags, keys, 37, 10, 3, allow=np.ones(n, dtype=bool), what="all set"),
                check(gpu, idx, case, tags, keys, 37, 10, 3, what="no bitmap"), "all set = no bitmap")


def test_bad_keys(gpu, world):
    """Keys of -1 (any negative key) are excluded; a key >= n_groups on a matching row raises the status word on the device
    variant and RASS_ERR_INVALID on the host variant — not on a tombstone, not on a row the filter keeps out."""
    import rassengine_amd._native as N
    eng, idx, case = world(SWEEP[2])
    n, nq = case.n, case.nq
    tags = case.live_tags
    live = np.flatnonzero(tags != -1)
    keys = np.arange(n) % 9
    keys[live[:4]] = (-1, -2, -(1 << 31), -(1 << 20))
    keys[case.dead[0]] = 1 << 30                             # on a tombstone: nothing happens
    want = check(gpu, idx, case, tags, keys, 9, 9, 4, what="negative keys and a tombstone's key")
    assert not np.isin(want[1], live[:4]).any()
    bad_row = int(live[10])
    keys[bad_row] = 9
    d_keys = dev(gpu, keys, np.int32)
    ref = H.expect_group_hits(case.scores, tags, keys, 9, 5, 3)
    assert ref[6] == 1
    got = run_device(gpu, idx, case.q_raw, 5, d_keys, 9, 3, True)
    assert got[-1] == 1
    assert_same(got[:-1], ref[:6], "key out of range: the rest of the answer is intact")
    with pytest.raises(N.RassError) as e:
        idx.search_group_hits(case.q_raw, 5, d_keys, 9, 3)
    assert e.value.code == INVALID and "n_groups" in str(e.value)
    other = np.full(nq, (int(tags[bad_row]) & PMASK) ^ 1, dtype=np.int32)
    check(gpu, idx, case, tags, keys, 9, 5, 3, qfilter=other, qmask=np.full(nq, PMASK, np.int32), what="filtered out")
    allow = np.ones(n, dtype=bool)
    allow[bad_row] = False
    check(gpu, idx, case, tags, keys, 9, 5, 3, allow=allow, what="not allowed")


def test_nonfinite_rows_and_queries(gpu, oracle):
    """tests/nonfinite_ref.py's rule: an index holding NaN / Inf rows answers, bit for bit, as its twin that holds a deleted
    finite row in the place of each (and as the restatement over the cleaned corpus); a poisoned query matches nothing."""
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SWEEP[2])
    n, nq = case.n, case.nq
    rng = np.random.default_rng(31)
    poison = {int(r): NF.KINDS[j % 3] for j, r in enumerate(rng.permutation(n)[:9])}
    keys = np.arange(n) % 6
    eng = Engine(0, case.dim)
    try:
        # every other row is stored as it is (normalize=False), so the oracle's score matrix holds for them; a poisoned row is
        # a tombstone in the reference, whatever it would score
        xa, xb, norm = NF.twin_vectors(rng, case.xn, poison)
        as_is = np.zeros(n, dtype=bool)
        as_is[sorted(poison)] = norm[sorted(poison)]
        A, B = NF.open_twin(eng, "nf", xa, xb, as_is, case.tags, poison)
        tags_ref = case.tags.copy()
        tags_ref[sorted(poison)] = -1
        d_keys = dev(gpu, keys, np.int32)
        clean = case
        for gs, k in ((3, 6), (16, 2)):
            want = check(gpu, B, clean, tags_ref, keys, 6, k, gs, what=f"twin B gs {gs}")
            got = A.search_group_hits(case.q_raw, k, d_keys, 6, gs, capped=True)
            assert_same(got, want, f"twin A gs {gs}")
            got = run_device(gpu, A, case.q_raw, k, d_keys, 6, gs, True)
            assert got[-1] == 0
            assert_same(got[:-1], want, f"twin A device gs {gs}")
            assert not np.isin(got[1], sorted(poison)).any()
        where = [1, 4, 9]
        qp = NF.poison_queries(case.q_raw, where)
        got = A.search_group_hits(qp, 6, d_keys, 6, 3, capped=True)
        NF.empty_rows(got, where, (float("-inf"), -1, -1, 0, float("-inf"), -1))
        ok = np.setdiff1d(np.arange(nq), where)
        want = H.expect_group_hits(clean.scores, tags_ref, keys, 6, 6, 3)
        assert_same(tuple(g[ok] for g in got), tuple(w[ok] for w in want[:6]), "the finite queries next to the poisoned ones")
        bad_keys = keys.copy()
        bad_keys[sorted(poison)] = 6                         # a poisoned row is no match: its key raises no status
        assert run_device(gpu, A, case.q_raw, 6, dev(gpu, bad_keys, np.int32), 6, 3, False)[-1] == 0
    finally:
        eng.close()


def test_caller_assigned_ids_and_id_base(gpu, oracle):
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SWEEP[0])
    n = case.n
    keys = np.arange(n) % 25
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], tags=case.tags[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], tags=case.tags[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(n - 300)]).astype(np.int64)
        want = check(gpu, idx, case, case.tags, keys, 25, 30, 4, ids=gids, what="global ids")
        assert want[5][0, :4].tolist() == [1002, 1007, 1040, 50_000 + n - 1 - 300]       # ties: by ROW, whatever the ids are
        d_keys = dev(gpu, keys, np.int32)
        assert_same(run_device(gpu, idx, case.q_raw, 30, d_keys, 25, 4, True, id_base=123)[:-1], want, "id_base ignored under an id map")
        plain = eng.open_index("plain")
        plain.add(case.xn, tags=case.tags, normalize=False)
        ref = H.expect_group_hits(case.scores, case.tags, keys, 25, 30, 4)
        got = run_device(gpu, plain, case.q_raw, 30, d_keys, 25, 4, True, id_base=7_000_000_000)
        shift = lambda i: np.where(i >= 0, i + 7_000_000_000, -1)
        assert_same(got[:-1], (ref[0], shift(ref[1]), ref[2], ref[3], ref[4], shift(ref[5])), "id_base")
    finally:
        eng.close()


def test_capped_list(gpu, world):
    """The capped list against its restatement over ALL groups, where the cap binds hard (few big groups) and where k * gs
    sits at the bound; with group_size >= the largest group it is search(k) (HIP against HIP)."""
    eng, idx, case = world(SWEEP[16])                        # 1024 x 33: two launch groups
    n = case.n
    rng = np.random.default_rng(77)
    skew = np.minimum(rng.geometric(0.3, size=n) - 1, 11)    # group 0 holds ~30 % of the rows
    for gs, k in ((1, 12), (2, 10), (3, 300), (8, 512), (16, 256)):
        check(gpu, idx, case, case.live_tags, skew, 12, k, gs, what=f"skewed gs {gs} k {k}")
    keys = np.arange(n) % 100                                # groups of 15 rows: a cap of 16 binds nothing
    for k in (1, 40, 256):
        want = check(gpu, idx, case, case.live_tags, keys, 100, k, 16, what=f"loose cap k {k}")
        ks, ki = idx.search(case.q_raw, k)
        assert np.array_equal(want[5], ki) and np.array_equal(NF.bits(want[4]), NF.bits(ks))


def test_refusals(gpu, world):
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    eng, idx, case = world(SWEEP[2])
    n, nq = case.n, case.nq
    L = idx._L
    d_keys = dev(gpu, np.zeros(n), np.int32)
    dq = dev(gpu, case.q_raw)
    cells = 4096 * 16
    os_, oi = gpu.empty((nq * cells,), dtype=gpu.float32, device="cuda"), gpu.empty((nq * cells,), dtype=gpu.int64, device="cuda")
    og, ot = gpu.empty((nq, 4096), dtype=gpu.int32, device="cuda"), gpu.empty((nq,), dtype=gpu.int64, device="cuda")
    cs, ci = gpu.empty((nq, 4096), dtype=gpu.float32, device="cuda"), gpu.empty((nq, 4096), dtype=gpu.int64, device="cuda")
    st = gpu.empty((1,), dtype=gpu.int32, device="cuda")
    bits = gpu.zeros((nq, (n + 31) // 32), dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def dcall(ix=idx, k=4, keys=d_keys, n_keys=n, n_groups=1, gs=3, allow=None, n_bitmaps=0, words=0, capped=True, cap_ids=True):
        return L.rass_index_search_group_hits_keys_device(ix._h, vp(dq), nq, k, vp(keys), n_keys, n_groups, gs, vp(allow), n_bitmaps,
                                                          words, None, None, 0, vp(os_), vp(oi), vp(og), vp(ot),
                                                          vp(cs) if capped else None, vp(ci) if capped and cap_ids else None, vp(st))

    assert dcall() == N.RASS_OK and dcall(capped=False) == N.RASS_OK
    assert dcall(allow=bits, n_bitmaps=nq, words=(n + 31) // 32) == N.RASS_OK and dcall(gs=16, k=256) == N.RASS_OK
    assert dcall(k=4096, gs=16, capped=False) == N.RASS_OK and dcall(n_groups=1 << 16, gs=16) == N.RASS_OK
    idx.engine.synchronize()
    for bad in (dict(gs=0), dict(gs=17), dict(gs=-1), dict(n_groups=(1 << 16) + 1, gs=16), dict(n_groups=1 << 20, gs=2),
                dict(n_groups=0), dict(n_groups=(1 << 20) + 1, gs=1), dict(k=0), dict(k=4097), dict(k=257, gs=16), dict(k=2048, gs=3),
                dict(n_keys=n - 1), dict(n_keys=-1), dict(keys=None), dict(cap_ids=False),
                dict(allow=bits, n_bitmaps=2, words=(n + 31) // 32), dict(allow=bits, n_bitmaps=nq, words=(n + 31) // 32 - 1)):
        assert dcall(**bad) == INVALID, bad
    with pytest.raises(N.RassError) as e:                    # the host variant draws the same lines
        L_host(idx, case, d_keys, n - 1)
    assert e.value.code == INVALID and "n_keys" in str(e.value)
    bf = eng.open_index("hits-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    assert dcall(ix=bf, n_keys=64) == UNSUPPORTED
    with pytest.raises(N.RassError) as e:
        bf.search_group_hits(case.q_raw, 4, dev(gpu, np.zeros(64), np.int32), 1, 3)
    assert e.value.code == UNSUPPORTED
    eng.drop_index(bf.name)
    wide_eng = Engine(0, 1100)
    try:
        wide = wide_eng.open_index("hits-wide")
        wq = np.random.default_rng(3).standard_normal((2, 1100), dtype=np.float32)
        wide.add(np.random.default_rng(4).standard_normal((40, 1100), dtype=np.float32))
        with pytest.raises(N.RassError) as e:
            wide.search_group_hits(wq, 4, dev(gpu, np.zeros(40), np.int32), 1, 3)
        assert e.value.code == UNSUPPORTED
    finally:
        wide_eng.close()


def L_host(idx, case, d_keys, n_keys):
    """The host entry point itself with ``n_keys`` as given (the Python wrapper would pad a short column)."""
    import rassengine_amd._native as N
    nq = case.nq
    out = [np.empty((nq, 4, 3), dtype=np.float32), np.empty((nq, 4, 3), dtype=np.int64), np.empty((nq, 4), dtype=np.int32),
           np.empty((nq,), dtype=np.int64)]
    q = np.ascontiguousarray(case.q_raw)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    N.check("rass_index_search_group_hits_keys",
            idx._L.rass_index_search_group_hits_keys(idx._h, p(q), nq, 4, ctypes.c_void_p(d_keys.data_ptr()), n_keys, 1, 3, None, 0, 0, None,
                                                     None, p(out[0]), p(out[1]), p(out[2]), p(out[3]), None, None))
