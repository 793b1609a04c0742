"""The terms aggregation with a top_hits sub-aggregation over a key column: ``rass_index_aggregate_hits_keys`` and its
``_device`` form — per bucket the hit count and the ``top_hits`` best hits, the buckets ordered by count or by their best hit.

The expected answer never comes from the engine: scores are the oracle's emulation of the scan's fmaf order
(``KIND_F32_MFMA``) for the queries as the GPU normalised them, counting, ranking and bucket order are
``tests/tophits_ref.py``.  Everything is compared bit for bit (scores as ``uint32``), for the host and the device variant, the
device outputs poisoned first.  The HIP-against-HIP tests (``top_hits = 1`` against ``rass_index_aggregate_keys``, the score
order at -inf against ``rass_index_search_group_hits_keys``, one bucket against ``search``) say so."""
import ctypes

import numpy as np
import pytest

import nonfinite_ref as NF
import tophits_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5          # RASS_ERR_INVALID, RASS_ERR_UNSUPPORTED
NEG_INF = R.NEG_INF
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
BOTH = (R.BY_COUNT, R.BY_SCORE)
N_ROWS = 1500                           # 46 tiles and a tail of 28 rows
# one dim per row-stride class (CH = 1 .. 8), 16 queries (NT = 1) and 17 (NT = 2): all 16 instantiations; two launch groups
SWEEP = [(N_ROWS, dim, nq) for dim in (100, 256, 384, 500, 640, 768, 872, 1024) for nq in (16, 17)] + [(N_ROWS, 1024, 33)]
EMPTY = (-1, 0, float("-inf"), -1, 0, 0)


class Corpus:
    """Rows, queries and tags of one shape with the oracle's score matrix, computed once and never changed by a test.  Rows 2,
    7, 40 and n - 1 are one vector: every query's scores tie there, and query 0's best rows ARE the tie."""

    def __init__(self, torch, oracle, n, dim, nq, seed=0):
        from rassengine_amd import ops
        rng = np.random.default_rng(9300 + n + dim + nq + seed)
        self.n, self.dim, self.nq = n, dim, nq
        x = rng.standard_normal((n, dim), dtype=np.float32)
        x[7] = x[40] = x[n - 1] = x[2]
        self.xn = oracle.normalize_ref(x).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0
        self.q_raw[0] = x[2] * 2.0
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.ranked = -np.sort(-self.scores, axis=1)
        self.tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 4, size=n) << DSHIFT)).astype(np.int32)
        self.dead = rng.permutation(n)[:max(1, n // 40)]
        self.dead = self.dead[~np.isin(self.dead, (2, 7, 40, n - 1))]      # the tied rows stay
        self.live_tags = self.tags.copy()
        self.live_tags[self.dead] = -1

    def mixed_thresholds(self):
        """One call, four kinds of threshold: -inf; the query's 200th best score; above every score (no hit); and, for query
        0, exactly its tied top score."""
        kind = np.arange(self.nq) % 4
        above = np.nextafter(self.ranked[:, 0], np.float32(np.inf))
        thr = np.where(kind == 1, self.ranked[:, min(200, self.n) - 1], np.where(kind == 2, above, NEG_INF)).astype(np.float32)
        thr[0] = self.ranked[0, 0]
        return thr


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
            idx = eng.open_index("tophits")
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


def device_outputs(torch, nq, size, th):
    """The seven outputs of the device variant, pre-filled with 7s."""
    shapes = [((nq, size), torch.int32), ((nq, size), torch.int64), ((nq, size, th), torch.float32), ((nq, size, th), torch.int64),
              ((nq,), torch.int64), ((nq,), torch.int64), ((1,), torch.int32)]
    return [torch.full(s, 7, dtype=t, device="cuda") for s, t in shapes]


def run_device(torch, idx, q_raw, thr, size, d_keys, n_groups, th, order, allow=None, qfilter=None, qmask=None, id_base=0):
    """The device variant (nq <= 32) on poisoned outputs -> (groups, counts, scores, ids, n_buckets, total_hits, status)."""
    nq = q_raw.shape[0]
    dq, df, dm = dev(torch, q_raw), dev(torch, qfilter, np.int32), dev(torch, qmask, np.int32)
    dt = dev(torch, np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,)).copy())
    da = words_of(torch, allow)
    n_bitmaps, words = (0, 0) if da is None else ((1 if da.dim() == 1 else da.shape[0]), da.shape[-1])
    out = device_outputs(torch, nq, size, th)
    torch.cuda.synchronize()
    idx.search_counts_hits_by_keys_device(dq.data_ptr(), nq, dt.data_ptr(), size, d_keys.data_ptr(), d_keys.shape[0], n_groups, th,
                                          *[o.data_ptr() for o in out], order_by=R.ORDER_NAMES[order], d_allow_ptr=ptr(da),
                                          n_bitmaps=n_bitmaps, words_per_bitmap=words, id_base=id_base, d_q_filter_ptr=ptr(df),
                                          d_q_filter_mask_ptr=ptr(dm))
    idx.engine.synchronize()
    return tuple(o.cpu().numpy() for o in out[:6]) + (int(out[6].item()),)


def assert_same(got, want, what):
    assert len(got) >= 6 and len(want) >= 6, what
    for g, w, name in zip(got[:6], want[:6], R.NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        gb, wb = NF.bits(g), NF.bits(w)
        assert np.array_equal(gb, wb), (what, name, np.argwhere(gb != wb)[:5].tolist(), g[gb != wb][:5], w[gb != wb][:5])


def cut(full, size, th):
    """The answer at (size, top_hits) out of the restatement at (SIZE >= size, TH >= top_hits): lists are prefixes both ways."""
    return (full[0][:, :size].copy(), full[1][:, :size].copy(), full[2][:, :size, :th].copy(), full[3][:, :size, :th].copy(), full[4],
            full[5])


def check(torch, idx, case, tags, keys, n_groups, size, th, thr, orders=BOTH, full=None, allow=None, qfilter=None, qmask=None, ids=None,
          n_keys=None, what=""):
    """Host variant (any nq) and device variant (launch groups of <= 32) under every order of ``orders`` against the numpy
    answer.  ``full``: {order: the restatement at a larger (size, top_hits)} to cut from.  ``n_keys`` > rows: the column the
    engine gets is that long, the surplus filled with keys that would raise the status word if they were read.  Returns
    {order: answer}."""
    col = np.asarray(keys, dtype=np.int64)
    if n_keys is not None:
        col = np.concatenate([col, np.full(n_keys - len(col), n_groups + 5)])
    d_keys = dev(torch, col, np.int32)
    thr_q = np.broadcast_to(np.asarray(thr, dtype=np.float32), (case.nq,))
    sl_of = lambda a, sl: None if a is None else a[sl]
    allow_q = lambda sl: None if allow is None else (allow if allow.ndim == 1 else allow[sl])
    out = {}
    for order in orders:
        if full is not None:
            want = cut(full[order], size, th)
        else:
            want = R.expect_top_hits(case.scores, tags, keys, n_groups, size, th, thr, order, allow, qfilter, qmask, ids)
            assert want[6] == 0
        tag = f"{what} order {R.ORDER_NAMES[order]} size {size} top_hits {th}"
        got = idx.search_counts_hits_by_keys(case.q_raw, thr_q, size, d_keys, n_groups, th, R.ORDER_NAMES[order], allow=words_of(torch, allow),
                                             q_filter=qfilter, q_filter_mask=qmask)
        assert_same(got, want, tag + " host")
        for q0 in range(0, case.nq, 32):
            sl = slice(q0, min(q0 + 32, case.nq))
            got = run_device(torch, idx, case.q_raw[sl], thr_q[sl], size, d_keys, n_groups, th, order, allow_q(sl), sl_of(qfilter, sl),
                             sl_of(qmask, sl))
            assert got[6] == 0
            assert_same(got, tuple(w[sl] for w in want[:6]), tag + " device")
        out[order] = want
    return out


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_stride_sweep(gpu, world, shape):
    eng, idx, case = world(shape)
    n, dim, nq = shape
    rng = np.random.default_rng(n + dim + nq)
    thr = case.mixed_thresholds()
    styles = {"7 random": (rng.integers(0, 7, size=n), 7), "300 random": (rng.integers(0, 300, size=n), 300),
              "7 runs": ((np.arange(n) // 32) % 7, 7), "300 runs": ((np.arange(n) // 32) % 300, 300)}
    assert case.scores[0, 2] == case.scores[0, 7] == case.scores[0, 40] == case.scores[0, n - 1] == case.ranked[0, 0] == thr[0]
    for name, (keys, n_groups) in styles.items():
        full = {order: R.expect_top_hits(case.scores, case.live_tags, keys, n_groups, 300, 16, thr, order) for order in BOTH}
        assert full[R.BY_COUNT][6] == 0
        hits = full[R.BY_COUNT][5]
        assert hits[0] == 4 and not hits[np.arange(nq) % 4 == 2].any() and np.all(hits[np.arange(nq) % 4 == 3] == n - len(case.dead))
        for th, size in ((1, 300), (2, 7), (3, 1), (3, 10), (8, 10), (16, 1), (16, 300)):
            check(gpu, idx, case, case.live_tags, keys, n_groups, size, th, thr, full=full, what=name)
        # top_hits = 1 under the count order IS the aggregation of the existing kernels, on every shared output (HIP against HIP)
        d_keys = dev(gpu, keys, np.int32)
        for size in (1, 10, 300):
            g, c, s, i, nb, tot = idx.search_counts_hits_by_keys(case.q_raw, thr, size, d_keys, n_groups, 1)
            assert_same((g, c, s[:, :, 0], i[:, :, 0], nb, tot), idx.search_counts_by_keys(case.q_raw, thr, size, d_keys, n_groups),
                        f"{name} top_hits 1 size {size}")
        # the score order at -inf IS the grouped search with inner hits (HIP against HIP); the counts are the groups' sizes
        live = np.bincount(keys[case.live_tags != -1], minlength=n_groups)
        for th, size in ((3, 10), (16, 300)):
            g, c, s, i, nb, tot = idx.search_counts_hits_by_keys(case.q_raw, NEG_INF, size, d_keys, n_groups, th, "max_score")
            hs, hi, hg, ht = idx.search_group_hits(case.q_raw, size, d_keys, n_groups, th)
            assert np.array_equal(NF.bits(s), NF.bits(hs)) and np.array_equal(i, hi) and np.array_equal(g, hg) and np.array_equal(nb, ht)
            assert np.array_equal(c, np.where(g >= 0, live[np.maximum(g, 0)], 0)) and np.all(tot == live.sum())


def test_full_grid_under_contention(gpu, oracle):
    """65 536 x 128, 32 queries: a workgroup on every CU.  8 buckets, then ONE bucket with top_hits 16 — every workgroup races
    on the 32 counters and the 32 chains: the counters are the number of live rows, the chain is search(k = 16) (HIP against
    HIP, next to the restatement)."""
    from rassengine_amd.engine import Engine
    n = 65536
    case = Corpus(gpu, oracle, n, 128, 32, seed=73)
    tags = case.live_tags
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("grid")
        idx.add(case.xn, tags=case.tags, normalize=False)
        for r in case.dead:
            idx.delete(int(r))
        n_live = n - len(case.dead)
        keys8 = np.random.default_rng(74).integers(0, 8, size=n)
        want = check(gpu, idx, case, tags, keys8, 8, 8, 16, NEG_INF, what="8 buckets")[R.BY_COUNT]
        assert np.all(want[1].sum(axis=1) == n_live) and np.all(want[5] == n_live) and np.all(want[4] == 8)
        want = check(gpu, idx, case, tags, np.zeros(n, dtype=np.int64), 1, 3, 16, NEG_INF, what="1 bucket")[R.BY_SCORE]
        ks, ki = idx.search(case.q_raw, 16)
        assert np.array_equal(want[3][:, 0, :], ki) and np.array_equal(NF.bits(want[2][:, 0, :]), NF.bits(ks))
        assert np.all(want[1][:, 0] == n_live) and np.all(want[0][:, 1:] == -1) and np.all(want[3][:, 1:] == -1)
        check(gpu, idx, case, tags, np.zeros(n, dtype=np.int64), 1, 1, 16, case.ranked[:, 999], what="1 bucket, 1 000 hits")
    finally:
        eng.close()


@pytest.mark.parametrize("nq", [16, 17])
def test_deep_loop_three_iterations_per_workgroup(gpu, world, nq):
    """5 * CUs + 3 tiles and a tail of 7 rows: the scan launches one workgroup per CU, so every workgroup runs the pair loop
    three times.  A tile's keys requested in one iteration are parked and read in the next, the LDS image pair flips twice, and
    the run-ahead refill goes past the last tile."""
    n = (5 * gpu.cuda.get_device_properties(0).multi_processor_count + 3) * 32 + 7
    eng, idx, case = world((n, 128, nq))
    rng = np.random.default_rng(n + nq)
    keys = rng.integers(0, 64, size=n)          # a row's group says nothing about its tile: keys parked for the wrong tile show
    keys[rng.random(n) < 0.05] = -1
    check(gpu, idx, case, case.live_tags, keys, 64, 10, 3, case.mixed_thresholds(), what="deep")
    check(gpu, idx, case, case.live_tags, keys, 64, 10, 3, NEG_INF, allow=rng.random((nq, n)) < 0.3, what="deep, per-query bitmap")


def test_small_buckets_count_ties_and_surplus_keys(gpu, world):
    eng, idx, case = world(SWEEP[2])
    n = case.n
    # buckets of 1, 2, 3, ... rows next to top_hits 3 and 16: shorter lists, padded; rows without a bucket (RASS_KEY_NONE)
    sizes = np.repeat(np.arange(50), np.arange(1, 51))[:n]
    keys = np.concatenate([sizes, np.full(n - len(sizes), -1)])
    live = np.array([np.count_nonzero((keys == g) & (case.live_tags != -1)) for g in range(50)])
    for th in (3, 16):
        for order, want in check(gpu, idx, case, case.live_tags, keys, 50, 50, th, NEG_INF, n_keys=n + 77, what="small buckets").items():
            listed = want[0] >= 0
            filled = (want[3] >= 0).sum(axis=2)
            assert np.array_equal(filled[listed], np.minimum(live, th)[want[0][listed]]) and not filled[~listed].any()
            assert np.array_equal(want[1][listed], live[want[0][listed]]) and np.all(want[5] == live.sum())
    # every bucket the same count: the key breaks the tie, whatever the scores say
    tags = case.tags.copy()
    ix = eng.open_index("ties")
    try:
        ix.add(case.xn, tags=tags, normalize=False)
        even = np.arange(n) % 12                                # 125 rows each
        want = check(gpu, ix, case, tags, even, 12, 5, 2, NEG_INF, orders=(R.BY_COUNT,), what="count ties")[R.BY_COUNT]
        assert np.all(want[0] == np.arange(5)) and np.all(want[1] == 125)
        # rows 2, 7, 40 and n - 1 hold one vector: score descending, then row ascending, within a chain and between buckets
        inside, across = even.copy(), even.copy()
        inside[[2, 7, 40, n - 1]] = 3
        across[[2, 7, 40, n - 1]] = (4, 1, 1, 0)
        for th in (1, 2, 3, 16):
            want = check(gpu, ix, case, tags, inside, 12, 5, th, case.mixed_thresholds(), what="ties inside")[R.BY_SCORE]
            assert want[0][0, 0] == 3 and want[1][0, 0] == 4 and want[3][0, 0, :min(th, 4)].tolist() == [2, 7, 40, n - 1][:th]
            want = check(gpu, ix, case, tags, across, 12, 5, th, case.mixed_thresholds(), what="ties across")
            assert want[R.BY_SCORE][0][0, :3].tolist() == [4, 1, 0] and want[R.BY_SCORE][3][0, :3, 0].tolist() == [2, 7, n - 1]
            assert want[R.BY_COUNT][0][0, :3].tolist() == [1, 0, 4] and want[R.BY_COUNT][1][0, :3].tolist() == [2, 1, 1]
    finally:
        eng.drop_index("ties")


def test_filters_and_bitmaps(gpu, world):
    eng, idx, case = world(SWEEP[15])                        # 1024 x 17
    n, nq = case.n, case.nq
    rng = np.random.default_rng(5)
    tags = case.live_tags
    thr = case.mixed_thresholds()
    keys = rng.integers(0, 37, size=n)
    keys[rng.random(n) < 0.1] = -1
    exact = np.where(np.arange(nq) % 3 == 2, -1, case.tags[np.arange(nq) % n]).astype(np.int32)
    by_dt = np.where(np.arange(nq) % 4 == 3, 9 << DSHIFT, ((np.arange(nq) % 3) + 1) << DSHIFT).astype(np.int32)
    by_p = (np.arange(nq) % 7 - 1).astype(np.int32)
    for what, f, m in (("exact", exact, None), ("doc type", by_dt, np.full(nq, DMASK, np.int32)), ("patient", by_p, np.full(nq, PMASK, np.int32))):
        for th, size in ((3, 10), (16, 37)):
            check(gpu, idx, case, tags, keys, 37, size, th, thr if th == 3 else NEG_INF, qfilter=f, qmask=m, what=f"filter {what}")
    per_q = rng.random((nq, n)) < 0.3
    for what, allow in (("per query", per_q), ("shared", per_q[0]), ("none", np.zeros(n, dtype=bool)), ("all", np.ones(n, dtype=bool))):
        want = check(gpu, idx, case, tags, keys, 37, 10, 3, NEG_INF, allow=allow, what=f"bitmap {what}")[R.BY_COUNT]
        assert what != "none" or not (want[4].any() or want[5].any())
        check(gpu, idx, case, tags, keys, 37, 37, 8, thr, allow=allow, qfilter=by_p, qmask=np.full(nq, PMASK, np.int32),
              what=f"bitmap {what} with a filter")
    assert_same(check(gpu, idx, case, tags, keys, 37, 10, 3, thr, allow=np.ones(n, dtype=bool), what="all set")[R.BY_SCORE],
                check(gpu, idx, case, tags, keys, 37, 10, 3, thr, what="no bitmap")[R.BY_SCORE], "all set = no bitmap")


def test_bad_keys(gpu, world):
    """Negative keys are in no bucket; a HIT with key >= n_groups raises the status word on the device variant and
    RASS_ERR_INVALID on the host variant — not on a tombstone, not on a row the filter keeps out, and not on a row below the
    threshold."""
    import rassengine_amd._native as N
    eng, idx, case = world(SWEEP[2])
    n, nq = case.n, case.nq
    tags = case.live_tags
    live = np.flatnonzero(tags != -1)
    keys = np.arange(n) % 9
    keys[live[:4]] = (-1, -2, -(1 << 31), -(1 << 20))
    keys[case.dead[0]] = 1 << 30                             # on a tombstone: nothing happens
    want = check(gpu, idx, case, tags, keys, 9, 9, 4, NEG_INF, what="negative keys and a tombstone's key")[R.BY_COUNT]
    assert not np.isin(want[3], live[:4]).any()
    bad_row = int(live[10])
    keys[bad_row] = 9
    d_keys = dev(gpu, keys, np.int32)
    for order in BOTH:
        ref = R.expect_top_hits(case.scores, tags, keys, 9, 5, 3, NEG_INF, order)
        assert ref[6] == 1
        got = run_device(gpu, idx, case.q_raw, NEG_INF, 5, d_keys, 9, 3, order)
        assert got[6] == 1
        assert_same(got, ref, "key out of range: the rest of the answer is intact")
        with pytest.raises(N.RassError) as e:
            idx.search_counts_hits_by_keys(case.q_raw, NEG_INF, 5, d_keys, 9, 3, R.ORDER_NAMES[order])
        assert e.value.code == INVALID and "n_groups" in str(e.value)
    below = np.nextafter(case.scores[:, bad_row], np.float32(np.inf))     # every query's threshold just above that row's score
    check(gpu, idx, case, tags, keys, 9, 5, 3, below, what="below the threshold")
    other = np.full(nq, (int(tags[bad_row]) & PMASK) ^ 1, dtype=np.int32)
    check(gpu, idx, case, tags, keys, 9, 5, 3, NEG_INF, qfilter=other, qmask=np.full(nq, PMASK, np.int32), what="filtered out")
    allow = np.ones(n, dtype=bool)
    allow[bad_row] = False
    check(gpu, idx, case, tags, keys, 9, 5, 3, NEG_INF, allow=allow, what="not allowed")


def test_nonfinite_rows_and_queries_and_thresholds(gpu, oracle):
    """tests/nonfinite_ref.py's rule: an index holding NaN / Inf rows answers, bit for bit, as its twin that holds a deleted
    finite row in the place of each (and as the restatement over the cleaned corpus); a poisoned query has no hit; a NaN
    threshold is refused by the host variant and matches nothing in the device variant."""
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SWEEP[2])
    n, nq = case.n, case.nq
    rng = np.random.default_rng(31)
    poison = {int(r): NF.KINDS[j % 3] for j, r in enumerate(rng.permutation(n)[:9])}
    keys = np.arange(n) % 6
    thr = case.mixed_thresholds()
    eng = Engine(0, case.dim)
    try:
        xa, xb, norm = NF.twin_vectors(rng, case.xn, poison)
        as_is = np.zeros(n, dtype=bool)
        as_is[sorted(poison)] = norm[sorted(poison)]
        A, B = NF.open_twin(eng, "nf", xa, xb, as_is, case.tags, poison)
        tags_ref = case.tags.copy()
        tags_ref[sorted(poison)] = -1
        d_keys = dev(gpu, keys, np.int32)
        for th, size, t in ((3, 6, thr), (16, 2, NEG_INF)):
            want = check(gpu, B, case, tags_ref, keys, 6, size, th, t, what=f"twin B top_hits {th}")
            for order in BOTH:
                got = A.search_counts_hits_by_keys(case.q_raw, t, size, d_keys, 6, th, R.ORDER_NAMES[order])
                assert_same(got, want[order], f"twin A top_hits {th}")
                got = run_device(gpu, A, case.q_raw, t, size, d_keys, 6, th, order)
                assert got[6] == 0
                assert_same(got, want[order], f"twin A device top_hits {th}")
                assert not np.isin(got[3], sorted(poison)).any()
        where = [1, 4, 9]
        qp = NF.poison_queries(case.q_raw, where)
        ok = np.setdiff1d(np.arange(nq), where)
        for order in BOTH:
            got = A.search_counts_hits_by_keys(qp, NEG_INF, 6, d_keys, 6, 3, R.ORDER_NAMES[order])
            NF.empty_rows(got, where, EMPTY)
            want = R.expect_top_hits(case.scores, tags_ref, keys, 6, 6, 3, NEG_INF, order)
            assert_same(tuple(g[ok] for g in got), tuple(w[ok] for w in want[:6]), "the finite queries next to the poisoned ones")
        bad_keys = keys.copy()
        bad_keys[sorted(poison)] = 6                         # a poisoned row is no hit: its key raises no status
        assert run_device(gpu, A, case.q_raw, NEG_INF, 6, dev(gpu, bad_keys, np.int32), 6, 3, R.BY_COUNT)[6] == 0
        # a NaN threshold
        nan_thr = thr.copy()
        nan_thr[[0, 5]] = np.nan
        ref_thr = np.where(np.isnan(nan_thr), np.float32(np.inf), nan_thr)       # +inf: nothing is >= it
        for order in BOTH:
            got = run_device(gpu, B, case.q_raw, nan_thr, 6, d_keys, 6, 3, order)
            assert got[6] == 0
            assert_same(got, R.expect_top_hits(case.scores, tags_ref, keys, 6, 6, 3, ref_thr, order), "NaN threshold, device")
            NF.empty_rows(got[:6], [0, 5], EMPTY)
        assert host_call(B, case.q_raw, nan_thr, d_keys, n, 6)[0] == INVALID
        assert host_call(B, case.q_raw, thr, d_keys, n, 6)[0] == N.RASS_OK
    finally:
        eng.close()


def test_caller_assigned_ids_id_base_and_an_empty_index(gpu, oracle):
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SWEEP[0])
    n, nq = case.n, case.nq
    keys = np.arange(n) % 25
    thr = case.mixed_thresholds()
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], tags=case.tags[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], tags=case.tags[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(n - 300)]).astype(np.int64)
        want = check(gpu, idx, case, case.tags, keys, 25, 30, 4, thr, ids=gids, what="global ids")
        assert want[R.BY_SCORE][3][0, :4, 0].tolist() == [1002, 1007, 1040, 50_000 + n - 1 - 300]   # ties: by ROW, whatever the ids are
        d_keys = dev(gpu, keys, np.int32)
        for order in BOTH:
            assert_same(run_device(gpu, idx, case.q_raw, thr, 30, d_keys, 25, 4, order, id_base=123), want[order], "id_base ignored under an id map")
        plain = eng.open_index("plain")
        plain.add(case.xn, tags=case.tags, normalize=False)
        for order in BOTH:
            ref = R.expect_top_hits(case.scores, case.tags, keys, 25, 30, 4, thr, order)
            got = run_device(gpu, plain, case.q_raw, thr, 30, d_keys, 25, 4, order, id_base=7_000_000_000)
            assert_same(got, ref[:3] + (np.where(ref[3] >= 0, ref[3] + 7_000_000_000, -1),) + ref[4:6], "id_base")
        empty = eng.open_index("empty")
        none = np.zeros((nq, 0), dtype=np.float32)
        for order in BOTH:
            want = R.expect_top_hits(none, np.zeros(0, np.int32), np.zeros(0, np.int64), 25, 4, 3, NEG_INF, order)
            got = empty.search_counts_hits_by_keys(case.q_raw, NEG_INF, 4, dev(gpu, np.zeros(8), np.int32), 25, 3, R.ORDER_NAMES[order])
            assert_same(got, want, "empty index, host")
            NF.empty_rows(got, np.arange(nq), EMPTY)
            got = run_device(gpu, empty, case.q_raw, NEG_INF, 4, dev(gpu, np.zeros(8), np.int32), 25, 3, order)
            assert got[6] == 0
            assert_same(got, want, "empty index, device")
    finally:
        eng.close()


def host_call(idx, q_raw, thr, d_keys, n_keys, n_groups, size=4, th=3, order=R.BY_COUNT):
    """The host entry point itself (the Python wrapper refuses bad arguments before it and pads a short column) on outputs
    pre-filled with 7s -> (rc, outputs)."""
    nq = q_raw.shape[0]
    out = [np.full((nq, size), 7, dtype=np.int32), np.full((nq, size), 7, dtype=np.int64), np.full((nq, size, th), 7, dtype=np.float32),
           np.full((nq, size, th), 7, dtype=np.int64), np.full((nq,), 7, dtype=np.int64), np.full((nq,), 7, dtype=np.int64)]
    q = np.ascontiguousarray(q_raw)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,)))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = idx._L.rass_index_aggregate_hits_keys(idx._h, p(q), nq, p(t), size, ctypes.c_void_p(d_keys.data_ptr()), n_keys, n_groups, th, order,
                                               None, 0, 0, None, None, *[p(o) for o in out])
    return rc, out


def test_refusals(gpu, world):
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    eng, idx, case = world(SWEEP[2])
    n, nq = case.n, case.nq
    L = idx._L
    d_keys = dev(gpu, np.zeros(n), np.int32)
    dq, dt = dev(gpu, case.q_raw), dev(gpu, np.full(nq, NEG_INF, dtype=np.float32))
    cells = 4096 * 16
    og, oc = gpu.full((nq, 4096), 7, dtype=gpu.int32, device="cuda"), gpu.full((nq, 4096), 7, dtype=gpu.int64, device="cuda")
    os_, oi = gpu.full((nq * cells,), 7, dtype=gpu.float32, device="cuda"), gpu.full((nq * cells,), 7, dtype=gpu.int64, device="cuda")
    nb, tot = gpu.full((nq,), 7, dtype=gpu.int64, device="cuda"), gpu.full((nq,), 7, dtype=gpu.int64, device="cuda")
    st = gpu.full((1,), 7, dtype=gpu.int32, device="cuda")
    bits = gpu.zeros((nq, (n + 31) // 32), dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def dcall(ix=idx, nq_=nq, size=4, keys=d_keys, n_keys=n, n_groups=1, th=3, order=R.BY_COUNT, allow=None, n_bitmaps=0, words=0,
              mask=None, groups=og):
        return L.rass_index_aggregate_hits_keys_device(ix._h, vp(dq), nq_, vp(dt), size, vp(keys), n_keys, n_groups, th, order, vp(allow),
                                                       n_bitmaps, words, None, vp(mask), 0, vp(groups), vp(oc), vp(os_), vp(oi), vp(nb),
                                                       vp(tot), vp(st))

    bad = (dict(th=0), dict(th=17), dict(th=-1), dict(n_groups=(1 << 16) + 1, th=16), dict(n_groups=1 << 20, th=2), dict(n_groups=0),
           dict(n_groups=(1 << 20) + 1, th=1), dict(size=0), dict(size=4097), dict(size=-3), dict(order=2), dict(order=-1),
           dict(n_keys=n - 1), dict(n_keys=-1), dict(keys=None), dict(groups=None), dict(nq_=0), dict(nq_=33), dict(mask=bits),
           dict(allow=bits, n_bitmaps=2, words=(n + 31) // 32), dict(allow=bits, n_bitmaps=nq, words=(n + 31) // 32 - 1))
    for kw in bad:                                           # refused with nothing launched: the poisoned outputs stay
        assert dcall(**kw) == INVALID, kw
    idx.engine.synchronize()
    for o in (og, oc, os_, oi, nb, tot, st):
        assert bool((o == 7).all())
    assert dcall() == N.RASS_OK and dcall(order=R.BY_SCORE) == N.RASS_OK
    assert dcall(allow=bits, n_bitmaps=nq, words=(n + 31) // 32) == N.RASS_OK and dcall(th=16, size=256) == N.RASS_OK
    assert dcall(size=4096, th=16) == N.RASS_OK and dcall(n_groups=1 << 16, th=16, order=R.BY_SCORE) == N.RASS_OK
    idx.engine.synchronize()
    assert int(st.item()) == 0
    # the host variant draws the same lines and leaves its outputs alone
    for kw in (dict(n_keys=n - 1), dict(th=17), dict(size=4097), dict(order=2), dict(n_groups=1 << 20, th=2)):
        a = dict(dict(n_keys=n, n_groups=1, size=4, th=3, order=R.BY_COUNT), **kw)
        sz, th = min(a["size"], 8), min(a["th"], 4)          # the arrays only have to exist: a refused call writes nothing
        out = [np.full((nq, sz), 7, dtype=np.int32), np.full((nq, sz), 7, dtype=np.int64), np.full((nq, sz, th), 7, dtype=np.float32),
               np.full((nq, sz, th), 7, dtype=np.int64), np.full((nq,), 7, dtype=np.int64), np.full((nq,), 7, dtype=np.int64)]
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        q, t = np.ascontiguousarray(case.q_raw), np.full(nq, NEG_INF, dtype=np.float32)
        rc = L.rass_index_aggregate_hits_keys(idx._h, p(q), nq, p(t), a["size"], vp(d_keys), a["n_keys"], a["n_groups"], a["th"], a["order"],
                                              None, 0, 0, None, None, *[p(o) for o in out])
        assert rc == INVALID and all(np.all(o == 7) for o in out), kw
    bf = eng.open_index("tophits-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    assert dcall(ix=bf, n_keys=64) == UNSUPPORTED
    with pytest.raises(N.RassError) as e:
        bf.search_counts_hits_by_keys(case.q_raw, NEG_INF, 4, dev(gpu, np.zeros(64), np.int32), 1, 3)
    assert e.value.code == UNSUPPORTED
    eng.drop_index(bf.name)
    wide_eng = Engine(0, 1100)
    try:
        wide = wide_eng.open_index("tophits-wide")
        wq = np.random.default_rng(3).standard_normal((2, 1100), dtype=np.float32)
        wide.add(np.random.default_rng(4).standard_normal((40, 1100), dtype=np.float32))
        with pytest.raises(N.RassError) as e:
            wide.search_counts_hits_by_keys(wq, NEG_INF, 4, dev(gpu, np.zeros(40), np.int32), 1, 3)
        assert e.value.code == UNSUPPORTED
    finally:
        wide_eng.close()


def test_shim_top_hits(gpu, oracle, monkeypatch):
    """``HipIndexer.semantic_aggregate(top_hits=3)`` over a real index of ~300 docs, by ``patientId`` (keys from the tag), by an
    attribute field, with ``where=`` and under ``order="max_score"``, against a host loop over the stored docs."""
    from rassengine_amd import config, indexer
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    from test_gpu_group_by_attr import DIM, Host, _docs
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,code:int,chunkDate:date")
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "cosine")
    eng = Engine(0, DIM)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: eng.open_index(name))
    try:
        rng = np.random.default_rng(37)
        name, n = "rass-idx-tophits", 300
        docs = _docs(rng, n)
        emb = rng.standard_normal((n, DIM), dtype=np.float32)
        indexer.add_documents(name, docs, emb)
        st = REGISTRY.get(name)
        with st.lock:                                                                                 # deleted outright
            for i in range(100, 110):
                r = st.doc_row.pop(f"d{i}")
                st.index.delete(r)
                st.row_doc[r] = None
        hip = indexer.HipIndexer(None, name)
        q = rng.standard_normal(DIM).astype(np.float32)
        host = Host(gpu, oracle, st, q)
        thr = host.live[119][0]                                                   # the 120 best chunks are the hits
        patients, types = st.patients.names(), st.attrs.dicts["resourceType"].names()

        def want(key_of, rank_of, keep=lambda d: True, by_score=False, size=5):
            per = {}
            for s, r, d in host.live:                    # score desc, row asc: a key's docs come best first
                if s >= thr and keep(d):
                    per.setdefault(key_of(d), []).append((d["doc_id"], s))
            order = sorted(per, key=(lambda k: (-per[k][0][1], rank_of(k))) if by_score else (lambda k: (-len(per[k]), rank_of(k))))
            return [(k, len(per[k]), per[k][:3]) for k in order[:size]], len(per), sum(len(v) for v in per.values())

        def listed(agg):
            assert all(b["top_hit"] == b["top_hits"][0] for b in agg["buckets"])
            return [(b["key"], b["doc_count"], [(d["doc_id"], s) for d, s in b["top_hits"]]) for b in agg["buckets"]], agg["cardinality"], agg["total"]

        kw_rank = lambda k: 0 if k is None else 1 + types.index(k)
        assert listed(hip.semantic_aggregate(q, thr, by="patientId", top_hits=3)) == want(lambda d: d["patientId"], patients.index)
        assert listed(hip.semantic_aggregate(q, thr, by="resourceType", top_hits=3)) == want(lambda d: d.get("resourceType"), kw_rank)
        got = hip.semantic_aggregate(q, thr, by="resourceType", top_hits=3, order="max_score", size=2)
        assert listed(got) == want(lambda d: d.get("resourceType"), kw_rank, by_score=True, size=2)
        assert got["sum_other_doc_count"] == 120 - sum(b["doc_count"] for b in got["buckets"])
        where = {"range": {"chunkDate": {"gte": "2024-01-01", "lt": "2024-03-01"}}}
        inside = lambda d: "2024-01-01" <= d.get("chunkDate", "") < "2024-03-01"
        got = listed(hip.semantic_aggregate(q, thr, by="patientId", top_hits=3, where=where))
        assert got == want(lambda d: d["patientId"], patients.index, keep=inside) and 0 < got[2] < 120
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()
