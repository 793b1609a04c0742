"""The grouped search and the aggregation over a key column, optionally within a bitmap: ``rass_index_search_grouped_keys``,
``rass_index_aggregate_keys`` and their ``_device`` forms.

The expected answer never comes from the engine: scores are the oracle's emulation of the scan's fmaf order
(``KIND_F32_MFMA``) for the queries as the GPU normalised them, grouping and counting are ``tests/groupkeys_ref.py``.
Everything is compared with ``array_equal``; the one HIP-against-HIP test (the tag-keyed calls over the same groups) says so."""
import ctypes

import numpy as np
import pytest

import groupkeys_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5          # RASS_ERR_INVALID, RASS_ERR_UNSUPPORTED

NEG_INF = R.NEG_INF
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
GNAMES = ("scores", "ids", "groups", "totals")
CNAMES = ("groups", "counts", "scores", "ids", "n_buckets", "total_hits")
# n, dim, nq: one launch group; a full half-batch; two host groups; wide rows in two launches; the widest panel; a partial tile
SHAPES = [(1000, 100, 1), (3000, 256, 16), (2500, 1024, 33), (2000, 1536, 17), (2000, 2048, 16), (33, 128, 2)]


class Corpus:
    """Rows, queries and tags of one shape with the oracle's score matrix, computed once and never changed by a test.  Rows 2,
    7 and n - 1 are one vector: every query's scores tie there, at whatever rank that vector lands."""

    def __init__(self, torch, oracle, n, dim, nq):
        from rassengine_amd import ops
        rng = np.random.default_rng(7000 + n + dim + nq)
        self.n, self.dim, self.nq = n, dim, nq
        x = rng.standard_normal((n, dim), dtype=np.float32)
        x[7] = x[2]
        x[n - 1] = x[2]
        self.xn = oracle.normalize_ref(x).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0
        self.q_raw[0] = x[2] * 2.0                                   # query 0's best rows ARE the tie
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.ranked = -np.sort(-self.scores, axis=1)
        self.tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 4, size=n) << DSHIFT)).astype(np.int32)
        self.dead = rng.permutation(n)[:max(1, n // 40)]
        self.live_tags = self.tags.copy()
        self.live_tags[self.dead] = -1

    def at_rank(self, r):
        return self.ranked[:, min(r, self.n) - 1].copy()


_CORPORA = {}


@pytest.fixture(scope="module")
def world(gpu, oracle):
    """shape -> (engine, index with tombstones, corpus); built on first use, shared by the tests of this file."""
    from rassengine_amd.engine import Engine
    made = {}

    def get(shape):
        if shape not in made:
            n, dim, nq = shape
            case = _CORPORA.setdefault(shape, Corpus(gpu, oracle, n, dim, nq))
            eng = Engine(0, dim)
            idx = eng.open_index("by-keys")
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


def bitmap_args(torch, allow):
    """bool [n] / [nq, n] / None -> (device words or None, n_bitmaps, words)."""
    if allow is None:
        return None, 0, 0
    w = dev(torch, R.pack_bits(allow).view(np.int32))
    return w, (1 if w.dim() == 1 else w.shape[0]), w.shape[-1]


def run_grouped_device(torch, idx, q_raw, k, d_keys, n_groups, allow=None, qfilter=None, qmask=None, id_base=0):
    nq = q_raw.shape[0]
    dq, df, dm = dev(torch, q_raw), dev(torch, qfilter, np.int32), dev(torch, qmask, np.int32)
    da, n_bitmaps, words = bitmap_args(torch, allow)
    os_ = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    og = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    ot = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_grouped_by_keys_device(dq.data_ptr(), nq, k, d_keys.data_ptr(), d_keys.shape[0], n_groups, os_.data_ptr(),
                                      oi.data_ptr(), og.data_ptr(), ot.data_ptr(), st.data_ptr(), d_allow_ptr=ptr(da),
                                      n_bitmaps=n_bitmaps, words_per_bitmap=words, id_base=id_base, d_q_filter_ptr=ptr(df),
                                      d_q_filter_mask_ptr=ptr(dm))
    idx.engine.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy(), og.cpu().numpy(), ot.cpu().numpy(), int(st.item())


def run_counts_device(torch, idx, q_raw, thr, size, d_keys, n_groups, allow=None, qfilter=None, qmask=None, id_base=0):
    nq = q_raw.shape[0]
    dq, df, dm = dev(torch, q_raw), dev(torch, qfilter, np.int32), dev(torch, qmask, np.int32)
    dt = dev(torch, np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,)).copy())
    da, n_bitmaps, words = bitmap_args(torch, allow)
    og = torch.full((nq, size), 7, dtype=torch.int32, device="cuda")
    oc = torch.full((nq, size), 7, dtype=torch.int64, device="cuda")
    os_ = torch.full((nq, size), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, size), 7, dtype=torch.int64, device="cuda")
    ob = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    ot = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_counts_by_keys_device(dq.data_ptr(), nq, dt.data_ptr(), size, d_keys.data_ptr(), d_keys.shape[0], n_groups,
                                     og.data_ptr(), oc.data_ptr(), os_.data_ptr(), oi.data_ptr(), ob.data_ptr(), ot.data_ptr(),
                                     st.data_ptr(), d_allow_ptr=ptr(da), n_bitmaps=n_bitmaps, words_per_bitmap=words,
                                     id_base=id_base, d_q_filter_ptr=ptr(df), d_q_filter_mask_ptr=ptr(dm))
    idx.engine.synchronize()
    return (og.cpu().numpy(), oc.cpu().numpy(), os_.cpu().numpy(), oi.cpu().numpy(), ob.cpu().numpy(), ot.cpu().numpy(),
            int(st.item()))


def assert_same(got, want, names, what):
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check(torch, idx, case, tags, keys, n_groups, k, thr, allow=None, qfilter=None, qmask=None, ids=None, what=""):
    """Both searches, host variant (any nq) and device variant (groups of <= 32), against the numpy answer."""
    d_keys = dev(torch, keys, np.int32)
    sl_of = lambda a, sl: None if a is None else a[sl]
    allow_q = lambda sl: None if allow is None else (allow if allow.ndim == 1 else allow[sl])
    want_g = R.expect_grouped(case.scores, tags, keys, n_groups, k, allow, qfilter, qmask, ids)
    want_c = R.expect_counts(case.scores, tags, keys, n_groups, k, thr, allow, qfilter, qmask, ids)
    assert want_g[4] == 0 and want_c[6] == 0
    words = None if allow is None else dev(torch, R.pack_bits(allow).view(np.int32))
    got = idx.search_grouped_by_keys(case.q_raw, k, d_keys, n_groups, allow=words, q_filter=qfilter, q_filter_mask=qmask)
    assert_same(got, want_g, GNAMES, what + " grouped host")
    got = idx.search_counts_by_keys(case.q_raw, thr, k, d_keys, n_groups, allow=words, q_filter=qfilter, q_filter_mask=qmask)
    assert_same(got, want_c, CNAMES, what + " counts host")
    thr_q = np.broadcast_to(np.asarray(thr, dtype=np.float32), (case.nq,))
    for q0 in range(0, case.nq, 32):
        sl = slice(q0, min(q0 + 32, case.nq))
        got = run_grouped_device(torch, idx, case.q_raw[sl], k, d_keys, n_groups, allow_q(sl), sl_of(qfilter, sl), sl_of(qmask, sl))
        assert got[4] == 0
        assert_same(got, tuple(w[sl] for w in want_g[:4]), GNAMES, what + " grouped device")
        got = run_counts_device(torch, idx, case.q_raw[sl], thr_q[sl], k, d_keys, n_groups, allow_q(sl), sl_of(qfilter, sl),
                                sl_of(qmask, sl))
        assert got[6] == 0
        assert_same(got, tuple(w[sl] for w in want_c[:6]), CNAMES, what + " counts device")
    return want_g, want_c


def key_styles(rng, n):
    """name -> (keys, n_groups): random keys; runs of 32 equal keys (the one-add-per-half path); ~10 % without a group; one
    group."""
    holes = rng.integers(0, 37, size=n)
    holes[rng.random(n) < 0.1] = -1
    holes[rng.random(n) < 0.02] = -(1 << 31)                         # any negative key is "no group"
    one = np.zeros(n, dtype=np.int64)
    one[rng.random(n) < 0.1] = -1
    return {"random": (rng.integers(0, 37, size=n), 37), "runs": ((np.arange(n) // 32) % 5, 5), "holes": (holes, 37),
            "one group": (one, 1)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_keys_match_oracle(gpu, world, shape):
    eng, idx, case = world(shape)
    n, dim, nq = shape
    rng = np.random.default_rng(n + dim)
    tags = case.live_tags
    thresholds = {"rank 1": case.at_rank(1), "rank 50": case.at_rank(50), "-inf": np.full(nq, NEG_INF)}
    assert case.scores[0, 2] == case.scores[0, 7] == case.scores[0, n - 1] == case.ranked[0, 0]    # the tie sits AT rank 1
    styles = key_styles(rng, n)
    for name, (keys, n_groups) in styles.items():
        for tname, thr in thresholds.items():
            for k in (1, 10, 4096):
                check(gpu, idx, case, tags, keys, n_groups, k, thr, what=f"{name} {tname} k {k}")
    keys, n_groups = styles["holes"]
    thr = case.at_rank(50)
    # the tag still filters: exact (whole tag) and masked (doc type; patient), -1 = no filter, and a value no row carries
    exact = np.where(np.arange(nq) % 3 == 2, -1, case.tags[np.arange(nq) % n]).astype(np.int32)
    by_dt = np.where(np.arange(nq) % 4 == 3, 9 << DSHIFT, ((np.arange(nq) % 3) + 1) << DSHIFT).astype(np.int32)
    by_p = (np.arange(nq) % 7 - 1).astype(np.int32)
    for what, f, m in (("exact", exact, None), ("doc type", by_dt, np.full(nq, DMASK, np.int32)), ("patient", by_p, np.full(nq, PMASK, np.int32))):
        for k in (1, 10):
            check(gpu, idx, case, tags, keys, n_groups, k, thr, qfilter=f, qmask=m, what=f"filter {what} k {k}")
            check(gpu, idx, case, tags, keys, n_groups, k, NEG_INF, qfilter=f, qmask=m, what=f"filter {what} -inf k {k}")
    if dim > 1024:
        return
    # a bitmap: one per query, one shared; random bits, none, all (bits of tombstones and rows without a group change nothing)
    per_q = rng.random((nq, n)) < 0.3
    for what, allow in (("per query", per_q), ("shared", per_q[0]), ("none", np.zeros(n, dtype=bool)), ("all", np.ones(n, dtype=bool)),
                        ("none per query", np.zeros((nq, n), dtype=bool))):
        for tname, thr in thresholds.items():
            want_g, want_c = check(gpu, idx, case, tags, keys, n_groups, 10, thr, allow=allow, what=f"bitmap {what} {tname}")
            if what.startswith("none"):
                assert not want_g[3].any() and not want_c[5].any()
        check(gpu, idx, case, tags, keys, n_groups, 4096, NEG_INF, allow=allow, qfilter=by_p, qmask=np.full(nq, PMASK, np.int32),
              what=f"bitmap {what} with a filter")
    all_set = R.expect_counts(case.scores, tags, keys, n_groups, 10, NEG_INF, np.ones(n, dtype=bool))
    assert_same(all_set[:6], R.expect_counts(case.scores, tags, keys, n_groups, 10, NEG_INF)[:6], CNAMES, "all set = no bitmap")


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_tag_keys_equal_the_tag_keyed_calls(gpu, world, shape):
    """HIP against HIP: keys computed on the host as (tag & mask) >> shift, no bitmap -> every output of
    rass_index_search_grouped / rass_index_aggregate on the same index."""
    eng, idx, case = world(shape)
    for mask, shift, n_groups in ((PMASK, 0, 6), (DMASK, DSHIFT, 4)):
        keys = dev(gpu, (case.tags.astype(np.int64) & mask) >> shift, np.int32)
        built = idx.group_keys_from_tag(mask)                  # the same groups by the device builder (tombstones: no group)
        assert_same(idx.search_grouped_by_keys(case.q_raw, 10, built, n_groups), idx.search_grouped(case.q_raw, 10, mask, n_groups),
                    GNAMES, f"grouped mask {mask:#x}, keys from the tag")
        for k in (1, 10, 4096):
            assert_same(idx.search_grouped_by_keys(case.q_raw, k, keys, n_groups), idx.search_grouped(case.q_raw, k, mask, n_groups),
                        GNAMES, f"grouped mask {mask:#x} k {k}")
            for thr in (case.at_rank(1), case.at_rank(50), NEG_INF):
                assert_same(idx.search_counts_by_keys(case.q_raw, thr, k, keys, n_groups),
                            idx.search_counts(case.q_raw, thr, k, mask, n_groups), CNAMES, f"counts mask {mask:#x} k {k}")


def test_sparse_keys_at_the_group_bound(gpu, world):
    eng, idx, case = world(SHAPES[0])
    n = case.n
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 1 << 20, size=n)
    keys[:3] = ((1 << 20) - 1, 0, (1 << 20) - 1)
    for k in (1, 10, 4096):
        check(gpu, idx, case, case.live_tags, keys, 1 << 20, k, case.at_rank(50), what=f"2^20 groups k {k}")
        check(gpu, idx, case, case.live_tags, keys, 1 << 20, k, NEG_INF, what=f"2^20 groups -inf k {k}")


def test_status_word(gpu, world):
    """A key >= n_groups raises the status word on a matching row / a hit only: not below the threshold, not on a tombstone,
    not on a row the filter or the bitmap keeps out, and never for a negative key."""
    import rassengine_amd._native as N
    eng, idx, case = world(SHAPES[1])
    n, nq = case.n, case.nq
    tags = case.live_tags
    live = np.flatnonzero(tags != -1)
    bad_row = int(live[np.argmax(case.scores[0, live] < case.ranked[0, 99])])     # a live row outside query 0's best 100
    keys = np.arange(n) % 9
    keys[bad_row] = 9
    d_keys = dev(gpu, keys, np.int32)
    want = R.expect_grouped(case.scores, tags, keys, 9, 5)
    assert want[4] == 1
    got = run_grouped_device(gpu, idx, case.q_raw, 5, d_keys, 9)
    assert got[4] == 1
    assert_same(got[:4], want[:4], GNAMES, "grouped, key out of range")
    want = R.expect_counts(case.scores, tags, keys, 9, 5, NEG_INF)
    got = run_counts_device(gpu, idx, case.q_raw, NEG_INF, 5, d_keys, 9)
    assert want[6] == 1 and got[6] == 1
    assert_same(got[:6], want[:6], CNAMES, "counts, key out of range")
    for call in (lambda: idx.search_grouped_by_keys(case.q_raw, 5, d_keys, 9), lambda: idx.search_counts_by_keys(case.q_raw, NEG_INF, 5, d_keys, 9)):
        with pytest.raises(N.RassError) as e:
            call()
        assert e.value.code == -1 and "n_groups" in str(e.value)
    # below every query's threshold the row is no hit: the aggregation answers (the grouped search has no threshold)
    thr = np.nextafter(case.scores[:, bad_row], np.float32(np.inf))
    want = R.expect_counts(case.scores, tags, keys, 9, 5, thr)
    assert want[6] == 0
    assert_same(idx.search_counts_by_keys(case.q_raw, thr, 5, d_keys, 9), want[:6], CNAMES, "below the threshold")
    assert run_counts_device(gpu, idx, case.q_raw, thr, 5, d_keys, 9)[6] == 0
    # filtered out by the tag, and by the bitmap
    other = np.full(nq, (int(tags[bad_row]) & PMASK) ^ 1, dtype=np.int32)
    check(gpu, idx, case, tags, keys, 9, 5, NEG_INF, qfilter=other, qmask=np.full(nq, PMASK, np.int32), what="filtered out")
    allow = np.ones(n, dtype=bool)
    allow[bad_row] = False
    check(gpu, idx, case, tags, keys, 9, 5, NEG_INF, allow=allow, what="not allowed")
    # on a tombstoned row, and a negative key of any size
    keys2 = np.arange(n) % 9
    keys2[case.dead[0]] = 1 << 30
    keys2[live[:4]] = (-1, -2, -(1 << 31), -(1 << 20))
    check(gpu, idx, case, tags, keys2, 9, 5, NEG_INF, what="tombstone and negative keys")


def test_keys_shorter_than_the_index(gpu, oracle):
    """Rows appended after the column was built: the device call refuses the short column, the Python wrapper pads it with
    'no group' (and a short bitmap with zero words)."""
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    case = _CORPORA.setdefault(SHAPES[1], Corpus(gpu, oracle, *SHAPES[1]))
    n, first = case.n, 2000
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("short")
        idx.add(case.xn[:first], tags=case.tags[:first], normalize=False)
        idx.set_attr(0, 0, np.arange(first) % 11)
        built = idx.group_keys_from_attr(0)[:first].contiguous()          # exactly the rows there were
        bits = gpu.full(((first + 31) // 32,), -1, dtype=gpu.int32, device="cuda")
        idx.add(case.xn[first:], tags=case.tags[first:], normalize=False)
        keys = np.concatenate([np.arange(first) % 11, np.full(n - first, -1)])
        allow = np.concatenate([np.ones((first + 31) // 32 * 32, dtype=bool), np.zeros(n, dtype=bool)])[:n]
        for a_dev, a_ref in ((None, None), (bits, allow)):
            want = R.expect_grouped(case.scores, case.tags, keys, 11, 20, a_ref)
            assert_same(idx.search_grouped_by_keys(case.q_raw, 20, built, 11, allow=a_dev), want, GNAMES, "padded grouped")
            want = R.expect_counts(case.scores, case.tags, keys, 11, 20, case.at_rank(500), a_ref)
            assert_same(idx.search_counts_by_keys(case.q_raw, case.at_rank(500), 20, built, 11, allow=a_dev), want, CNAMES, "padded counts")
        with pytest.raises(N.RassError) as e:
            run_grouped_device(gpu, idx, case.q_raw, 20, built, 11)
        assert e.value.code == -1 and "n_keys" in str(e.value)
        with pytest.raises(N.RassError) as e:
            run_counts_device(gpu, idx, case.q_raw, NEG_INF, 20, built, 11)
        assert e.value.code == -1 and "n_keys" in str(e.value)
        # ... and the column built now covers them: the appended rows have no value, so they join the missing key
        full = idx.group_keys_from_attr(0, missing=11)
        keys = np.concatenate([np.arange(first) % 11, np.full(n - first, 11)])
        assert_same(idx.search_grouped_by_keys(case.q_raw, 20, full, 12), R.expect_grouped(case.scores, case.tags, keys, 12, 20),
                    GNAMES, "missing key")
    finally:
        eng.close()


def test_caller_assigned_ids_and_id_base(gpu, oracle):
    from rassengine_amd.engine import Engine
    case = _CORPORA.setdefault(SHAPES[0], Corpus(gpu, oracle, *SHAPES[0]))
    n = case.n
    keys = np.arange(n) % 25
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], tags=case.tags[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], tags=case.tags[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(n - 300)]).astype(np.int64)
        want_g, want_c = check(gpu, idx, case, case.tags, keys, 25, 30, case.at_rank(400), ids=gids, what="global ids")
        d_keys = dev(gpu, keys, np.int32)
        assert_same(run_grouped_device(gpu, idx, case.q_raw, 30, d_keys, 25, id_base=123)[:4], want_g[:4], GNAMES, "id_base ignored")
        plain = eng.open_index("plain")
        plain.add(case.xn, tags=case.tags, normalize=False)
        es, ei, eg, et, _ = R.expect_grouped(case.scores, case.tags, keys, 25, 30)
        got = run_grouped_device(gpu, plain, case.q_raw, 30, d_keys, 25, id_base=7_000_000_000)
        assert_same(got[:4], (es, np.where(ei >= 0, ei + 7_000_000_000, -1), eg, et), GNAMES, "id_base")
        eg, ec, es, ei, eb, et, _ = R.expect_counts(case.scores, case.tags, keys, 25, 30, NEG_INF)
        got = run_counts_device(gpu, plain, case.q_raw, NEG_INF, 30, d_keys, 25, id_base=7_000_000_000)
        assert_same(got[:6], (eg, ec, es, np.where(ei >= 0, ei + 7_000_000_000, -1), eb, et), CNAMES, "id_base")
    finally:
        eng.close()


def test_refusals(gpu, world):
    import rassengine_amd._native as N
    eng, idx, case = world(SHAPES[1])
    weng, widx, wcase = world(SHAPES[3])
    n, nq = case.n, case.nq
    d_keys = dev(gpu, np.zeros(n), np.int32)
    # a bitmap on wide rows: UNSUPPORTED, host and device variants, before anything runs
    wkeys = dev(gpu, np.zeros(wcase.n), np.int32)
    wbits = gpu.full(((wcase.n + 31) // 32,), -1, dtype=gpu.int32, device="cuda")
    for call in (lambda: widx.search_grouped_by_keys(wcase.q_raw, 5, wkeys, 1, allow=wbits),
                 lambda: widx.search_counts_by_keys(wcase.q_raw, NEG_INF, 5, wkeys, 1, allow=wbits),
                 lambda: run_grouped_device(gpu, widx, wcase.q_raw[:16], 5, wkeys, 1, allow=np.ones(wcase.n, dtype=bool)),
                 lambda: run_counts_device(gpu, widx, wcase.q_raw[:16], NEG_INF, 5, wkeys, 1, allow=np.ones(wcase.n, dtype=bool))):
        with pytest.raises(N.RassError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    # the bitmap's shape: n_bitmaps neither 1 nor nq, too few words
    L = idx._L
    dq = dev(gpu, case.q_raw)
    out = [gpu.empty((nq, 4), dtype=t, device="cuda") for t in (gpu.float32, gpu.int64, gpu.int32)]
    tot, st = gpu.empty((nq,), dtype=gpu.int64, device="cuda"), gpu.empty((1,), dtype=gpu.int32, device="cuda")
    bits = gpu.zeros((nq, (n + 31) // 32), dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def dcall(keys=d_keys, n_keys=n, n_groups=1, allow=bits, n_bitmaps=nq, words=(n + 31) // 32, k=4):
        return L.rass_index_search_grouped_keys_device(idx._h, vp(dq), nq, k, None if keys is None else vp(keys), n_keys, n_groups,
                                                       None if allow is None else vp(allow), n_bitmaps, words, None, None, 0,
                                                       vp(out[0]), vp(out[1]), vp(out[2]), vp(tot), vp(st))

    assert dcall() == N.RASS_OK and dcall(allow=None, n_bitmaps=0, words=0) == N.RASS_OK and dcall(n_bitmaps=1) == N.RASS_OK
    idx.engine.synchronize()
    for bad in (dict(n_bitmaps=2), dict(n_bitmaps=0), dict(words=(n + 31) // 32 - 1), dict(words=-1), dict(keys=None),
                dict(n_keys=n - 1), dict(n_keys=-1), dict(n_groups=0), dict(n_groups=(1 << 20) + 1), dict(k=0), dict(k=4097)):
        assert dcall(**bad) == INVALID, bad
    bf = eng.open_index("keys-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    with pytest.raises(N.RassError) as e:
        bf.search_grouped_by_keys(case.q_raw, 4, dev(gpu, np.zeros(64), np.int32), 1)
    assert e.value.code == UNSUPPORTED
    eng.drop_index(bf.name)
