"""The stats sub-aggregation over a key column: ``rass_index_aggregate_stats_keys`` and its ``_device`` form — per bucket the
hit count and best hit of the terms aggregation plus count / sum / min / max of an attribute column over the bucket's hits.

The expected answer never comes from the engine: scores are the oracle's emulation of the scan's fmaf order
(``KIND_F32_MFMA``) for the queries as the GPU normalised them, and ``tests/stats_ref.py`` turns them into tables and bucket
lists.  Everything is integer arithmetic or a score the scan must reproduce bit for bit, so everything is compared with
``array_equal``.  Two tests are HIP against HIP and say so: the default order against ``rass_index_aggregate_keys``, and the
global form against ``rass_index_attr_minmax``."""
import ctypes

import numpy as np
import pytest

import stats_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5          # RASS_ERR_INVALID, RASS_ERR_UNSUPPORTED
NEG_INF = R.NEG_INF
MISSING = R.MISSING
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
I32_MAX = (1 << 31) - 1
# n, dim, nq: a partial tile; a padded stride; a full NT = 1 group; NT = 2 plus a second host group at CH = 8
SHAPES = [(33, 128, 2), (1000, 100, 1), (3000, 256, 16), (2500, 1024, 33)]
# attribute columns of every index here (NEVER is not set by anyone)
FULL, NEGATIVE, SPARSE, LEVELS, NEVER = 0, 1, 2, 3, 5
ORDERS = [(by, desc) for by in (R.BY_COUNT, R.BY_VALUE_COUNT, R.BY_MIN, R.BY_MAX) for desc in (True, False)]
ORDER_NAMES = {R.BY_COUNT: "_count", R.BY_VALUE_COUNT: "value_count", R.BY_MIN: "min", R.BY_MAX: "max"}


class Corpus:
    """Rows, queries, tags and value columns of one shape with the oracle's score matrix, computed once and never changed by a
    test.  Rows 2, 7 and n - 1 are one vector and query 0 points at it: a three-way tie at rank 1."""

    def __init__(self, torch, oracle, n, dim, nq):
        from rassengine_amd import ops
        rng = np.random.default_rng(9100 + n + dim + nq)
        self.n, self.dim, self.nq = n, dim, nq
        x = rng.standard_normal((n, dim), dtype=np.float32)
        x[7] = x[2]
        x[n - 1] = x[2]
        self.xn = oracle.normalize_ref(x).astype(np.float32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0
        self.q_raw[0] = x[2] * 2.0
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.ranked = -np.sort(-self.scores, axis=1)
        self.tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 4, size=n) << DSHIFT)).astype(np.int32)
        self.dead = rng.permutation(n)[:max(1, n // 40)]
        self.live_tags = self.tags.copy()
        self.live_tags[self.dead] = -1
        # uniform over every int32 above MISSING, both ends present: sums leave 32 bits, the biased encodings see both signs
        full = rng.integers(MISSING + 1, I32_MAX + 1, size=n)
        live = np.setdiff1d(np.arange(n), self.dead)
        full[live[0]], full[live[1]] = MISSING + 1, I32_MAX
        sparse = rng.integers(-1000, 1000, size=n)
        sparse[rng.random(n) < 0.2] = MISSING
        levels = rng.integers(0, 5, size=n) * 1000 - 2000                 # 5 distinct levels: the metrics tie across any cut
        levels[rng.random(n) < 0.2] = MISSING
        self.values = {FULL: full, NEGATIVE: -rng.integers(1, I32_MAX, size=n), SPARSE: sparse, LEVELS: levels, NEVER: None}

    def at_rank(self, r):
        return self.ranked[:, min(r, self.n) - 1].copy()

    def fill(self, idx):
        idx.add(self.xn, tags=self.tags, normalize=False)
        for col, v in self.values.items():
            if v is not None:
                idx.set_attr(col, 0, v.astype(np.int32))


_CORPORA = {}


def corpus(torch, oracle, shape):
    return _CORPORA.setdefault(shape, Corpus(torch, oracle, *shape))


@pytest.fixture(scope="module")
def world(gpu, oracle):
    """shape -> (engine, index with tombstones and the value columns, corpus); built on first use, shared by the tests here."""
    from rassengine_amd.engine import Engine
    made = {}

    def get(shape):
        if shape not in made:
            case = corpus(gpu, oracle, shape)
            eng = Engine(0, case.dim)
            idx = eng.open_index("stats")
            case.fill(idx)
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


def device_outputs(torch, nq, size):
    """The eleven outputs of the device variant, pre-filled with 7s."""
    shapes = [((nq, size), torch.int32), ((nq, size), torch.int64), ((nq, size), torch.float32), ((nq, size), torch.int64),
              ((nq, size), torch.int64), ((nq, size), torch.int64), ((nq, size), torch.int32), ((nq, size), torch.int32),
              ((nq,), torch.int64), ((nq,), torch.int64), ((1,), torch.int32)]
    return [torch.full(s, 7, dtype=t, device="cuda") for s, t in shapes]


def run_device(torch, idx, q_raw, thr, size, d_keys, n_groups, col, by=R.BY_COUNT, desc=True, allow=None, qfilter=None, qmask=None,
               id_base=0):
    nq = q_raw.shape[0]
    dq, df, dm = dev(torch, q_raw), dev(torch, qfilter, np.int32), dev(torch, qmask, np.int32)
    dt = dev(torch, np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,)).copy())
    da = None if allow is None else dev(torch, R.pack_bits(allow).view(np.int32))
    n_bitmaps, words = (0, 0) if da is None else ((1 if da.dim() == 1 else da.shape[0]), da.shape[-1])
    out = device_outputs(torch, nq, size)
    torch.cuda.synchronize()
    idx.search_stats_by_keys_device(dq.data_ptr(), nq, dt.data_ptr(), size, ptr(d_keys), 0 if d_keys is None else d_keys.shape[0],
                                    n_groups, col, *[o.data_ptr() for o in out], order_by=ORDER_NAMES[by], descending=desc,
                                    d_allow_ptr=ptr(da), n_bitmaps=n_bitmaps, words_per_bitmap=words, id_base=id_base,
                                    d_q_filter_ptr=ptr(df), d_q_filter_mask_ptr=ptr(dm))
    idx.engine.synchronize()
    return tuple(o.cpu().numpy() for o in out[:10]) + (int(out[10].item()),)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, R.NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check(torch, idx, case, tags, keys, n_groups, col, size, thr, orders=((R.BY_COUNT, True),), allow=None, qfilter=None, qmask=None,
          ids=None, values=None, host=True, device=True, what=""):
    """Host variant (any nq) and device variant (groups of <= 32) under every order of ``orders`` against the numpy answer; the
    table behind it is computed once.  Returns the answer under the first order."""
    values = case.values[col] if values is None else values
    d_keys = dev(torch, keys, np.int32)
    words = None if allow is None else dev(torch, R.pack_bits(allow).view(np.int32))
    tab = R.table(case.scores, tags, keys, values, n_groups, thr, allow, qfilter, qmask)
    sl_of = lambda a, sl: None if a is None else a[sl]
    allow_q = lambda sl: None if allow is None else (allow if allow.ndim == 1 else allow[sl])
    thr_q = np.broadcast_to(np.asarray(thr, dtype=np.float32), (case.nq,))
    first = None
    for by, desc in orders:
        want = R.expect(case.scores, tags, keys, values, n_groups, size, thr, by, desc, ids=ids, tab=tab)
        assert want[10] == 0
        first = first or want
        tag = f"{what} order {ORDER_NAMES[by]} {'desc' if desc else 'asc'} size {size}"
        if host:
            got = idx.search_stats_by_keys(case.q_raw, thr, size, d_keys, n_groups, col, ORDER_NAMES[by], desc, allow=words,
                                           q_filter=qfilter, q_filter_mask=qmask)
            assert_same(got, want, tag + " host")
        for q0 in range(0, case.nq if device else 0, 32):
            sl = slice(q0, min(q0 + 32, case.nq))
            got = run_device(torch, idx, case.q_raw[sl], thr_q[sl], size, d_keys, n_groups, col, by, desc, allow_q(sl),
                             sl_of(qfilter, sl), sl_of(qmask, sl))
            assert got[10] == 0
            assert_same(got, tuple(w[sl] for w in want[:10]), tag + " device")
    return first


def key_styles(rng, n):
    """name -> (keys, n_groups): random keys over 7 and over 300 groups with ~10 % of the rows in no group; runs of 32 aligned to
    the tiles (every half shares a group: the reduced path); runs of 32 offset by 16 (every half straddles two groups: the
    per-lane path); None = one group."""
    def holes(k):
        k = k.copy()
        k[rng.random(n) < 0.1] = -1
        return k
    return {"random 7": (holes(rng.integers(0, 7, size=n)), 7), "random 300": (holes(rng.integers(0, 300, size=n)), 300),
            "runs": ((np.arange(n) // 32) % 11, 11), "runs + 16": (((np.arange(n) + 16) // 32) % 11, 11), "global": (None, 1)}


def thresholds(case):
    """At the score of rank 1 (a three-way tie for query 0), rank 50 and n / 2; just above the maximum; -inf; mixed per query."""
    nq = case.nq
    above = np.nextafter(case.ranked[:, 0], np.float32(np.inf))
    mixed = np.where(np.arange(nq) % 3 == 0, NEG_INF, np.where(np.arange(nq) % 3 == 1, case.at_rank(50), above)).astype(np.float32)
    return {"rank 1": case.at_rank(1), "rank 50": case.at_rank(50), "n / 2": case.at_rank(case.n // 2), "above the maximum": above,
            "-inf": np.full(nq, NEG_INF), "mixed": mixed}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_match_oracle(gpu, world, shape):
    eng, idx, case = world(shape)
    n, dim, nq = shape
    rng = np.random.default_rng(n + dim)
    tags = case.live_tags
    assert case.scores[0, 2] == case.scores[0, 7] == case.scores[0, n - 1] == case.ranked[0, 0]    # the tie sits AT rank 1
    thrs = thresholds(case)
    styles = key_styles(rng, n)
    for name, (keys, n_groups) in styles.items():
        for tname, thr in thrs.items():
            want = check(gpu, idx, case, tags, keys, n_groups, FULL, 10, thr, what=f"{name} {tname}")
            if tname == "above the maximum":
                assert not want[8].any() and not want[9].any()               # no hit: the zeroed table is the answer
    # the other value columns: all negative; ~20 % missing; a column never set; one bucket whose hits are all missing
    keys, n_groups = styles["random 300"]
    for tname in ("rank 50", "-inf"):
        for col in (NEGATIVE, SPARSE, NEVER):
            want = check(gpu, idx, case, tags, keys, n_groups, col, 300, thrs[tname], what=f"column {col} {tname}")
            if col == NEVER:
                assert not want[4].any() and not want[5].any() and not want[6].any() and not want[7].any() and want[1].any()
        for style in ("runs", "runs + 16", "global"):
            check(gpu, idx, case, tags, *styles[style], SPARSE, 11, thrs[tname], what=f"sparse {style} {tname}")
    hollow = case.values[SPARSE].copy()
    g0 = int(keys[keys >= 0][0])                                         # a group that exists at every shape
    hollow[keys == g0] = MISSING
    scratch = eng.open_index("hollow")
    try:
        scratch.add(case.xn, tags=tags.clip(min=0), normalize=False)
        scratch.set_attr(0, 0, hollow.astype(np.int32))
        want = check(gpu, scratch, case, tags.clip(min=0), keys, n_groups, 0, 300, NEG_INF, values=hollow,
                     orders=[(R.BY_COUNT, True), (R.BY_MAX, True), (R.BY_MIN, False)], what="a bucket without a value")
        at = want[0] == g0
        assert at.any() and np.all(want[1][at] > 0) and not want[4][at].any() and not want[7][at].any()
    finally:
        eng.drop_index(scratch.name)


def test_orders_and_size_cuts(gpu, world):
    """The four order_by values, ascending and descending, with the metrics tying across the cut (5 distinct levels, ~20 %
    missing, a few buckets with no value at all): ties by key, no-value buckets last in both directions; sizes 1, 10 and all."""
    eng, idx, case = world(SHAPES[2])
    n = case.n
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 300, size=n)
    keys[rng.random(n) < 0.1] = -1
    values = case.values[LEVELS].copy()
    values[np.isin(keys, (4, 150, 299))] = MISSING
    scratch = eng.open_index("orders")
    try:
        scratch.add(case.xn, tags=case.tags, normalize=False)
        scratch.set_attr(0, 0, values.astype(np.int32))
        for tname, thr in (("-inf", NEG_INF), ("n / 2", case.at_rank(n // 2)), ("rank 50", case.at_rank(50))):
            for size in (1, 10, 300):
                want = check(gpu, scratch, case, case.tags, keys, 300, 0, size, thr, orders=ORDERS, values=values, device=size == 10,
                             what=f"orders {tname}")
            assert want[8].min() > 10 or tname == "rank 50"
    finally:
        eng.drop_index(scratch.name)


def test_select_at_the_list_bound(gpu, oracle):
    """5 000 buckets, 4 096 and 4 095 of them listed: the radix select cuts inside a run of equal metrics."""
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, (5200, 128, 2))
    n = case.n
    keys = np.arange(n) % 5000
    values = (np.arange(n) % 7 - 3) * 100
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("bound")
        idx.add(case.xn, tags=case.tags, normalize=False)
        idx.set_attr(2, 0, values.astype(np.int32))
        for size in (4096, 4095):
            want = check(gpu, idx, case, case.tags, keys, 5000, 2, size, NEG_INF, values=values,
                         orders=[(R.BY_COUNT, True), (R.BY_MAX, True), (R.BY_MIN, False), (R.BY_VALUE_COUNT, False)], what="5 000 buckets")
            assert np.all(want[8] == 5000) and np.all(want[0][:, size - 1] >= 0)
    finally:
        eng.close()


def test_contention_on_a_full_grid(gpu, oracle):
    """Every row of a full grid a hit of ONE slot per query (the global form: all traffic of a query on five words), of 8 slots
    in aligned runs (reduced) and of 8 slots row by row (per lane)."""
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, (16500, 128, 32))
    n = case.n
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("contention")
        case.fill(idx)
        for what, keys, n_groups in (("one slot", None, 1), ("8 slots in runs", (np.arange(n) // 32) % 8, 8), ("8 slots by row", np.arange(n) % 8, 8)):
            for col in (FULL, SPARSE):
                want = check(gpu, idx, case, case.tags, keys, n_groups, col, 8, NEG_INF, what=f"{what} column {col}")
                assert np.all(want[9] == n)
                if col == FULL:
                    assert np.abs(want[5]).max() > 1 << 33                   # the sums have left 32 bits
    finally:
        eng.close()


def test_sparse_keys_at_the_group_bound(gpu, world):
    eng, idx, case = world(SHAPES[1])
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 1 << 20, size=case.n)
    keys[:3] = ((1 << 20) - 1, 0, (1 << 20) - 1)
    for thr in (case.at_rank(50), NEG_INF):
        check(gpu, idx, case, case.live_tags, keys, 1 << 20, FULL, 10, thr, orders=ORDERS, what="2^20 groups")
        check(gpu, idx, case, case.live_tags, keys, 1 << 20, SPARSE, 4096, thr, orders=[(R.BY_MIN, True)], what="2^20 groups")


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_filters_and_bitmaps(gpu, world, shape):
    eng, idx, case = world(shape)
    n, dim, nq = shape
    rng = np.random.default_rng(n)
    tags = case.live_tags
    keys = rng.integers(0, 37, size=n)
    keys[rng.random(n) < 0.1] = -1
    thr = case.at_rank(n // 2)
    exact = np.where(np.arange(nq) % 3 == 2, -1, case.tags[np.arange(nq) % n]).astype(np.int32)
    by_dt = np.where(np.arange(nq) % 4 == 3, 9 << DSHIFT, ((np.arange(nq) % 3) + 1) << DSHIFT).astype(np.int32)
    by_p = (np.arange(nq) % 7 - 1).astype(np.int32)
    for what, f, m in (("exact", exact, None), ("doc type", by_dt, np.full(nq, DMASK, np.int32)), ("patient", by_p, np.full(nq, PMASK, np.int32))):
        check(gpu, idx, case, tags, keys, 37, SPARSE, 10, thr, qfilter=f, qmask=m, what=f"filter {what}")
        check(gpu, idx, case, tags, None, 1, FULL, 1, NEG_INF, qfilter=f, qmask=m, what=f"filter {what}, global")
    per_q = rng.random((nq, n)) < 0.3
    for what, allow in (("per query", per_q), ("shared", per_q[0]), ("empty", np.zeros(n, dtype=bool)), ("full", np.ones(n, dtype=bool))):
        want = check(gpu, idx, case, tags, keys, 37, SPARSE, 10, thr, allow=allow, orders=[(R.BY_COUNT, True), (R.BY_MAX, False)],
                     what=f"bitmap {what}")
        check(gpu, idx, case, tags, None, 1, FULL, 1, NEG_INF, allow=allow, qfilter=by_p, qmask=np.full(nq, PMASK, np.int32),
              what=f"bitmap {what}, global, filtered")
        if what == "empty":
            assert not want[9].any()
        if what == "full":
            assert_same(want, R.expect(case.scores, tags, keys, case.values[SPARSE], 37, 10, thr), "all set = no bitmap")


def test_tombstones_before_and_after_a_compaction(gpu, oracle):
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SHAPES[2])
    n = case.n
    keys = (np.arange(n) // 5) % 40
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("compacted")
        case.fill(idx)
        for r in case.dead:
            idx.delete(int(r))
        thr = case.at_rank(n // 2)
        check(gpu, idx, case, case.live_tags, keys, 40, SPARSE, 40, thr, orders=ORDERS[:4], what="tombstones")
        old_to_new = idx.compact()
        live = np.flatnonzero(old_to_new >= 0)
        assert len(live) == n - len(case.dead)

        class Moved:      # the same corpus as the compacted index holds it
            nq, q_raw, scores = case.nq, case.q_raw, np.ascontiguousarray(case.scores[:, live])
            values = {c: (None if v is None else v[live]) for c, v in case.values.items()}
        check(gpu, idx, Moved, case.tags[live], keys[live], 40, SPARSE, 40, thr, orders=ORDERS[:4], what="compacted")
        check(gpu, idx, Moved, case.tags[live], None, 1, FULL, 1, NEG_INF, what="compacted, global")
    finally:
        eng.close()


def test_keys_shorter_than_the_index(gpu, oracle):
    """Rows appended after the column was built: the device call refuses the short column, the Python wrapper pads it with 'no
    group' (and a short bitmap with zero words); the appended rows have no value either."""
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SHAPES[2])
    n, first = case.n, 2000
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("short")
        idx.add(case.xn[:first], tags=case.tags[:first], normalize=False)
        idx.set_attr(0, 0, case.values[SPARSE][:first].astype(np.int32))
        built = dev(gpu, np.arange(first) % 11, np.int32)
        bits = gpu.full(((first + 31) // 32,), -1, dtype=gpu.int32, device="cuda")
        idx.add(case.xn[first:], tags=case.tags[first:], normalize=False)
        keys = np.concatenate([np.arange(first) % 11, np.full(n - first, -1)])
        values = np.concatenate([case.values[SPARSE][:first], np.full(n - first, MISSING)])
        allow = np.concatenate([np.ones((first + 31) // 32 * 32, dtype=bool), np.zeros(n, dtype=bool)])[:n]
        for a_dev, a_ref in ((None, None), (bits, allow)):
            want = R.expect(case.scores, case.tags, keys, values, 11, 20, case.at_rank(500), R.BY_MAX, True, a_ref)
            got = idx.search_stats_by_keys(case.q_raw, case.at_rank(500), 20, built, 11, 0, "max", True, allow=a_dev)
            assert_same(got, want, "padded")
        with pytest.raises(N.RassError) as e:
            run_device(gpu, idx, case.q_raw, NEG_INF, 20, built, 11, 0)
        assert e.value.code == INVALID and "n_keys" in str(e.value)
        # the global form has no column to outgrow: the appended rows count and carry no value
        want = R.expect(case.scores, case.tags, None, values, 1, 1, NEG_INF)
        assert_same(idx.search_stats_by_keys(case.q_raw, NEG_INF, 1, None, 1, 0), want, "global after an append")
        assert np.all(want[1][:, 0] == n) and np.all(want[4][:, 0] < first)
    finally:
        eng.close()


def test_caller_assigned_ids_and_id_base(gpu, oracle):
    from rassengine_amd.engine import Engine
    case = corpus(gpu, oracle, SHAPES[1])
    n = case.n
    keys = np.arange(n) % 25
    eng = Engine(0, case.dim)
    try:
        idx = eng.open_index("gid")
        idx.add(case.xn[:300], tags=case.tags[:300], normalize=False, first_global_id=1000)
        idx.add(case.xn[300:], tags=case.tags[300:], normalize=False, first_global_id=50_000)
        idx.set_attr(FULL, 0, case.values[FULL].astype(np.int32))
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(n - 300)]).astype(np.int64)
        want = check(gpu, idx, case, case.tags, keys, 25, FULL, 30, case.at_rank(400), orders=[(R.BY_COUNT, True), (R.BY_MIN, True)],
                     ids=gids, what="global ids")
        d_keys = dev(gpu, keys, np.int32)
        assert_same(run_device(gpu, idx, case.q_raw, case.at_rank(400), 30, d_keys, 25, FULL, id_base=123)[:10], want[:10], "id_base ignored")
        plain = eng.open_index("plain")
        plain.add(case.xn, tags=case.tags, normalize=False)
        plain.set_attr(FULL, 0, case.values[FULL].astype(np.int32))
        want = list(R.expect(case.scores, case.tags, keys, case.values[FULL], 25, 30, NEG_INF, R.BY_MAX, False))
        want[3] = np.where(want[3] >= 0, want[3] + 7_000_000_000, -1)
        got = run_device(gpu, plain, case.q_raw, NEG_INF, 30, d_keys, 25, FULL, R.BY_MAX, False, id_base=7_000_000_000)
        assert_same(got[:10], want[:10], "id_base")
    finally:
        eng.close()


def test_status_word(gpu, world):
    """A key >= n_groups raises the status word on a hit only — not below the threshold — and the hit is left out of every figure."""
    import rassengine_amd._native as N
    eng, idx, case = world(SHAPES[2])
    n = case.n
    tags = case.live_tags
    live = np.flatnonzero(tags != -1)
    bad_row = int(live[np.argmax(case.scores[0, live] < case.ranked[0, 99])])     # a live row outside query 0's best 100
    keys = np.arange(n) % 9
    keys[bad_row] = 9
    d_keys = dev(gpu, keys, np.int32)
    want = R.expect(case.scores, tags, keys, case.values[FULL], 9, 5, NEG_INF)
    got = run_device(gpu, idx, case.q_raw, NEG_INF, 5, d_keys, 9, FULL)
    assert want[10] == 1 and got[10] == 1
    assert_same(got[:10], want[:10], "key out of range")
    with pytest.raises(N.RassError) as e:
        idx.search_stats_by_keys(case.q_raw, NEG_INF, 5, d_keys, 9, FULL)
    assert e.value.code == INVALID and "n_groups" in str(e.value)
    thr = np.nextafter(case.scores[:, bad_row], np.float32(np.inf))               # just above the row in every query: no hit
    want = R.expect(case.scores, tags, keys, case.values[FULL], 9, 5, thr)
    assert want[10] == 0
    assert_same(idx.search_stats_by_keys(case.q_raw, thr, 5, d_keys, 9, FULL), want, "below the threshold")
    assert run_device(gpu, idx, case.q_raw, thr, 5, d_keys, 9, FULL)[10] == 0


def test_refusals_leave_the_outputs_untouched(gpu, world):
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    eng, idx, case = world(SHAPES[2])
    n, nq = case.n, case.nq
    L = idx._L
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    d_keys = dev(gpu, np.zeros(n), np.int32)
    dq, dt = dev(gpu, case.q_raw), dev(gpu, np.zeros(nq), np.float32)
    bits = gpu.zeros((nq, (n + 31) // 32), dtype=gpu.int32, device="cuda")
    out = device_outputs(gpu, nq, 4)
    gpu.cuda.synchronize()

    def dcall(index=idx, keys=d_keys, n_keys=n, n_groups=1, col=FULL, by=R.BY_COUNT, desc=1, allow=bits, n_bitmaps=nq,
              words=(n + 31) // 32, size=4, queries=nq):
        return L.rass_index_aggregate_stats_keys_device(index._h, vp(dq), queries, vp(dt), size, vp(keys), n_keys, n_groups, col, by, desc,
                                                        vp(allow), n_bitmaps, words, None, None, 0, *[vp(o) for o in out])

    def untouched():
        idx.engine.synchronize()
        return all(bool((o == 7).all()) for o in out)

    bad = [dict(col=-1), dict(col=8), dict(by=-1), dict(by=4), dict(size=0), dict(size=4097), dict(n_groups=0),
           dict(n_groups=(1 << 20) + 1), dict(keys=None, n_groups=2), dict(n_keys=n - 1), dict(n_keys=-1), dict(n_bitmaps=2),
           dict(n_bitmaps=0), dict(words=(n + 31) // 32 - 1), dict(words=-1), dict(queries=0), dict(queries=33)]
    for kw in bad:
        assert dcall(**kw) == INVALID, kw
    assert untouched()
    bf = eng.open_index("stats-bf16", dtype="bf16")
    bf.add(case.xn[:64], normalize=False)
    assert dcall(index=bf, keys=None, n_keys=0, allow=None, n_bitmaps=0, words=0) == UNSUPPORTED
    eng.drop_index(bf.name)
    wide = Engine(0, 1536)
    try:
        widx = wide.open_index("stats-wide")
        widx.add(np.ones((40, 1536), dtype=np.float32))
        assert L.rass_index_aggregate_stats_keys_device(widx._h, vp(dq), 1, vp(dt), 4, None, 0, 1, 0, 0, 1, None, 0, 0, None, None, 0,
                                                        *[vp(o) for o in out]) == UNSUPPORTED
        with pytest.raises(N.RassError) as e:
            widx.search_stats_by_keys(np.ones((1, 1536), dtype=np.float32), 0.0, 4, None, 1, 0)
        assert e.value.code == UNSUPPORTED
    finally:
        wide.close()
    assert untouched()
    # the host variant: a NaN threshold, with its outputs untouched as well
    host = [np.full((nq, 4), 7, dtype=t) for t in (np.int32, np.int64, np.float32, np.int64, np.int64, np.int64, np.int32, np.int32)]
    host += [np.full(nq, 7, dtype=np.int64), np.full(nq, 7, dtype=np.int64)]
    thr = np.zeros(nq, dtype=np.float32)
    thr[nq - 1] = np.nan
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    q = np.ascontiguousarray(case.q_raw)
    rc = L.rass_index_aggregate_stats_keys(idx._h, hp(q), nq, hp(thr), 4, vp(d_keys), n, 1, FULL, 0, 1, None, 0, 0, None, None,
                                           *[hp(a) for a in host])
    assert rc == INVALID and all((a == 7).all() for a in host)
    # ... which the device variant takes: that query matches nothing
    dthr = dev(gpu, thr)
    got = run_device(gpu, idx, case.q_raw, thr, 4, d_keys, 1, FULL)
    assert dthr is not None and got[9][nq - 1] == 0 and got[8][nq - 1] == 0 and got[9][0] > 0
    assert dcall() == N.RASS_OK and dcall(allow=None, n_bitmaps=0, words=0) == N.RASS_OK and dcall(keys=None, n_keys=0) == N.RASS_OK
    idx.engine.synchronize()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_default_order_equals_aggregate_keys(gpu, world, shape):
    """HIP against HIP: under RASS_STATS_BY_COUNT descending, groups / counts / scores / ids / n_buckets / total_hits are
    rass_index_aggregate_keys' on the same arguments."""
    eng, idx, case = world(shape)
    n, nq = case.n, case.nq
    rng = np.random.default_rng(3)
    keys = dev(gpu, np.where(rng.random(n) < 0.1, -1, rng.integers(0, 50, size=n)), np.int32)
    allow = dev(gpu, R.pack_bits(rng.random((nq, n)) < 0.5).view(np.int32))
    f = (np.arange(nq) % 7 - 1).astype(np.int32)
    m = np.full(nq, PMASK, np.int32)
    for thr in (case.at_rank(1), case.at_rank(50), NEG_INF):
        for size in (1, 10, 4096):
            for kw in (dict(), dict(allow=allow), dict(q_filter=f, q_filter_mask=m)):
                got = idx.search_stats_by_keys(case.q_raw, thr, size, keys, 50, SPARSE, **kw)
                ref = idx.search_counts_by_keys(case.q_raw, thr, size, keys, 50, **kw)
                for g, w, name in zip(got[:4] + got[8:], ref, ("groups", "counts", "scores", "ids", "n_buckets", "total_hits")):
                    assert g.dtype == w.dtype and np.array_equal(g, w), (name, size, sorted(kw))


def test_global_form_equals_attr_minmax(gpu, world):
    """HIP against HIP: NULL keys, -inf and no filter -> min / max / value_count are rass_index_attr_minmax's over the live rows."""
    for shape in SHAPES:
        eng, idx, case = world(shape)
        for col in (FULL, NEGATIVE, SPARSE, LEVELS, NEVER):
            lo, hi, present = idx.attr_minmax(col)
            got = idx.search_stats_by_keys(case.q_raw, NEG_INF, 1, None, 1, col)
            assert np.all(got[4][:, 0] == present) and np.all(got[1][:, 0] == case.n - len(case.dead)), (shape, col)
            if present:
                assert np.all(got[6][:, 0] == lo) and np.all(got[7][:, 0] == hi), (shape, col)
            else:
                assert not got[6].any() and not got[7].any() and not got[5].any()
