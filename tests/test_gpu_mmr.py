"""The diversified (MMR) search and the Gram entry point on the GPU: ``rass_index_rows_gram(_device)`` and
``rass_index_search_mmr(_device)``.

What is held to what:
  * the Gram matrix to a float64 Gram matrix of the stored rows (``get_rows``), within the standard bound of a length-dim
    fp32 dot product in ANY summation order, |delta| <= dim * 2^-24 * sum_k |a_k b_k|, computed per pair; bitwise symmetry and
    exact zeros on padding are required on top;
  * the candidates to ``FlatIndex.search`` (itself held to the CPU oracle by the other suites): lambda = 1 must reproduce it;
  * the selection to ``tests/mmr_ref.select_f32`` over the engine's own candidate scores and Gram matrix: ranks, ids and
    scores must be EQUAL, no tolerance.

Shapes: dims 128, 1024 and 1536 (a K-panelled wide row), n = 20 (fewer rows than fetch_k, less than a tile), 1 000 and 4 128;
tombstones and two-field tags.  Each world is built once for the module."""
import ctypes

import numpy as np
import pytest

from tests import mmr_ref as R

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
PATIENT_MASK = 0x00FFFFFF
NQ_MAX = 70
SHAPES = [(20, 128), (1000, 128), (4128, 1024), (1000, 1536)]


class World:
    """48 Gaussian centres, rows = centre + 0.6 noise (normalised at add), two-field tags with tombstones; 70 queries, each
    three centres mixed with weights 1 / 0.8 / 0.6."""

    def __init__(self, n, dim):
        from rassengine_amd.engine import Engine
        rng = np.random.default_rng(9000 + n + dim)
        self.n, self.dim = n, dim
        centres = rng.standard_normal((48, dim), dtype=np.float32)
        x = centres[rng.integers(0, 48, size=n)] + np.float32(0.6) * rng.standard_normal((n, dim), dtype=np.float32)
        pick = np.stack([rng.permutation(48)[:3] for _ in range(NQ_MAX)])
        self.q_raw = (centres[pick[:, 0]] + np.float32(0.8) * centres[pick[:, 1]] + np.float32(0.6) * centres[pick[:, 2]]) * np.float32(3.0)
        self.tags = (rng.integers(0, 3 if n < 100 else 40, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)
        self.dead = sorted({3, n // 2, n - 1} if n < 100 else set(rng.choice(n, size=n // 25, replace=False).tolist()) | {n - 1, 31, 32})
        self.eng = Engine(0, dim)
        self.idx = self.eng.open_index("mmr")
        self.idx.add(x, tags=self.tags, normalize=True)
        for r in self.dead:
            self.idx.delete(int(r))
        self.tags = self.tags.copy()
        self.tags[self.dead] = -1
        self.stored = self.idx.get_rows(0, n).astype(np.float64)      # the rows as they lie in the slab
        self.qfilter = (self.tags[rng.integers(0, n, size=NQ_MAX)] & PATIENT_MASK).astype(np.int32)
        self.qfilter[::7] = -1                                        # some queries unfiltered
        self.qmask = np.full(NQ_MAX, PATIENT_MASK, dtype=np.int32)

    def flt(self, nq, masked):
        return dict(q_filter=self.qfilter[:nq], q_filter_mask=self.qmask[:nq]) if masked else {}

    def expect(self, nq, k, fetch_k, lam, masked=False):
        """The reference selection over the engine's own candidates (``search``) and Gram matrix (``rows_gram``)."""
        cs, ci = self.idx.search(self.q_raw[:nq], fetch_k, **self.flt(nq, masked))
        G = self.idx.rows_gram(ci)
        lam = np.broadcast_to(np.asarray(lam, dtype=np.float32), (nq,))
        es = np.full((nq, k), NEG_INF, dtype=np.float32)
        ei = np.full((nq, k), -1, dtype=np.int64)
        er = np.full((nq, k), -1, dtype=np.int32)
        for q in range(nq):
            p = R.select_f32(np.where(ci[q] >= 0, cs[q], NEG_INF), G[q], lam[q], k)
            es[q, :len(p)], ei[q, :len(p)], er[q, :len(p)] = cs[q, p], ci[q, p], p
        return es, ei, er


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids", "ranks")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def run_device(torch, idx, q_raw, k, fetch_k, lam, id_base=0, qfilter=None, qmask=None, ranks=True):
    nq = q_raw.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(q_raw, dtype=np.float32)).cuda()
    dl = torch.from_numpy(np.broadcast_to(np.asarray(lam, dtype=np.float32), (nq,)).copy()).cuda()
    df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter[:nq], dtype=np.int32)).cuda()
    dm = None if qmask is None else torch.from_numpy(np.ascontiguousarray(qmask[:nq], dtype=np.int32)).cuda()
    os_ = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    orank = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # the engine works on its own stream
    idx.search_mmr_device(dq.data_ptr(), nq, k, fetch_k, dl.data_ptr(), os_.data_ptr(), oi.data_ptr(),
                          d_out_rank_ptr=orank.data_ptr() if ranks else 0, id_base=id_base,
                          d_q_filter_ptr=0 if df is None else df.data_ptr(), d_q_filter_mask_ptr=0 if dm is None else dm.data_ptr())
    idx.engine.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy(), orank.cpu().numpy()


@pytest.fixture(scope="module")
def worlds(gpu):
    made = {}

    def get(n, dim):
        if (n, dim) not in made:
            made[(n, dim)] = World(n, dim)
        return made[(n, dim)]

    yield get
    for w in made.values():
        w.eng.close()


# ---------------------------------------------------------------------------------------------- 1. Gram accuracy
def gram_lists(w, L, n_lists, seed):
    """Random lists of length L; where there is room each holds a repeated ordinal, a -1, an out-of-range ordinal and a
    tombstoned row (L = 1: one list of each kind)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, w.n, size=(n_lists, L)).astype(np.int64)
    specials = [-1, w.n, int(w.dead[0]), w.n + 12345, -7]
    if L >= 8:
        for l in range(n_lists):
            pos = rng.permutation(L)[:6]
            rows[l, pos[0]] = rows[l, pos[1]]                          # a repeated ordinal
            rows[l, pos[2]], rows[l, pos[3]] = -1, w.n + l             # padding by value
            rows[l, pos[4]] = int(w.dead[l % len(w.dead)])             # a tombstoned row
            rows[l, pos[5]] = specials[l % len(specials)]
    else:
        for l in range(min(n_lists, len(specials))):
            rows[l, l % L] = specials[l]
    return rows


def check_gram(w, rows, got, what):
    n_lists, L = rows.shape
    assert got.shape == (n_lists, L, L) and got.dtype == np.float32
    live = (rows >= 0) & (rows < w.n)
    live[live] &= w.tags[rows[live]] != -1
    worst = 0.0
    for l in range(n_lists):
        r = w.stored[np.where(live[l], rows[l], 0)] * live[l][:, None]
        ref = R.gram_f64(r)
        bound = w.dim * 2.0 ** -24 * (np.abs(r) @ np.abs(r).T)
        err = np.abs(got[l].astype(np.float64) - ref)
        worst = max(worst, float(err.max()))
        assert np.all(err <= bound), (what, l, float(err.max()), float(bound[err > bound].min()))
        assert np.array_equal(got[l].view(np.uint32), got[l].T.view(np.uint32)), (what, l, "not bitwise symmetric")
        pad = ~live[l]
        assert np.all(got[l][pad, :].view(np.uint32) == 0) and np.all(got[l][:, pad].view(np.uint32) == 0), (what, l, "padding")
        d = np.flatnonzero(live[l])
        assert np.all(np.abs(got[l][d, d] - 1.0) < 1e-5)              # stored rows are unit vectors
    return worst


@pytest.mark.parametrize("n,dim", SHAPES)
def test_gram_accuracy(gpu, worlds, n, dim):
    w = worlds(n, dim)
    worst = 0.0
    for L in (1, 16, 17, 100, 128):
        rows = gram_lists(w, L, 5, seed=L + n)
        got = w.idx.rows_gram(rows)
        worst = max(worst, check_gram(w, rows, got, (n, dim, L)))
        # the device variant, and a list on its own: the same bits whatever the batch
        d_rows = gpu.from_numpy(rows).cuda()
        d_out = gpu.full((rows.shape[0], L, L), 7.0, dtype=gpu.float32, device="cuda")
        gpu.cuda.synchronize()
        w.idx.rows_gram_device(d_rows.data_ptr(), rows.shape[0], L, d_out.data_ptr())
        w.eng.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), got.view(np.uint32))
        assert np.array_equal(w.idx.rows_gram(rows[3]).view(np.uint32), got[3:4].view(np.uint32))
    print(f"rows_gram n={n} dim={dim}: max |delta| vs float64 = {worst:.3e}")


def test_gram_many_lists_cross_the_staging_groups(worlds):
    w = worlds(1000, 128)
    rows = gram_lists(w, 16, 300, seed=5)          # the host variant stages 256 lists of 16 at a time
    got = w.idx.rows_gram(rows)
    check_gram(w, rows, got, "300 lists")
    assert np.array_equal(w.idx.rows_gram(rows[270:290]).view(np.uint32), got[270:290].view(np.uint32))


def test_a_prefix_of_a_list_has_the_same_bits(worlds):
    """Element (i, j) is one chain whatever the list length and the tile it falls in: the MMR call's [fetch_k] lists and a
    caller's own lists agree bit for bit."""
    w = worlds(1000, 1536)
    rows = gram_lists(w, 128, 2, seed=11)
    full = w.idx.rows_gram(rows)
    for L in (1, 17, 100):
        assert np.array_equal(w.idx.rows_gram(np.ascontiguousarray(rows[:, :L])).view(np.uint32),
                              np.ascontiguousarray(full[:, :L, :L]).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. candidates
@pytest.mark.parametrize("n,dim,nqs,kf", [
    (1000, 128, (1, 32, 33, 70), ((1, 1), (8, 32), (10, 33), (32, 128), (128, 128))),
    (4128, 1024, (32, 33), ((8, 32), (10, 33), (128, 128))),
    (1000, 1536, (1, 33), ((8, 32), (10, 33), (32, 128))),
    (20, 128, (33,), ((1, 1), (10, 33), (128, 128))),
])
def test_lambda_one_reproduces_search(worlds, n, dim, nqs, kf):
    w = worlds(n, dim)
    for nq in nqs:
        for k, fetch_k in kf:
            for masked in (False, True):
                s, i = w.idx.search(w.q_raw[:nq], k, **w.flt(nq, masked))
                c = np.count_nonzero(i >= 0, axis=1)
                ranks = np.where(np.arange(k)[None, :] < c[:, None], np.arange(k, dtype=np.int32)[None, :], -1).astype(np.int32)
                got = w.idx.search_mmr(w.q_raw[:nq], k, fetch_k=fetch_k, lambda_mult=1.0, **w.flt(nq, masked))
                assert_same(got, (np.where(i >= 0, s, NEG_INF), i, ranks), ("lambda=1", n, dim, nq, k, fetch_k, masked))


# ---------------------------------------------------------------------------------------------- 3. selection
@pytest.mark.parametrize("n,dim,nq,k,fetch_k", [(1000, 128, 33, 8, 32), (4128, 1024, 32, 32, 128), (1000, 1536, 33, 10, 100),
                                               (4128, 1024, 70, 10, 40)])
def test_selection_equals_the_reference(worlds, n, dim, nq, k, fetch_k):
    w = worlds(n, dim)
    for lam in (0.0, 0.3, 0.5, 0.7):
        for masked in (False, True):
            want = w.expect(nq, k, fetch_k, lam, masked)
            got = w.idx.search_mmr(w.q_raw[:nq], k, fetch_k=fetch_k, lambda_mult=lam, **w.flt(nq, masked))
            assert_same(got, want, ("selection", n, dim, nq, k, fetch_k, lam, masked))
            if lam == 0.5 and not masked:       # not test 2 in disguise: the re-rank reorders
                reordered = sum(not np.array_equal(want[2][q], np.arange(k)) for q in range(nq))
                assert 2 * reordered >= nq, (reordered, nq)
    # one lambda per query
    lams = np.linspace(0.0, 1.0, nq).astype(np.float32)
    assert_same(w.idx.search_mmr(w.q_raw[:nq], k, fetch_k=fetch_k, lambda_mult=lams), w.expect(nq, k, fetch_k, lams), "per-query lambda")


# ---------------------------------------------------------------------------------------------- 4. meaning
def test_duplicates_are_passed_over(gpu):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(44)
    base = rng.standard_normal((128, 128)).astype(np.float32)
    x = np.repeat(base, 4, axis=0)                  # n = 512: every vector four times, at rows 4 v .. 4 v + 3
    q_raw = (base[rng.integers(0, 128, size=8)] + base[rng.integers(0, 128, size=8)] + rng.standard_normal((8, 128))).astype(np.float32)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("dups")
        idx.add(x, normalize=True)
        stored = idx.get_rows(0, 512).astype(np.float64)
        cs, ci = idx.search(q_raw, 32)
        assert len({int(r) // 4 for r in ci[0, :4]}) == 1                     # plain top-k: four copies of one vector
        G = idx.rows_gram(ci)
        got = idx.search_mmr(q_raw, 8, fetch_k=32, lambda_mult=0.5)
        for q in range(8):
            qn = q_raw[q].astype(np.float64) / np.linalg.norm(q_raw[q].astype(np.float64))
            ref = R.mmr_f64(qn, stored[ci[q]], 0.5, 8)
            assert len({int(ci[q, p]) // 4 for p in ref}) == 8, "the reference itself returns a duplicate"
            p = R.select_f32(cs[q], G[q], 0.5, 8)
            assert np.array_equal(got[2][q], p) and np.array_equal(got[1][q], ci[q, p]) and np.array_equal(got[0][q], cs[q, p])
            assert len({int(r) // 4 for r in got[1][q]}) == 8
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. exact ties
def test_exact_ties_give_rank_order(gpu):
    from rassengine_amd.engine import Engine
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("ties")
        idx.add(np.eye(128, dtype=np.float32), normalize=True)
        on = np.sort(np.random.default_rng(3).permutation(128)[:40])
        q = np.zeros((1, 128), dtype=np.float32)
        q[0, on] = 2.0
        for fetch_k, k in ((32, 8), (64, 48), (128, 128)):
            cs, ci = idx.search(q, fetch_k)
            assert np.array_equal(ci[0, :min(40, fetch_k)], on[:fetch_k]) and len(set(cs[0, :min(40, fetch_k)].tolist())) == 1
            for lam in (0.0, 0.3, 0.5, 1.0):
                s, i, r = idx.search_mmr(q, k, fetch_k=fetch_k, lambda_mult=lam)
                assert np.array_equal(r[0], np.arange(k)) and np.array_equal(i[0], ci[0, :k]) and np.array_equal(s[0], cs[0, :k]), (fetch_k, lam)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 6. short lists
def test_short_candidate_lists_pad(gpu, worlds):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(6)
    eng = Engine(0, 128)
    try:
        idx = eng.open_index("short")
        tags = np.array([1] * 5 + [2] * 15, dtype=np.int32)
        idx.add(rng.standard_normal((20, 128)).astype(np.float32), tags=tags, normalize=True)
        q = rng.standard_normal((3, 128)).astype(np.float32)
        f = np.array([1, 3, -1], dtype=np.int32)               # five rows; none; no filter (20 rows < fetch_k)
        cs, ci = idx.search(q, 32, q_filter=f)
        assert np.count_nonzero(ci >= 0, axis=1).tolist() == [5, 0, 20]
        G = idx.rows_gram(ci)
        s, i, r = idx.search_mmr(q, 8, fetch_k=32, lambda_mult=0.5, q_filter=f)
        for qi, c in enumerate((5, 0, 8)):
            p = R.select_f32(np.where(ci[qi] >= 0, cs[qi], NEG_INF), G[qi], 0.5, 8)
            assert len(p) == c
            assert np.array_equal(r[qi, :c], p) and np.array_equal(i[qi, :c], ci[qi, p]) and np.array_equal(s[qi, :c], cs[qi, p])
            assert np.all(r[qi, c:] == -1) and np.all(i[qi, c:] == -1) and np.all(s[qi, c:] == NEG_INF)
        assert sorted(i[0, :5].tolist()) == [0, 1, 2, 3, 4]
    finally:
        eng.close()
    # n = 20 with tombstones, k = fetch_k = 32: every live row once, then padding
    w = worlds(20, 128)
    s, i, r = w.idx.search_mmr(w.q_raw[:2], 32, fetch_k=32, lambda_mult=0.3)
    live = 20 - len(w.dead)
    assert_same((s, i, r), w.expect(2, 32, 32, 0.3), "n = 20")
    assert np.all(i[:, live:] == -1) and sorted(i[0, :live].tolist()) == [x for x in range(20) if x not in w.dead]


# ---------------------------------------------------------------------------------------------- 7. the device entry point
@pytest.mark.parametrize("n,dim,k,fetch_k", [(1000, 128, 10, 100), (1000, 1536, 10, 100), (4128, 1024, 8, 32)])
def test_device_entry_point(gpu, worlds, n, dim, k, fetch_k):
    w = worlds(n, dim)
    nq = 32
    lams = np.linspace(0.1, 0.9, nq).astype(np.float32)
    host = w.idx.search_mmr(w.q_raw[:nq], k, fetch_k=fetch_k, lambda_mult=lams, **w.flt(nq, True))
    dev = run_device(gpu, w.idx, w.q_raw[:nq], k, fetch_k, lams, qfilter=w.qfilter, qmask=w.qmask)
    assert_same(dev, host, "device = host")
    assert_same(host, w.expect(nq, k, fetch_k, lams, True), "host = reference")
    # id_base is added to real ids only; a NaN lambda and 1.5 give the empty list, the others are unaffected
    bad = lams.copy()
    bad[3], bad[17] = np.nan, 1.5
    host = w.idx.search_mmr(w.q_raw[:nq], k, fetch_k=fetch_k, lambda_mult=lams)
    s, i, r = run_device(gpu, w.idx, w.q_raw[:nq], k, fetch_k, bad, id_base=7_000_000_000)
    ok = np.ones(nq, dtype=bool)
    ok[[3, 17]] = False
    assert np.array_equal(s[ok], host[0][ok]) and np.array_equal(r[ok], host[2][ok])
    assert np.array_equal(i[ok], np.where(host[1][ok] >= 0, host[1][ok] + 7_000_000_000, -1))
    assert np.all(s[~ok] == NEG_INF) and np.all(i[~ok] == -1) and np.all(r[~ok] == -1)
    # no rank output asked for
    s2, i2, r2 = run_device(gpu, w.idx, w.q_raw[:5], k, fetch_k, lams[:5], ranks=False)
    assert np.array_equal(s2, host[0][:5]) and np.array_equal(i2, host[1][:5]) and np.all(r2 == 7)


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(gpu, worlds):
    import rassengine_amd._native as N
    from rassengine_amd.engine import Engine
    w = worlds(1000, 128)
    L = w.idx._L
    q = np.ascontiguousarray(w.q_raw[:2])
    s = np.empty((2, 128), dtype=np.float32)
    i = np.empty((2, 128), dtype=np.int64)
    r = np.empty((2, 128), dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(handle, k, fetch_k, lam=(0.5, 0.5), flt=None, msk=None, rank=r):
        return L.rass_index_search_mmr(handle, p(q), 2, k, fetch_k, p(np.array(lam, dtype=np.float32)), p(flt), p(msk), p(s), p(i), p(rank))

    assert call(w.idx._h, 8, 32) == N.RASS_OK and call(w.idx._h, 8, 32, rank=None) == N.RASS_OK
    assert call(w.idx._h, 33, 32) == -1 and call(w.idx._h, 0, 32) == -1 and call(w.idx._h, 8, 129) == -1 and call(w.idx._h, 1, 0) == -1
    assert call(w.idx._h, 8, 32, lam=(0.5, np.nan)) == -1 and b"lambda" in L.rass_last_error()
    assert call(w.idx._h, 8, 32, lam=(-0.1, 0.5)) == -1 and call(w.idx._h, 8, 32, lam=(0.5, 1.5)) == -1
    assert call(w.idx._h, 8, 32, msk=np.full(2, PATIENT_MASK, dtype=np.int32)) == -1
    rows = np.zeros((2, 4), dtype=np.int64)
    g = np.empty((2, 128, 128), dtype=np.float32)
    assert L.rass_index_rows_gram(w.idx._h, p(rows), 2, 4, p(g)) == N.RASS_OK
    assert L.rass_index_rows_gram(w.idx._h, p(rows), 2, 0, p(g)) == -1 and L.rass_index_rows_gram(w.idx._h, p(rows), 0, 4, p(g)) == -1
    assert L.rass_index_rows_gram(w.idx._h, p(rows), 2, 129, p(g)) == -1 and L.rass_index_rows_gram(w.idx._h, None, 2, 4, p(g)) == -1
    with pytest.raises(N.RassError) as e:
        run_device(gpu, w.idx, w.q_raw[np.zeros(33, dtype=np.int64)], 4, 16, 0.5)           # nq > 32 on the device variant
    assert e.value.code == -1
    eng = Engine(0, 128)
    try:
        # a bf16 index (its dim is a multiple of 256): unsupported
        eng_bf = Engine(0, 256)
        try:
            bf = eng_bf.open_index("mmr-bf16", dtype="bf16")
            bf.add(np.random.default_rng(8).standard_normal((64, 256)).astype(np.float32), normalize=True)
            q256 = np.ones((2, 256), dtype=np.float32)
            assert L.rass_index_search_mmr(bf._h, p(q256), 2, 8, 32, p(np.array([0.5, 0.5], dtype=np.float32)), None, None, p(s), p(i),
                                           p(r)) == -5
            assert L.rass_index_rows_gram(bf._h, p(rows), 2, 4, p(g)) == -5
            with pytest.raises(N.RassError) as e:
                run_device(gpu, bf, q256, 4, 16, 0.5)
            assert e.value.code == -5
        finally:
            eng_bf.close()
        # caller-assigned ids: served with rass_index_search_ex's limit — fetch_k <= 32 reports them, beyond is unsupported
        gid = eng.open_index("mmr-gid")
        x = w.stored[:700].astype(np.float32)
        gid.add(x[:300], normalize=False, first_global_id=1000)
        gid.add(x[300:], normalize=False, first_global_id=50_000)
        gids = np.concatenate([1000 + np.arange(300), 50_000 + np.arange(400)]).astype(np.int64)
        cs, ci = gid.search(w.q_raw[:5], 32)
        assert np.all(np.isin(ci, gids))
        rows_of = np.searchsorted(gids, ci)
        G = gid.rows_gram(rows_of)
        got = gid.search_mmr(w.q_raw[:5], 8, fetch_k=32, lambda_mult=0.5)
        dev = run_device(gpu, gid, w.q_raw[:5], 8, 32, 0.5, id_base=123)                    # id_base ignored
        for qi in range(5):
            pk = R.select_f32(cs[qi], G[qi], 0.5, 8)
            assert np.array_equal(got[2][qi], pk) and np.array_equal(got[1][qi], ci[qi, pk]) and np.array_equal(got[0][qi], cs[qi, pk])
        assert_same(dev, got, "gid device")
        with pytest.raises(N.RassError) as e:
            gid.search_mmr(w.q_raw[:5], 8, fetch_k=33)
        assert e.value.code == -5
        with pytest.raises(N.RassError) as e:
            run_device(gpu, gid, w.q_raw[:5], 8, 33, 0.5)
        assert e.value.code == -5
    finally:
        eng.close()


def test_the_prefilter_mode_is_ignored(worlds):
    w = worlds(4128, 1024)
    want = w.idx.search_mmr(w.q_raw[:33], 8, fetch_k=16, lambda_mult=0.5)
    w.idx.set_prefilter("int8")
    try:
        got = w.idx.search_mmr(w.q_raw[:33], 8, fetch_k=16, lambda_mult=0.5)
    finally:
        w.idx.set_prefilter(False)
    assert_same(got, want, "prefilter mode")


# ---------------------------------------------------------------------------------------------- 9. HipIndexer
def test_semantic_search_diverse_end_to_end(gpu):
    from rassengine_amd import indexer
    from rassengine_amd.docstore import REGISTRY, IndexState
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(99)
    dim, name = 128, "mmr-e2e"
    topic = rng.standard_normal(dim).astype(np.float32)
    base = (topic[None, :] + 0.7 * rng.standard_normal((12, dim))).astype(np.float32)      # 12 different chunks on one topic
    emb = np.repeat(base, 3, axis=0)                                                       # each uploaded three times
    docs = [{"doc_id": f"c{v}-{c}", "patientId": f"p{v % 2}", "doc_type": "note", "text": f"chunk {v}"} for v in range(12) for c in range(3)]
    eng = Engine(0, dim)
    try:
        REGISTRY.put(IndexState(name, eng.open_index(name)))
        indexer.add_documents(name, docs, emb)
        hip = indexer.HipIndexer(None, name)
        plain = hip.semantic_search(topic, k=6)
        assert len({d["text"] for d, _ in plain}) == 2                                     # two chunks, three copies each
        st = REGISTRY.get(name, create=False)
        for kw, n_distinct in ((dict(), 12), (dict(patient_id="p1"), 6)):
            cs, ci = st.index.search(topic[None, :], 16) if not kw else \
                st.index.search(topic[None, :], 16, q_filter=np.array([st.filter_for("p1", None)[0]], dtype=np.int32),
                                q_filter_mask=np.array([st.filter_for("p1", None)[1]], dtype=np.int32))
            p = R.select_f32(np.where(ci[0] >= 0, cs[0], NEG_INF), st.index.rows_gram(ci)[0], 0.5, 6)
            texts = [st.row_doc[int(ci[0, j])]["text"] for j in p]
            assert len(set(texts)) == 6, "the reference selection itself repeats a chunk"
            hits = hip.semantic_search_diverse(topic, k=6, fetch_k=16, lambda_mult=0.5, **kw)
            assert [d["text"] for d, _ in hits] == texts                                   # no text twice
            assert [sc for _, sc in hits] == [indexer._score_out(float(cs[0, j])) for j in p]
            assert all(d["patientId"] == "p1" for d, _ in hits) or not kw
        assert [d["doc_id"] for d, _ in hip.semantic_search_diverse(topic, k=6, lambda_mult=1.0)] == [d["doc_id"] for d, _ in plain]
    finally:
        REGISTRY.drop(name)
        eng.close()
