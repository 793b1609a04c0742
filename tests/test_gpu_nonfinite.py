"""Rows and queries that are not finite (include/rass_engine.h, "Scores that are not finite"): a live row whose score for a
query is NaN or -inf is, for that query, as if it were deleted, and a query that normalises to NaN gets the empty answer of
its entry point without disturbing the other queries of its call.

Every search form is held to that by two references, both independent of the path under test:
 * the fp64 oracle (or the numpy restatement the form already has) over the CLEANED corpus: the poisoned rows tombstoned and
   a finite row in the place of each, ids unchanged.  Each case takes, from a seeded pool, the queries for which no two
   reference scores of the top k + 1 lie within 2 TOL_F64 (``_pick``, on the CPU; ``check_topk`` asserts it again on the
   reference it is given), so the tie allowance is never used.  The grouped and counted forms ask for equal ids outright;
 * a TWIN index: A holds the poisoned rows, B got the same add calls with a random unit row in the place of each and then
   delete(row).  Every call on A must equal the same call on B bit for bit — that is what catches a stale or racy slot.

Poison kinds: an all-NaN row (add(normalize=True) of a vector with one NaN), a second one (from a vector with one +Inf), a
partly-NaN row stored with normalize=False.  They sit at row 0, at the last row of a partial tile, inside the sample prefix,
two in one half-wave's 32 rows, as one whole 32-row tile, as the only rows of a patient / group / key bucket, as several of a
patient's fewer than 32 rows, and next to the row at which a k = 100 search's second pass begins."""
import os

import numpy as np
import pytest

from tests import groupkeys_ref as GK
from tests import nonfinite_ref as NF
from tests.nonfinite_ref import PM, TOL_F64, assert_same, check_topk

pytestmark = pytest.mark.gpu

DIM = 256
DT_MASK = 0x7F000000
NEG = float("-inf")


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Case:
    pass


def _rank(all64, ok, k):
    """(scores f64 [nq, k], ids) of the rows ``ok`` [nq, n] under (score desc, row asc): the oracle's scores, ranked."""
    nq = all64.shape[0]
    rs, ri = np.full((nq, k), -np.inf), np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        rows = np.flatnonzero(ok[q])
        if len(rows) > 4 * k:              # only the rows at or above the k-th best score can rank
            rows = rows[all64[q, rows] >= -np.partition(-all64[q, rows], k - 1)[k - 1]]
        order = np.lexsort((rows, -all64[q, rows]))[:k]
        rs[q, :len(order)], ri[q, :len(order)] = all64[q, rows[order]], rows[order]
    return rs, ri


def _main_case(oracle):
    """3 117 x 256 (a partial last tile), tags = patient | doc type << 24, a key column, a pool of 160 queries: the CPU half
    of the ``main`` fixture (the cleaned corpus and its fp64 scores)."""
    rng = np.random.default_rng(2024)
    n = 3117
    x = rng.standard_normal((n, DIM)).astype(np.float32)
    patient = rng.integers(10, 60, size=n)
    patient[64:96] = 7                     # a patient (and group) whose only rows are one whole poisoned tile
    patient[2000:2020] = 9                 # a patient with 20 rows, 6 of them poisoned
    patient[0] = 500                       # a poisoned row whose group is >= n_groups: it must not set the status
    tags = (patient | (rng.integers(1, 4, size=n) << 24)).astype(np.int32)
    keys = rng.integers(0, 40, size=n).astype(np.int32)
    keys[::97] = -1                        # rows in no group
    keys[64:96] = 45                       # a key bucket whose only rows are poisoned
    keys[n - 1] = 1000                     # as patient[0]
    poison = {0: "nan", n - 1: "inf", 100: "part", 101: "nan", 2001: "nan", 2003: "part", 2004: "inf", 2010: "nan",
              2011: "part", 2019: "inf"}
    poison.update({r: NF.KINDS[r % 3] for r in range(64, 96)})
    Q = rng.standard_normal((160, DIM)).astype(np.float32)
    Q[2] = x[300] * 2.5
    # the rows next to the ones at which the first pass of 32 ends and the second begins, for the first 16 queries of the
    # pool (k = 100 runs four passes, each continuing behind the last (score, row) of the one before)
    xn0 = oracle.normalize_ref(x).astype(np.float32)
    t0 = np.zeros(n, dtype=np.int32)
    t0[sorted(poison)] = -1
    _, ri0 = oracle.search(xn0, oracle.normalize_ref(Q[:16]).astype(np.float32), 33, tags=t0)
    for seam in sorted(set((ri0[:, 31] + 1).tolist() + (ri0[:, 32] - 1).tolist())):
        if 0 < seam < n - 1 and seam not in poison and not 2000 <= seam < 2020 and seam != 300:
            poison[int(seam)] = "part"
    c = _Case()
    c.x, c.n, c.tags, c.keys, c.poison, c.Q, c.oracle = x, n, tags, keys, poison, Q, oracle
    c.xa, c.xb, c.norm = NF.twin_vectors(np.random.default_rng(7), x, poison)
    c.tags_ref = tags.copy()
    c.tags_ref[sorted(poison)] = -1
    c.xn = oracle.normalize_ref(c.xb).astype(np.float32)
    c.all64 = oracle.scores(c.xn, oracle.normalize_ref(Q).astype(np.float32))
    c.clean = np.setdiff1d(np.arange(n), sorted(poison))
    return c


@pytest.fixture(scope="module")
def main(gpu, oracle):
    from rassengine_amd.engine import Engine
    c = _main_case(oracle)
    c.eng = Engine(0, DIM)
    c.A, c.B = NF.open_twin(c.eng, "nf", c.xa, c.xb, c.norm, c.tags, c.poison)
    assert c.A.count == c.n and c.B.count == c.n - len(c.poison) and c.A.rows == c.B.rows == c.n
    yield c
    c.eng.close()


def _pick(c, nq, k, f=None, m=None, bits=None, must=(), thr=None):
    """``nq`` queries of the pool (their indices, ascending) whose reference top k + 1 — under the per-pool-query filter
    ``f`` / ``m`` and rows ``bits`` [pool, n] or [n] — holds no two scores within 2 TOL_F64 (and no live row's score within
    that of ``thr``), and that reference.  ``must``: pool queries that have to be among them (the ones a case is about)."""
    P = len(c.Q)
    ok = _ok(c, f, m, P)
    if bits is not None:
        ok &= bits
    rs, ri = _rank(c.all64, ok, k + 1)
    good = [j for j in range(P) if NF.no_near_ties(rs[j:j + 1]) and (thr is None or NF.clear_of(thr, c.all64[j:j + 1], c.tags_ref))]
    sel = np.array(good[:nq], dtype=np.int64)
    assert len(sel) == nq and all(j in sel for j in must), "reference near-ties: choose another seed"
    return sel, (rs[sel], ri[sel])


def _scores(c, q):
    return c.oracle.scores(c.xn, c.oracle.normalize_ref(q).astype(np.float32))


def _filters(c, kind, nq):
    if kind is None:
        return None, None
    rng = np.random.default_rng(nq)
    rows = c.clean[rng.integers(0, len(c.clean), size=nq)]
    if kind == "plain":                    # the whole tag
        f = c.tags[rows].copy()
        f[0] = c.tags[2002]                # patient 9: some of its rows with this doc type are poisoned
        if nq > 1:
            f[1] = c.tags[70]              # patient 7: poisoned rows only
        return f.astype(np.int32), None
    f = (c.tags[rows] & PM).astype(np.int32)
    f[0] = 9
    if nq > 2:
        f[1], f[2] = 7, -1
    return f, np.full(nq, PM, dtype=np.int32)


def _ok(c, f, m, nq):
    ok = np.broadcast_to(c.tags_ref != -1, (nq, c.n)).copy()
    if f is not None:
        for q in range(nq):
            if f[q] >= 0:
                ok[q] &= ((c.tags_ref & m[q]) if m is not None else c.tags_ref) == f[q]
    return ok


# ---- search: plain, masked, k = 10 and the continuation passes of k = 100 -------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "plain", "masked"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("nq", [1, 16, 32])
def test_search(main, nq, k, filt):
    c = main
    f, m = _filters(c, filt, len(c.Q))
    sel, _ = _pick(c, nq, k, f, m, must=() if filt is None else (0, 1)[:nq])     # patient 9's and patient 7's queries
    q = c.Q[sel]
    f, m = (None if f is None else f[sel]), (None if m is None else m[sel])
    a = c.A.search(q, k, q_filter=f, q_filter_mask=m)
    assert_same(a, c.B.search(q, k, q_filter=f, q_filter_mask=m), "twin")
    qn = c.oracle.normalize_ref(q).astype(np.float32)
    ref = c.oracle.search(c.xn, qn, k + 1, tags=c.tags_ref, qfilter=f, qmask=m)
    check_topk(a, ref, c.all64[sel], k)
    assert not np.isin(a[1], sorted(c.poison)).any() and not np.isnan(a[0]).any()
    if filt is not None and nq > 1:
        assert np.all(a[1][1] == -1)       # patient 7


def test_search_multi(main):
    c = main
    rng = np.random.default_rng(3)
    other = c.eng.open_index("nf-other")
    try:
        other.add(rng.standard_normal((500, DIM)).astype(np.float32))
        q = c.Q[:9]
        f = np.array([9, -1, 7, -1, -1, -1, 9, -1, -1], dtype=np.int32)
        m = np.full(9, PM, dtype=np.int32)
        pick = lambda X: [X if j % 2 == 0 else other for j in range(9)]
        a = c.eng.search_multi(pick(c.A), q, 10, q_filter=f, q_filter_mask=m)
        assert_same(a, c.eng.search_multi(pick(c.B), q, 10, q_filter=f, q_filter_mask=m), "twin")
        even = np.arange(0, 9, 2)
        qn = c.oracle.normalize_ref(q[even]).astype(np.float32)
        ref = c.oracle.search(c.xn, qn, 11, tags=c.tags_ref, qfilter=f[even], qmask=m[even])
        check_topk((a[0][even], a[1][even]), ref, _scores(c, q[even]), 10)
    finally:
        c.eng.drop_index("nf-other")


# ---- range ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "masked"])
@pytest.mark.parametrize("thr", [NEG, 0.12])
def test_search_range(main, thr, filt):
    c = main
    nq = 32
    f, m = _filters(c, filt, len(c.Q))
    sel, ref = _pick(c, nq, 20, f, m, bits=c.all64 >= thr, must=() if filt is None else (0, 1), thr=thr)
    q, all64 = c.Q[sel], c.all64[sel]
    f, m = (None if f is None else f[sel]), (None if m is None else m[sel])
    assert NF.clear_of(thr, all64, c.tags_ref)
    a = c.A.search_range(q, thr, max_hits=4096, q_filter=f, q_filter_mask=m)
    assert_same(a, c.B.search_range(q, thr, max_hits=4096, q_filter=f, q_filter_mask=m), "twin")
    hit = _ok(c, f, m, nq) & (all64 >= thr)
    assert np.array_equal(a[2], hit.sum(axis=1))
    for r in range(nq):
        got = a[1][r][a[1][r] >= 0]
        assert np.array_equal(np.sort(got), np.flatnonzero(hit[r]))
    check_topk((a[0][:, :20], a[1][:, :20]), ref, all64, 20)
    assert not np.isnan(a[0]).any()


# ---- grouped and counted, by tag field and by key column ------------------------------------------------------------------------
def _allow_bits(c, kind, nq):
    rng = np.random.default_rng(11)
    if kind is None:
        return None
    if kind == "mixed":                    # clean and poisoned rows
        bits = rng.random(c.n) < 0.3
        bits[sorted(c.poison)] = True
        return bits
    if kind == "poisoned":                 # poisoned rows only: the answer is empty
        bits = np.zeros(c.n, dtype=bool)
        bits[sorted(c.poison)] = True
        return bits
    bits = rng.random((nq, c.n)) < 0.2     # one per query
    bits[:, sorted(c.poison)] = True
    bits[3] = False
    bits[3, sorted(c.poison)] = True
    return bits


def _check_grouped(a, exp):
    es, ei, eg, et, status = exp
    assert status == 0
    assert np.array_equal(a[1], ei) and np.array_equal(a[2], eg) and np.array_equal(a[3], et)
    ok = ei >= 0
    assert np.all(np.abs(a[0][ok].astype(np.float64) - es[ok]) <= TOL_F64) and np.all(np.isneginf(a[0][~ok]))


def _check_counts(a, exp):
    eg, ec, es, ei, eb, et, status = exp
    assert status == 0
    assert np.array_equal(a[0], eg) and np.array_equal(a[1], ec) and np.array_equal(a[3], ei)
    assert np.array_equal(a[4], eb) and np.array_equal(a[5], et)
    ok = ei >= 0
    assert np.all(np.abs(a[2][ok].astype(np.float64) - es[ok]) <= TOL_F64) and np.all(np.isneginf(a[2][~ok]))


@pytest.mark.parametrize("k", [10, 70])
@pytest.mark.parametrize("filt", [None, "doctype"])
def test_search_grouped(main, k, filt):
    """By patient, 64 groups: patient 7 holds poisoned rows only and is no group; row 0 (patient 500 >= n_groups) is
    poisoned and must not fail the call."""
    c = main
    nq = 32
    q = c.Q[:nq]
    f = m = None
    if filt:
        f = ((np.arange(nq) % 3 + 1) << 24).astype(np.int32)
        m = np.full(nq, DT_MASK, dtype=np.int32)
    a = c.A.search_grouped(q, k, PM, 64, q_filter=f, q_filter_mask=m)
    assert_same(a, c.B.search_grouped(q, k, PM, 64, q_filter=f, q_filter_mask=m), "twin")
    all64 = _scores(c, q)
    _check_grouped(a, GK.expect_grouped(all64, c.tags_ref, c.tags_ref & PM, 64, k, qfilter=f, qmask=m))
    assert not (a[2] == 7).any() and not np.isnan(a[0]).any()


@pytest.mark.parametrize("allow", [None, "mixed", "poisoned", "per_query"])
def test_search_grouped_by_keys(main, allow):
    c = main
    nq = 32
    q = c.Q[:nq]
    bits = _allow_bits(c, allow, nq)
    words = None if bits is None else GK.pack_bits(bits)
    a = c.A.search_grouped_by_keys(q, 10, c.keys, 48, allow=words)
    assert_same(a, c.B.search_grouped_by_keys(q, 10, c.keys, 48, allow=words), "twin")
    _check_grouped(a, GK.expect_grouped(_scores(c, q), c.tags_ref, c.keys, 48, 10, allow=bits))
    assert not (a[2] == 45).any()
    if allow == "poisoned":
        assert np.all(a[1] == -1) and np.all(a[3] == 0)


@pytest.mark.parametrize("thr", [NEG, 0.1])
def test_search_counts(main, thr):
    c = main
    nq = 32
    q = c.Q[:nq]
    all64 = _scores(c, q)
    assert NF.clear_of(thr, all64, c.tags_ref)
    a = c.A.search_counts(q, thr, 16, PM, 64)
    assert_same(a, c.B.search_counts(q, thr, 16, PM, 64), "twin")
    _check_counts(a, GK.expect_counts(all64, c.tags_ref, c.tags_ref & PM, 64, 16, thr))
    assert not (a[0] == 7).any()
    # the best-row fold of a count scan takes only hits (s >= thr is false for NaN): no bucket is represented by a NaN
    assert not np.isnan(a[2]).any() and not np.isin(a[3], sorted(c.poison)).any()


@pytest.mark.parametrize("allow", [None, "mixed", "poisoned", "per_query"])
@pytest.mark.parametrize("thr", [NEG, 0.1])
def test_search_counts_by_keys(main, thr, allow):
    c = main
    nq = 32
    q = c.Q[:nq]
    all64 = _scores(c, q)
    assert NF.clear_of(thr, all64, c.tags_ref)
    bits = _allow_bits(c, allow, nq)
    words = None if bits is None else GK.pack_bits(bits)
    a = c.A.search_counts_by_keys(q, thr, 16, c.keys, 48, allow=words)
    assert_same(a, c.B.search_counts_by_keys(q, thr, 16, c.keys, 48, allow=words), "twin")
    _check_counts(a, GK.expect_counts(all64, c.tags_ref, c.keys, 48, 16, thr, allow=bits))
    assert not (a[0] == 45).any() and not np.isnan(a[2]).any()
    if allow == "poisoned":
        assert np.all(a[4] == 0) and np.all(a[5] == 0)


# ---- within a bitmap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("allow", ["mixed", "poisoned", "per_query"])
def test_search_allowed(main, allow, k):
    c = main
    nq = 32
    bits = _allow_bits(c, allow, len(c.Q))
    sel, ref = _pick(c, nq, k, bits=bits, must=(3,))
    q = c.Q[sel]
    bits = bits if bits.ndim == 1 else bits[sel]
    words = GK.pack_bits(bits)
    a = c.A.search_allowed(q, k, words)
    assert_same(a, c.B.search_allowed(q, k, words), "twin")
    check_topk(a, ref, c.all64[sel], k)
    if allow == "poisoned":
        assert np.all(a[1] == -1)
    if allow == "per_query":
        assert np.all(a[1][list(sel).index(3)] == -1)       # its bitmap names poisoned rows only


# ---- MMR ------------------------------------------------------------------------------------------------------------------------
def test_search_mmr(main):
    c = main
    nq = 32
    q = c.Q[:nq]
    f, m = _filters(c, "masked", nq)
    lam = np.linspace(0.0, 1.0, nq).astype(np.float32)
    for kw in (dict(), dict(q_filter=f, q_filter_mask=m)):
        a = c.A.search_mmr(q, 8, fetch_k=32, lambda_mult=lam, **kw)
        assert_same(a, c.B.search_mmr(q, 8, fetch_k=32, lambda_mult=lam, **kw), "twin")
        assert not np.isnan(a[0]).any() and not np.isin(a[1], sorted(c.poison)).any()
    # lambda = 1 is the plain top-k: the oracle's
    sel, (rs, top) = _pick(c, nq, 32)
    q = c.Q[sel]
    a = c.A.search_mmr(q, 8, fetch_k=32, lambda_mult=1.0)
    check_topk(a[:2], (rs[:, :9], top[:, :9]), c.all64[sel], 8)
    # every pick is one of the oracle's top fetch_k (no near-ties among its 33 best), at the rank the engine reports
    a = c.A.search_mmr(q, 8, fetch_k=32, lambda_mult=0.5)
    assert_same(a, c.B.search_mmr(q, 8, fetch_k=32, lambda_mult=0.5), "twin")
    for r in range(nq):
        assert np.array_equal(top[r][a[2][r]], a[1][r])


# ---- the exact re-rank behind the bf16 / int8 / certified prefilters ------------------------------------------------------------
@pytest.fixture(scope="module")
def slab40(gpu, oracle):
    """40 rows, 12 of them poisoned: every live row is a re-rank candidate, and fewer than 32 of them are valid."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(40)
    x = rng.standard_normal((40, DIM)).astype(np.float32)
    poison = {r: NF.KINDS[j % 3] for j, r in enumerate((0, 1, 5, 6, 7, 15, 16, 20, 31, 32, 38, 39))}
    c = _Case()
    c.eng = Engine(0, DIM)
    c.A, c.B, xb, c.tags_ref = NF.build_twin(c.eng, "nf40", x, None, poison, np.random.default_rng(41))
    c.n, c.poison, c.oracle = 40, poison, oracle
    c.xn = oracle.normalize_ref(xb).astype(np.float32)
    c.Q = rng.standard_normal((64, DIM)).astype(np.float32)
    c.all64 = oracle.scores(c.xn, oracle.normalize_ref(c.Q).astype(np.float32))
    yield c
    c.eng.close()


def _device_search(torch, c, ix, q, k, f=None, m=None):
    """search_device into buffers pre-filled with a sentinel: a slot the kernels do not write shows."""
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(q).to(dev)
    df = torch.from_numpy(f).to(dev) if f is not None else None
    dm = torch.from_numpy(m).to(dev) if m is not None else None
    ds = torch.full((q.shape[0], k), 777.0, dtype=torch.float32, device=dev)
    di = torch.full((q.shape[0], k), -777, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), q.shape[0], k, ds.data_ptr(), di.data_ptr(), 0, df.data_ptr() if f is not None else 0,
                     dm.data_ptr() if m is not None else 0)
    c.eng.synchronize()
    return ds.cpu().numpy(), di.cpu().numpy()


@pytest.mark.parametrize("mode", ["bf16", "int8", "int8_exact"])
def test_prefilter_small_patient(gpu, main, mode):
    """A filter that matches fewer than 32 rows: every matching row, the poisoned ones included, is a re-rank candidate."""
    c = main
    nq = 8
    f = np.array([7 if j % 4 == 1 else 9 for j in range(len(c.Q))], dtype=np.int32)
    m = np.full(len(c.Q), PM, dtype=np.int32)
    sel, (rs, ri) = _pick(c, nq, 32, f, m, must=(0, 1))
    q, f, m = c.Q[sel], f[sel], m[sel]
    qn = c.oracle.normalize_ref(q).astype(np.float32)
    try:
        c.A.set_prefilter(mode)
        c.B.set_prefilter(mode)
        for k in (10, 32):
            a = c.A.search(q, k, q_filter=f, q_filter_mask=m)
            assert_same(a, c.A.search(q, k, q_filter=f, q_filter_mask=m), "second call")
            assert_same(a, c.B.search(q, k, q_filter=f, q_filter_mask=m), "twin")
            assert_same(a, _device_search(gpu, c, c.A, q, k, f, m), "device entry point")
            check_topk(a, c.oracle.search(c.xn, qn, k + 1, tags=c.tags_ref, qfilter=f, qmask=m), c.all64[sel], k)
            assert (a[1][0] >= 0).sum() == min(k, 14) and np.all(a[1][1] == -1)     # patient 9's clean rows; patient 7 has none
        if mode == "int8_exact":
            sa, sb = c.A.certify_stats(), c.B.certify_stats()
            assert sa["queries"] == 3 * sb["queries"] > 0          # A was searched three times per k, B once
            for s in (sa, sb):
                assert s["certified"] + s["fallbacks"] == s["queries"]
                assert np.isfinite(s["R"]) and np.isfinite(s["V"]) and s["R"] >= 0 and s["V"] >= 0
    finally:
        c.A.set_prefilter("off")
        c.B.set_prefilter("off")


@pytest.mark.parametrize("mode", ["off", "bf16", "int8", "int8_exact"])
def test_prefilter_slab_of_40_rows(gpu, slab40, mode):
    c = slab40
    sel, _ = _pick(c, 5, 32)
    q = c.Q[sel]
    qn = c.oracle.normalize_ref(q).astype(np.float32)
    try:
        c.A.set_prefilter(mode)
        c.B.set_prefilter(mode)
        for k in (10, 32):
            a = c.A.search(q, k)
            assert_same(a, c.A.search(q, k), "second call")
            assert_same(a, c.B.search(q, k), "twin")
            assert_same(a, _device_search(gpu, c, c.A, q, k), "device entry point")
            check_topk(a, c.oracle.search(c.xn, qn, k + 1, tags=c.tags_ref), c.all64[sel], k)
            assert np.all((a[1] >= 0).sum(axis=1) == min(k, 28))
    finally:
        c.A.set_prefilter("off")
        c.B.set_prefilter("off")


def test_bf16_index(gpu, oracle):
    """A dtype="bf16" index keeps the NaNs of its rows: the twin bit for bit, and against the oracle every returned row
    scores within the bf16 bound of the reference's k-th (|d score| <= 2 * 2^-9 * |x| |q| = 2^-8 for unit vectors: each
    operand is rounded to 8 significant bits)."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(16)
    n = 1003
    x = rng.standard_normal((n, DIM)).astype(np.float32)
    poison = {0: "nan", n - 1: "inf", 40: "part", 41: "nan"}
    poison.update({r: NF.KINDS[r % 3] for r in range(64, 96)})
    eng = Engine(0, DIM)
    try:
        A, B, xb, tags_ref = NF.build_twin(eng, "nf16", x, None, poison, np.random.default_rng(17), dtype="bf16")
        q = rng.standard_normal((32, DIM)).astype(np.float32)
        a = A.search(q, 10)
        assert_same(a, B.search(q, 10), "twin")
        xn = oracle.normalize_ref(xb).astype(np.float32)
        qn = oracle.normalize_ref(q).astype(np.float32)
        rs, _ = oracle.search(xn, qn, 10, tags=tags_ref)
        all64 = oracle.scores(xn, qn)
        assert np.all(a[1] >= 0) and not np.isin(a[1], sorted(poison)).any()
        got64 = np.take_along_axis(all64, a[1], axis=1)
        assert np.all(np.abs(a[0].astype(np.float64) - got64) <= 2.0 ** -8)
        assert np.all(got64 >= rs[:, 9:10] - 2 * 2.0 ** -8)
    finally:
        eng.close()


# ---- the sample floor, the pair kernel and sample_rep: 40 000 rows --------------------------------------------------------------
@pytest.fixture(scope="module")
def big(gpu, oracle):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(4040)
    n = 40_013
    x = rng.standard_normal((n, DIM)).astype(np.float32)
    poison = {0: "nan", n - 1: "inf", 100: "part", 101: "nan", 16_500: "nan", 20_000: "part", 39_990: "inf"}
    poison.update({r: NF.KINDS[r % 3] for r in range(64, 96)})
    poison.update({r: "nan" for r in range(25_600, 25_632)})
    c = _Case()
    c.eng = Engine(0, DIM)
    c.A, c.B, xb, c.tags_ref = NF.build_twin(c.eng, "nfbig", x, None, poison, np.random.default_rng(4041))
    c.n, c.poison, c.oracle = n, poison, oracle
    c.xn = oracle.normalize_ref(xb).astype(np.float32)
    c.Q = rng.standard_normal((240, DIM)).astype(np.float32)      # a pool: _pick takes the queries without reference near-ties
    c.Q[3] = xb[120] * 3.0
    c.Q[4] = xb[n - 2]
    c.all64 = oracle.scores(c.xn, oracle.normalize_ref(c.Q).astype(np.float32))
    c.picks = {(nq, k): _pick(c, nq, k, must=(3, 4) if k == 10 else ()) for nq, k in ((32, 10), (32, 70), (64, 10), (100, 10))}
    yield c
    c.eng.close()


@pytest.mark.parametrize("k", [10, 70])
def test_sample_floor_off_on_forced(big, k):
    c = big
    sel, _ = c.picks[32, k]
    q, all64 = c.Q[sel], c.all64[sel]
    ref = c.oracle.search(c.xn, c.oracle.normalize_ref(q).astype(np.float32), k + 1, tags=c.tags_ref)
    first = None
    for mode in ("0", "1", "force"):
        with _Env(RASS_SCAN_SAMPLE_FLOOR=mode):
            a = c.A.search(q, k)
            assert_same(a, c.B.search(q, k), "twin, floor " + mode)
        first = a if first is None else first
        assert_same(a, first, "floor " + mode)
    check_topk(first, ref, all64, k)


def _batch(torch, c, ix, q, k):
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(q).to(dev)
    ds = torch.full((q.shape[0], k), 777.0, dtype=torch.float32, device=dev)
    di = torch.full((q.shape[0], k), -777, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ix.search_device_batch(dq.data_ptr(), q.shape[0], k, ds.data_ptr(), di.data_ptr())
    c.eng.synchronize()
    return ds.cpu().numpy(), di.cpu().numpy()


@pytest.mark.parametrize("env", [dict(), dict(RASS_SCAN_SAMPLE_FLOOR="force"), dict(RASS_SCAN_BATCH_SAMPLE="f32"),
                                 dict(RASS_SCAN_SAMPLE_FLOOR="force", RASS_SCAN_BATCH_SAMPLE="f32")])
@pytest.mark.parametrize("nq", [64, 100])
def test_search_device_batch(gpu, big, nq, env):
    c = big
    sel, ref = c.picks[nq, 10]
    q = c.Q[sel]
    with _Env(**env):
        a = _batch(gpu, c, c.A, q, 10)
        assert_same(a, _batch(gpu, c, c.B, q, 10), "twin")
    check_topk(a, ref, c.all64[sel], 10)


# ---- the wide path --------------------------------------------------------------------------------------------------------------
def test_wide_index(gpu, oracle):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(1536)
    n, dim = 2011, 1536
    x = rng.standard_normal((n, dim)).astype(np.float32)
    patient = rng.integers(10, 40, size=n)
    patient[64:96] = 7
    tags = (patient | (rng.integers(1, 4, size=n) << 24)).astype(np.int32)
    keys = rng.integers(0, 30, size=n).astype(np.int32)
    keys[64:96] = 33
    poison = {0: "nan", n - 1: "inf", 100: "part", 101: "nan"}
    poison.update({r: NF.KINDS[r % 3] for r in range(64, 96)})
    eng = Engine(0, dim)
    try:
        A, B, xb, tags_ref = NF.build_twin(eng, "nfwide", x, tags, poison, np.random.default_rng(1537))
        xn = oracle.normalize_ref(xb).astype(np.float32)
        c = _Case()
        c.Q, c.n, c.tags_ref = rng.standard_normal((128, dim)).astype(np.float32), n, tags_ref
        c.all64 = oracle.scores(xn, oracle.normalize_ref(c.Q).astype(np.float32))
        sel, _ = _pick(c, 32, 70, thr=0.05)
        q, all64 = c.Q[sel], c.all64[sel]
        qn = oracle.normalize_ref(q).astype(np.float32)
        for k in (10, 70):
            a = A.search(q, k)
            assert_same(a, B.search(q, k), "twin")
            check_topk(a, oracle.search(xn, qn, k + 1, tags=tags_ref), all64, k)
        a = A.search_grouped(q, 10, PM, 64)
        assert_same(a, B.search_grouped(q, 10, PM, 64), "grouped twin")
        _check_grouped(a, GK.expect_grouped(all64, tags_ref, tags_ref & PM, 64, 10))
        a = A.search_grouped_by_keys(q, 10, keys, 40)
        assert_same(a, B.search_grouped_by_keys(q, 10, keys, 40), "keys twin")
        _check_grouped(a, GK.expect_grouped(all64, tags_ref, keys, 40, 10))
        assert NF.clear_of(0.05, all64, tags_ref)
        a = A.search_counts(q, 0.05, 16, PM, 64)
        assert_same(a, B.search_counts(q, 0.05, 16, PM, 64), "counts twin")
        _check_counts(a, GK.expect_counts(all64, tags_ref, tags_ref & PM, 64, 16, 0.05))
        a = A.search_counts_by_keys(q, NEG, 16, keys, 40)
        assert_same(a, B.search_counts_by_keys(q, NEG, 16, keys, 40), "key counts twin")
        _check_counts(a, GK.expect_counts(all64, tags_ref, keys, 40, 16, NEG))
        a = A.search_range(q, 0.05, max_hits=512)
        assert_same(a, B.search_range(q, 0.05, max_hits=512), "range twin")
        assert np.array_equal(a[2], ((tags_ref != -1) & (all64 >= 0.05)).sum(axis=1))
    finally:
        eng.close()


# ---- IVF ------------------------------------------------------------------------------------------------------------------------
NLIST = 16


@pytest.fixture(scope="module")
def trained(gpu, main):
    from rassengine_amd.ivf import train_centroids
    return train_centroids(main.A, NLIST, iters=6, seed=3)


def test_ivf_training_keeps_every_centroid_finite(gpu, main, trained):
    from rassengine_amd.ivf import train_centroids
    assert bool(gpu.isfinite(trained).all())
    one_level = train_centroids(main.A, NLIST, iters=6, seed=5, fine_factor=1)     # seeds and re-seeds drawn from the rows
    assert bool(gpu.isfinite(one_level).all())
    norms = one_level.norm(dim=1).cpu().numpy()
    assert np.all(np.abs(norms - 1.0) < 1e-4)


@pytest.mark.parametrize("slab", ["f32", "bf16", "int8"])
def test_ivf_every_list_probed(gpu, main, trained, slab):
    from rassengine_amd.ivf import IvfIndex
    c = main
    q = c.Q[:32]
    ia = IvfIndex.build(c.A, nlist=NLIST, centroids=trained, dtype=slab)
    ib = IvfIndex.build(c.B, nlist=NLIST, centroids=trained, dtype=slab)
    try:
        a = ia.search(q, 10, nprobe=NLIST)[:2]
        assert_same(a, ib.search(q, 10, nprobe=NLIST)[:2], "twin")
        assert not np.isin(a[1], sorted(c.poison)).any() and not np.isnan(a[0]).any()
        if slab != "bf16":                 # an f32 slab, and an int8 slab's exact re-rank: the flat index's answer
            assert_same(a, c.B.search(q, 10), "flat")
        f = np.array([9 if r % 2 else 7 for r in range(32)], dtype=np.int32)
        if slab != "bf16":
            af = ia.search_delta(c.A, q, 10, NLIST, f, np.full(32, PM, dtype=np.int32))[:2]
            assert_same(af, c.B.search(q, 10, q_filter=f, q_filter_mask=np.full(32, PM, dtype=np.int32)), "filtered")
        # every live finite row is in exactly one list
        assign, lens = ia.lists_device()
        assign, lens = assign.cpu().numpy(), lens.cpu().numpy()
        assert np.all((assign[c.clean] >= 0) & (assign[c.clean] < NLIST))
        assert int(lens.sum()) == int((assign >= 0).sum()) and np.array_equal(np.bincount(assign[assign >= 0], minlength=NLIST), lens)
    finally:
        ia.close()
        ib.close()


def test_ivf_delta_absorb_and_bitmap(gpu, main, trained):
    """Poisoned rows appended after the build: the delta scan, then absorb (they go to a list by the assign kernel); and the
    probe within a row bitmap — ``search_allowed_delta`` itself, the entry point ``IvfBackedIndex.search_allowed`` routes to
    under ``RASS_IVF_ALLOW=1`` (tests/test_gpu_ivf_allow.py pins that routing)."""
    from rassengine_amd.ivf import IvfIndex
    c = main
    q = c.Q[:32]
    want = c.B.search(q, 10)
    part = IvfIndex.build(c.A, nlist=NLIST, centroids=trained, n_rows=1984)         # rows 2000.. and the last row: the delta
    try:
        assert part.covered_rows == 1984
        assert_same(part.search_delta(c.A, q, 10, NLIST)[:2], want, "delta")
        full = part.absorb(c.A)
        try:
            assert full.covered_rows == c.n
            assert_same(full.search(q, 10, nprobe=NLIST)[:2], want, "absorbed")
            assign, lens = full.lists_device()
            assign = assign.cpu().numpy()
            assert np.all((assign[c.clean] >= 0) & (assign[c.clean] < NLIST)) and int(lens.sum()) == int((assign >= 0).sum())
            for kind in ("mixed", "poisoned", "per_query"):
                words = GK.pack_bits(_allow_bits(c, kind, 32))
                got = full.search_allowed_delta(c.A, q, 10, NLIST, words)[:2]
                assert_same(got, c.B.search_allowed(q, 10, words), "bitmap " + kind)
        finally:
            full.close()
    finally:
        part.close()


# ---- queries that are not finite ------------------------------------------------------------------------------------------------
def _nan_query_case(fn, q, bad, fills):
    """``fn(queries)`` with the queries ``bad`` poisoned: they get the empty answer, every other query the bits it gets
    without them."""
    clean = fn(q)
    got = fn(NF.poison_queries(q, bad))
    good = np.setdiff1d(np.arange(q.shape[0]), bad)
    assert_same(tuple(np.asarray(a)[good] for a in got), tuple(np.asarray(a)[good] for a in clean), "the other queries")
    NF.empty_rows(got, bad, fills)


@pytest.mark.parametrize("nq", [32, 64])
def test_nan_queries_flat_forms(main, nq):
    c = main
    q = c.Q[:nq]
    bad = [0, 17, nq - 1]
    f, m = _filters(c, "masked", nq)
    f[[0, 17, nq - 1]] = -1
    words = GK.pack_bits(_allow_bits(c, "mixed", nq))
    top = (NEG, -1)
    _nan_query_case(lambda v: c.A.search(v, 10), q, bad, top)
    _nan_query_case(lambda v: c.A.search(v, 70, q_filter=f, q_filter_mask=m), q, bad, top)
    _nan_query_case(lambda v: c.A.search_range(v, 0.1, max_hits=64), q, bad, (NEG, -1, 0))
    _nan_query_case(lambda v: c.A.search_range(v, NEG, max_hits=4096), q, bad, (NEG, -1, 0))
    _nan_query_case(lambda v: c.A.search_grouped(v, 10, PM, 64), q, bad, (NEG, -1, -1, 0))
    _nan_query_case(lambda v: c.A.search_grouped_by_keys(v, 10, c.keys, 48, allow=words), q, bad, (NEG, -1, -1, 0))
    _nan_query_case(lambda v: c.A.search_counts(v, NEG, 16, PM, 64), q, bad, (-1, 0, NEG, -1, 0, 0))
    _nan_query_case(lambda v: c.A.search_counts_by_keys(v, 0.1, 16, c.keys, 48), q, bad, (-1, 0, NEG, -1, 0, 0))
    _nan_query_case(lambda v: c.A.search_allowed(v, 10, words), q, bad, top)
    _nan_query_case(lambda v: c.A.search_mmr(v, 8, fetch_k=32), q, bad, (NEG, -1, -1))


@pytest.mark.parametrize("mode", ["bf16", "int8", "int8_exact"])
@pytest.mark.parametrize("nq", [32, 64])
def test_nan_queries_prefilter(main, slab40, nq, mode):
    for c in (main, slab40):
        q = c.Q[:nq]
        try:
            c.A.set_prefilter(mode)
            _nan_query_case(lambda v: c.A.search(v, 10), q, [0, 17, nq - 1], (NEG, -1))
        finally:
            c.A.set_prefilter("off")


@pytest.mark.parametrize("slab", ["f32", "bf16", "int8"])
def test_nan_queries_ivf(gpu, main, trained, slab):
    from rassengine_amd.ivf import IvfIndex
    c = main
    ivf = IvfIndex.build(c.A, nlist=NLIST, centroids=trained, dtype=slab)
    try:
        for nq in (32, 64):
            for nprobe in (4, NLIST):
                _nan_query_case(lambda v: ivf.search(v, 10, nprobe=nprobe)[:2], c.Q[:nq], [0, 17, nq - 1], (NEG, -1))
    finally:
        ivf.close()


def test_nan_queries_device_batch(gpu, big):
    c = big
    for nq in (64, 100):
        _nan_query_case(lambda v: _batch(gpu, c, c.A, v, 10), c.Q[:nq], [0, 17, nq - 1], (NEG, -1))
