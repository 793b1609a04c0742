"""Every flat scan mode at every row-stride class against the oracle.

The scan kernels are compiled once per stride class (CH = stride / 128 up to 1 024 columns, four panel shapes above), query
count class (NT = 1 up to 16 queries, NT = 2 up to 32; wide rows split 17..32 into two launches), mode and filter form (EXT:
masked filters / the continuation bound).  The files of the single modes run a few strides each; this file runs every mode
at one dim per stride class, half of them ending inside a padded stride:

    100 (128), 200 (256), 384, 500 (512), 640, 700 (768), 896, 1024 | 1100 (1280), 1536, 1700 (1792), 2048

One corpus per dim: 8 229 iid unit rows = 257 tiles of 32 and a ragged tile of 5 (256 persistent workgroups: one of them
walks two tiles), ``patient | doc_type << 24`` tags, a key column, tombstones at row 0, at the last row of a full tile and
inside the ragged tile.  Queries come from a seeded pool of 96; a case takes the first of them whose fp64 reference scores
among the top k + 1 are pairwise more than 2 tolerances apart (``nonfinite_ref.no_near_ties``), so ids are compared for
EQUALITY, and at least 33 must survive, which is asserted before anything is searched.  Query counts 16, 17, 32 and 33.

References.  top-k: the fp64 oracle (ids equal, scores within TOL_F64 / TOL_F64_WIDE of test_gpu_scan.py), and the emulation
of the kernel's fmaf order bit for bit.  range / group-max / group-count / key columns / continuation bound: the numpy
restatements of test_gpu_range_search.py, test_gpu_group_search.py, test_gpu_aggregate.py, test_gpu_group_by_keys.py
(groupkeys_ref.py) and test_gpu_search_after.py, everything EQUAL; score thresholds lie midway between two adjacent fp64
reference scores more than 4 tolerances apart, so the hit set does not depend on the kernel's rounding.  allow bitmaps:
the same ranking restricted to the set bits.  cross-index batch: bit-identical to each index's own ``search``.

The sample-floor pass of a flat scan (kFlatSample, plain and EXT) needs 32 768 rows before it runs at all: it has a corpus of
its own, 33 000 rows per narrow dim, in ``test_sample_floor_pass``.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_aggregate as AGG
import test_gpu_group_by_keys as GK
import test_gpu_group_search as GRP
import test_gpu_range_search as RS
import test_gpu_search_after as AFT
from nonfinite_ref import no_near_ties
from test_gpu_scan import TOL_F64, TOL_F64_WIDE

pytestmark = pytest.mark.gpu

NARROW = (100, 200, 384, 500, 640, 700, 896, 1024)
WIDE = (1100, 1536, 1700, 2048)
N = 257 * 32 + 5
DEAD = (0, 255 * 32 + 31, 257 * 32 + 2)      # row 0, the last row of a full tile, inside the ragged tile
POOL = 96
MIN_SURVIVORS = 33
NQS = (16, 17, 32, 33)
N_PATIENTS, N_KEYS = 40, 37
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
UNSUPPORTED = -5                              # RASS_ERR_UNSUPPORTED
NEG_INF = np.float32(-np.inf)

FLAT = ("topk", "after", "range", "group_max", "group_count", "keys")
CASES = [(d, f) for d in NARROW for f in FLAT + ("allow", "keys_allow", "multi")] + \
        [(d, f) for d in WIDE for f in FLAT + ("refused",)]


class World:
    """Rows, tags, keys, the query pool and both score matrices (fp64 truth, the emulation of the kernel's order) of one
    dim, with the live index.  Nothing here is changed by a test."""

    def __init__(self, torch, oracle, dim):
        from rassengine_amd.engine import Engine
        self.torch, self.oracle, self.dim = torch, oracle, dim
        self.tol = TOL_F64 if dim <= 1024 else TOL_F64_WIDE
        rng = np.random.default_rng(31000 + dim)
        tags = (rng.integers(0, N_PATIENTS, size=N) | (rng.integers(1, 3, size=N) << DSHIFT)).astype(np.int32)
        self.keys = rng.integers(0, N_KEYS, size=N).astype(np.int32)
        self.keys[rng.random(N) < 0.1] = -1                                  # ~10 % of the rows have no group
        self.pool = RS.Corpus(torch, oracle, N, dim, POOL, seed=32000 + dim)  # iid unit rows, un-normalised queries
        self.xn, self.q_raw, self.s32 = self.pool.xn, self.pool.q_raw, self.pool.scores
        self.qn64 = oracle.normalize_c(self.q_raw)
        self.all64 = oracle.scores(self.xn, self.qn64, kind=oracle.KIND_F64)
        assert np.abs(self.all64 - self.s32).max() <= self.tol               # the two references agree with each other
        self.bits = rng.random((POOL, N)) < 0.3
        self.tags = tags.copy()
        self.tags[list(DEAD)] = -1
        self.pool.tags = self.tags
        plain, filt, mask = AFT.mixed_filters(POOL)
        # the exact-tag values of mixed_filters name patients 0..5: every one of them has rows here too
        self.forms = {"none": (None, None), "plain": (plain, None), "masked": (filt, mask)}
        self._ranked, self._surv, self._thr = {}, {}, {}
        for k in (1, 10, 32, 40):       # the cap: at least 33 of the 96 survive at every k, before anything is searched
            self.survivors(k)
        self.eng = Engine(0, dim)
        self.idx = self.eng.open_index("matrix")
        assert self.idx.add(self.xn, tags=tags, normalize=False) == 0
        for r in DEAD:
            self.idx.delete(r)

    def close(self):
        self.eng.close()

    def match(self, q, form, allow=None):
        f, m = self.forms[form]
        ok = self.tags != -1
        if f is not None and f[q] >= 0:
            ok = ok & (((self.tags & m[q]) if m is not None else self.tags) == f[q])
        if allow is not None:
            ok = ok & allow[q]
        return ok

    def ranked(self, form):
        """Per pool query (scores f32, rows) of every matching row in the kernel's order, score desc, row asc."""
        if form not in self._ranked:
            f, m = self.forms[form]
            self._ranked[form] = self.pool.ranked(qfilter=f, qmask=m, check=form == "none")
        return self._ranked[form]

    def top64(self, q, k, form, allow=None):
        """(scores f64 [k], rows [k]) of pool query q's fp64 ranking over its matching rows, (-inf, -1) padding."""
        rows = np.flatnonzero(self.match(q, form, allow))
        s = self.all64[q, rows]
        order = np.lexsort((rows, -s))[:k]
        rs, ri = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
        rs[:len(order)], ri[:len(order)] = s[order], rows[order]
        return rs, ri

    def survivors(self, k, form="none", allow=None):
        """The pool queries whose fp64 reference scores among the top k + 1 are pairwise more than 2 tol apart."""
        key = (k, form, allow is not None)
        if key not in self._surv:
            keep = [q for q in range(POOL) if no_near_ties(self.top64(q, k + 1, form, allow)[0][None], self.tol)]
            assert len(keep) >= MIN_SURVIVORS, (self.dim, key, len(keep))
            self._surv[key] = np.array(keep)
        return self._surv[key]

    def thresholds(self, form):
        """One threshold per pool query: midway between two adjacent fp64 scores of its matching rows that are more than 4
        tol apart, the first such pair at or behind rank (37 q + 5) % 200; +inf for a query without such a pair."""
        if form not in self._thr:
            thr = np.full(POOL, np.inf, dtype=np.float32)
            for q in range(POOL):
                rows = np.flatnonzero(self.match(q, form))
                s = -np.sort(-self.all64[q, rows])
                if len(s) < 2:
                    continue
                wide = np.flatnonzero(s[:-1] - s[1:] > 4 * self.tol)
                wide = wide[wide >= (37 * q + 5) % min(len(s) - 1, 200)]
                if len(wide):
                    j = int(wide[0])
                    thr[q] = np.float32((s[j] + s[j + 1]) / 2)
                    assert s[j] - thr[q] > self.tol and thr[q] - s[j + 1] > self.tol
                    assert np.count_nonzero(self.s32[q, rows] >= thr[q]) == j + 1      # both references cut at the same row
            assert np.isfinite(thr).sum() >= POOL - 20
            self._thr[form] = thr
        return self._thr[form]

    def case(self, sel):
        """What the helpers of the single-mode files read off their Corpus, for the pool queries ``sel``."""
        return SimpleNamespace(n=N, dim=self.dim, nq=len(sel), q_raw=np.ascontiguousarray(self.q_raw[sel]),
                               scores=self.s32[sel])

    def filters(self, form, sel):
        f, m = self.forms[form]
        return (None if f is None else f[sel]), (None if m is None else m[sel])

    def check_topk(self, got, sel, k, form="none", allow=None, what=""):
        """ids equal to the fp64 ranking, scores within tol of it; ids and scores equal to the kernel-order ranking."""
        s, i = got
        ref = [self.top64(q, k + 1, form, allow) for q in sel]
        rs, ri = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        assert no_near_ties(rs, self.tol), what
        if allow is None:      # the numpy ranking above IS oracle.search's
            f, m = self.filters(form, sel)
            o_s, o_i = self.oracle.search(self.xn, self.qn64[sel], k + 1, tags=self.tags, qfilter=f, qmask=m,
                                          kind=self.oracle.KIND_F64)
            assert np.array_equal(o_i, ri) and np.array_equal(o_s, rs), what
        rs, ri = rs[:, :k], ri[:, :k]
        assert np.array_equal(i, ri), (what, np.argwhere(i != ri)[:5].tolist())
        ok = ri >= 0
        assert np.all(np.abs(s[ok].astype(np.float64) - rs[ok]) <= self.tol), (what, np.abs(s[ok] - rs[ok]).max())
        assert np.all(np.isneginf(s[~ok])), what
        exact = np.full((len(sel), k), NEG_INF, dtype=np.float32)
        for j, q in enumerate(sel):
            exact[j, ok[j]] = self.s32[q, ri[j, ok[j]]]
        assert np.array_equal(s.view(np.uint32), exact.view(np.uint32)), what


@pytest.fixture(scope="module")
def worlds(gpu, oracle):
    """dim -> World, one at a time: the cases of a dim are adjacent, so each world is built once."""
    cur = {}

    def get(dim):
        if cur.get("dim") != dim:
            if "w" in cur:
                cur.pop("w").close()
            cur["dim"], cur["w"] = dim, World(gpu, oracle, dim)
        return cur["w"]

    yield get
    if "w" in cur:
        cur["w"].close()


def _topk(w):
    for k in (1, 10, 32):
        keep = w.survivors(k)
        for nq in NQS:
            sel = keep[:nq]
            w.check_topk(w.idx.search(w.q_raw[sel], k), sel, k, what=f"k {k} nq {nq}")
    sel = w.survivors(40)[:33]
    w.check_topk(w.idx.search(w.q_raw[sel], 40), sel, 40, what="k 40: two passes")
    for form in ("plain", "masked"):
        keep = w.survivors(10, form)
        for nq in NQS:
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            w.check_topk(w.idx.search(w.q_raw[sel], 10, q_filter=f, q_filter_mask=m), sel, 10, form, what=f"{form} nq {nq}")


def _after(w):
    """search_device_after through two pages of 10: page 2's bound is the reference's row at rank 9, never the GPU's."""
    k = 10
    for form in ("none", "masked"):
        keep = w.survivors(2 * k, form)
        ranked = w.ranked(form)
        for nq in (16, 17, 32):
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            dev = AFT.Device(w.torch, w.idx, w.q_raw[sel], f, m)
            rk = [ranked[q] for q in sel]
            first = (np.full(nq, np.inf, dtype=np.float32), np.full(nq, -1, dtype=np.int64))
            for page, (a_s, a_r) in enumerate((first, AFT.bounds_at(rk, lambda q, n_: k - 1))):
                want = AFT.expect(rk, a_s, a_r, k)
                for j, (s, rows) in enumerate(rk):               # the cut IS the ranking's slice
                    assert np.array_equal(want[1][j, :len(rows[page * k:(page + 1) * k])], rows[page * k:(page + 1) * k])
                AFT.assert_same(dev.after(a_s, a_r, k), want, f"{form} nq {nq} page {page}")
                ids64 = np.stack([w.top64(q, 2 * k, form)[1][page * k:(page + 1) * k] for q in sel])
                assert np.array_equal(want[1], ids64)             # ... and the fp64 ranking's


def _range(w):
    for form in ("plain", "masked"):
        keep, ranked, thr = w.survivors(32, form), w.ranked(form), w.thresholds(form)
        for nq in NQS:
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            RS.check_both(w.torch, w.idx, w.case(sel), [ranked[q] for q in sel], thr[sel], 256, f, m, what=f"{form} nq {nq}")


def _group_max(w):
    for form in ("plain", "masked"):
        keep = w.survivors(32, form)
        for nq in NQS:
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            for k in (10, 64):                                    # 64: more than the 40 groups there are
                GRP.check_both(w.torch, w.idx, w.case(sel), w.tags, PMASK, N_PATIENTS, k, f, m, what=f"{form} nq {nq} k {k}")
        sel = keep[:17]
        f, m = w.filters(form, sel)
        GRP.check_both(w.torch, w.idx, w.case(sel), w.tags, DMASK, 3, 5, f, m, what=f"{form} by doc_type")


def _group_count(w):
    for form in ("plain", "masked"):
        keep, thr = w.survivors(32, form), w.thresholds(form)
        for nq in NQS:
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            for size in (10, 64):
                AGG.check_both(w.torch, w.idx, w.case(sel), w.tags, PMASK, N_PATIENTS, size, thr[sel], f, m,
                               what=f"{form} nq {nq} size {size}")
        sel = keep[:17]
        f, m = w.filters(form, sel)
        AGG.check_both(w.torch, w.idx, w.case(sel), w.tags, DMASK, 3, 5, thr[sel], f, m, what=f"{form} by doc_type")


def _keys(w, allow=False):
    for form in ("none", "masked"):
        keep, thr = w.survivors(32, form), w.thresholds(form)
        for nq in NQS:
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            GK.check(w.torch, w.idx, w.case(sel), w.tags, w.keys, N_KEYS, 10, thr[sel], w.bits[sel] if allow else None, f, m,
                     what=f"{form} nq {nq} allow {allow}")


def _allow(w):
    from rassengine_amd.engine import pack_allow
    for form in ("none", "masked"):
        for k, nqs in ((10, NQS), (40, (17,))):                   # 40: a second pass under the continuation bound
            keep = w.survivors(k, form, w.bits)
            for nq in nqs:
                sel = keep[:nq]
                f, m = w.filters(form, sel)
                words = pack_allow(w.bits[sel])
                got = w.idx.search_allowed(w.q_raw[sel], k, words, q_filter=f, q_filter_mask=m)
                w.check_topk(got, sel, k, form, allow=w.bits, what=f"{form} nq {nq} k {k}")
                d_words = w.torch.from_numpy(words.view(np.int32)).cuda()
                dev = w.idx.search_allowed(w.q_raw[sel], k, d_words, q_filter=f, q_filter_mask=m)
                assert np.array_equal(dev[1], got[1]) and np.array_equal(dev[0].view(np.uint32), got[0].view(np.uint32))


def _multi(w):
    """Three indices of 0, 33 and 8 229 rows in one cross-index batch."""
    empty = w.eng.open_index("matrix-empty")
    small = w.eng.open_index("matrix-33")
    if small.rows == 0:
        small.add(w.xn[:33], tags=np.where(w.tags[:33] == -1, 0, w.tags[:33]), normalize=False)
        small.delete(0)                                              # row 0 is a tombstone here as in the large index
    three = (w.idx, small, empty)
    for form in ("none", "masked"):
        keep = w.survivors(10, form)
        for nq in (16, 32):
            sel = keep[:nq]
            f, m = w.filters(form, sel)
            who = [(0, 1, 0, 2, 0, 0, 1)[j % 7] for j in range(nq)]
            s, i = w.eng.search_multi([three[u] for u in who], w.q_raw[sel], 10, f, m)
            for j, u in enumerate(who):
                s1, i1 = three[u].search(w.q_raw[sel[j]:sel[j] + 1], 10, None if f is None else f[j:j + 1],
                                         None if m is None else m[j:j + 1])
                assert np.array_equal(i[j], i1[0]) and np.array_equal(s[j].view(np.uint32), s1[0].view(np.uint32)), (form, nq, j, u)
                if u == 2:
                    assert np.all(i[j] == -1) and np.all(np.isneginf(s[j]))
            on_main = np.array([j for j, u in enumerate(who) if u == 0])
            w.check_topk((s[on_main], i[on_main]), sel[on_main], 10, form, what=f"multi {form} nq {nq}")


def _refused(w):
    """Wide rows have no allow-bitmap and no cross-index form: the documented RASS_ERR_UNSUPPORTED, never a wrong answer."""
    from rassengine_amd._native import RassError
    from rassengine_amd.engine import pack_allow
    with pytest.raises(RassError) as e:
        w.idx.search_allowed(w.q_raw[:2], 5, pack_allow(w.bits[:2]))
    assert e.value.code == UNSUPPORTED
    with pytest.raises(RassError) as e:
        w.eng.search_multi([w.idx], w.q_raw[:1], 3)
    assert e.value.code == UNSUPPORTED


class _Env:
    """An environment variable for the length of a block (the library reads RASS_SCAN_SAMPLE_FLOOR at every call)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        import os
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        import os
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


SAMPLE_N = 33_000           # >= 2 x 64 rows x 256 workgroups, the size at which "force" samples; 1 031 tiles and one of 8
SAMPLE_POOL = POOL


@pytest.mark.parametrize("dim", NARROW)
def test_sample_floor_pass(gpu, oracle, dim):
    """The score-floor sample pass of a flat scan with more than 16 queries (the kFlatSample kernels, plain and EXT) at every
    narrow stride: 33 000 rows under RASS_SCAN_SAMPLE_FLOOR=force, 17 and 32 queries, no filter, masked filters, and k = 40
    (the second pass samples under its continuation bound).  ids equal to the fp64 ranking, scores within TOL_F64 of it, and
    the answer bit-identical to the one without the floor."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(33000 + dim)
    xn = oracle.normalize_ref(rng.standard_normal((SAMPLE_N, dim), dtype=np.float32)).astype(np.float32)
    q_raw = rng.standard_normal((SAMPLE_POOL, dim), dtype=np.float32) * 3.0
    tags = (rng.integers(0, N_PATIENTS, size=SAMPLE_N) | (rng.integers(1, 3, size=SAMPLE_N) << DSHIFT)).astype(np.int32)
    dead = (0, 31, SAMPLE_N - 3)
    all64 = oracle.scores(xn, oracle.normalize_c(q_raw), kind=oracle.KIND_F64)
    _, filt, mask = AFT.mixed_filters(SAMPLE_POOL)
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("matrix-sample")
        idx.add(xn, tags=tags, normalize=False)
        for r in dead:
            idx.delete(r)
        tags[list(dead)] = -1
        for k, f, m in ((10, None, None), (10, filt, mask), (40, None, None)):
            ref = []
            for q in range(SAMPLE_POOL):
                ok = tags != -1
                if f is not None and f[q] >= 0:
                    ok &= (tags & m[q]) == f[q]
                rows = np.flatnonzero(ok)
                order = np.lexsort((rows, -all64[q, rows]))[:k + 1]
                rs, ri = np.full(k + 1, -np.inf), np.full(k + 1, -1, dtype=np.int64)
                rs[:len(order)], ri[:len(order)] = all64[q, rows[order]], rows[order]
                ref.append((rs, ri))
            keep = np.array([q for q in range(SAMPLE_POOL) if no_near_ties(ref[q][0][None], TOL_F64)])
            assert len(keep) >= MIN_SURVIVORS, (dim, k, len(keep))
            for nq in (17, 32):
                sel = keep[:nq]
                fs, ms = (None, None) if f is None else (f[sel], m[sel])
                with _Env("RASS_SCAN_SAMPLE_FLOOR", "force"):
                    s, i = idx.search(q_raw[sel], k, q_filter=fs, q_filter_mask=ms)
                with _Env("RASS_SCAN_SAMPLE_FLOOR", "0"):
                    s0, i0 = idx.search(q_raw[sel], k, q_filter=fs, q_filter_mask=ms)
                rs = np.stack([ref[q][0][:k] for q in sel])
                ri = np.stack([ref[q][1][:k] for q in sel])
                assert np.array_equal(i, ri), (k, f is not None, nq, np.argwhere(i != ri)[:5].tolist())
                ok = ri >= 0
                assert np.all(np.abs(s[ok].astype(np.float64) - rs[ok]) <= TOL_F64) and np.all(np.isneginf(s[~ok]))
                assert np.array_equal(i, i0) and np.array_equal(s.view(np.uint32), s0.view(np.uint32))
    finally:
        eng.close()


RUN = {"topk": _topk, "after": _after, "range": _range, "group_max": _group_max, "group_count": _group_count, "keys": _keys,
       "keys_allow": lambda w: _keys(w, allow=True), "allow": _allow, "multi": _multi, "refused": _refused}


@pytest.mark.parametrize("dim,family", CASES, ids=[f"{d}-{f}" for d, f in CASES])
def test_matrix(worlds, dim, family):
    RUN[family](worlds(dim))
