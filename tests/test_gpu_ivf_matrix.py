"""The IVF fine scans at every narrow stride class and slab dtype, exact, over hard list geometry.

Every other IVF test runs dim 1024 (test_gpu_ivf_absorb.py adds 256) with trained lists of a few hundred rows.  Here the
fine scans (the fp32 ``kIvf`` / ``kIvfGroups`` forms, the bf16 and int8 IVF forms, their masked EXT forms behind
``search_delta``) run at one dim per stride class

    100 (128), 200 (256), 384, 500 (512), 640, 700 (768), 896, 1024

with an fp32 slab and an int8 slab at all eight (dim 384: fp32 stride 384 against int8 stride 512) and a bf16 slab where the
stride is a whole number of 256-column units (200, 500, 700, 1024).

The IVF is built from the CALLER's centroids (24 random unit vectors) and the CALLER's assignment, so the slab's list
lengths are exactly

    0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 200, 500, then 120 .. 410 for the other ten

over 4 000 covered source rows with the rows of a list interleaved in source order, 8 rows tombstoned before the build (they
never enter the slab), 5 rows deleted after it (they keep their slot, skipped by tag), and a 45-row delta behind the covered
rows.  A query is ``c_a + 0.6 c_b + 0.3 c_c + noise``; only queries whose fp64 coarse ranking has a gap above 1e-3 at the
nprobe boundary are used, so ``probe_lists`` must EQUAL the fp64 ranking, and the fine result must equal the oracle's brute
force over the live rows of exactly those lists: ids equal (queries are taken free of near-ties within the restricted set, as
in test_gpu_scan_matrix.py), scores within TOL_F64 of fp64 — for a bf16 slab over the bf16-rounded operands, the rule of
test_gpu_ivf_bf16.py; an int8 slab must return the fp32 IVF's answer bit for bit (k <= 16), as test_gpu_ivf_int8.py asserts
at 1024.  ``scanned`` is the slab length of the union of each 32-query group's probed lists, plus the delta where there is one.
"""
import numpy as np
import pytest

from nonfinite_ref import no_near_ties
from test_gpu_scan import TOL_F64

pytestmark = pytest.mark.gpu

DIMS = (100, 200, 384, 500, 640, 700, 896, 1024)
BF16_DIMS = (200, 500, 700, 1024)
NLIST = 24
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 200, 500, 120, 180, 240, 300, 330, 350, 370, 390, 410, 265)
L_EMPTY, L_ONE, L_33, L_500 = 0, 1, 7, 13
PRE_DEAD_LISTS = (0, 1, 7, 7, 11, 13, 20, 23)      # the lists 8 tombstoned-before-the-build rows were assigned to
POST_DEAD_LISTS = (4, 7, 12, 13, 13)               # one row of each is deleted after the build
COVERED, DELTA = 4000, 45
PER_LIST = 10                                      # candidate queries aimed at each list
COARSE_GAP = 1e-3
PMASK, DMASK, DSHIFT = 0x00FFFFFF, 0x7F000000, 24
CASES = [(d, s, c) for d in DIMS for s in ("f32", "bf16", "int8") if s != "bf16" or d in BF16_DIMS
         for c in ("lists", "entries", "filters")]
assert sum(LENS) + len(PRE_DEAD_LISTS) == COVERED and COVERED % 32 == 0 and len(LENS) == NLIST


def _bf16_round(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


class World:
    def __init__(self, torch, oracle, dim):
        from rassengine_amd import ops
        from rassengine_amd.engine import Engine
        self.torch, self.oracle, self.dim = torch, oracle, dim
        rng = np.random.default_rng(41000 + dim)
        cent = rng.standard_normal((NLIST, dim))
        self.cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float32)
        # the assignment: LENS[l] live rows of list l and the rows that die before the build, shuffled into source order
        labels = np.concatenate([np.repeat(np.arange(NLIST), LENS), np.array(PRE_DEAD_LISTS)])
        dead = np.concatenate([np.zeros(sum(LENS), dtype=bool), np.ones(len(PRE_DEAD_LISTS), dtype=bool)])
        perm = rng.permutation(COVERED)
        self.assign = labels[perm].astype(np.int32)
        self.pre_dead = np.flatnonzero(dead[perm])
        n = COVERED + DELTA
        home = np.concatenate([self.assign, rng.integers(0, NLIST, size=DELTA)])
        x = self.cent[home] + rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
        self.xn = oracle.normalize_ref(x).astype(np.float32)
        tags = (rng.integers(0, 6, size=n) | (rng.integers(1, 3, size=n) << DSHIFT)).astype(np.int32)
        self.slab_len = np.bincount(self.assign[~dead[perm]], minlength=NLIST)      # rows that entered the slab, per list
        assert tuple(self.slab_len) == LENS
        self.post_dead = np.array([np.flatnonzero((self.assign == l) & ~dead[perm])[j] for j, l in enumerate(POST_DEAD_LISTS)])
        assert len(set(self.post_dead.tolist())) == len(POST_DEAD_LISTS)

        # queries aimed at every list: a is the best list by construction, b and c the next two
        a = np.repeat(np.arange(NLIST), PER_LIST)
        b = (a + 1 + rng.integers(0, NLIST - 1, size=len(a))) % NLIST
        c = rng.integers(0, NLIST, size=len(a))
        c = np.where((c == a) | (c == b), (np.maximum(a, b) + 1) % NLIST, c)
        c = np.where((c == a) | (c == b), (c + 1) % NLIST, c)
        self.aim = a
        self.q_raw = (self.cent[a] + 0.6 * self.cent[b] + 0.3 * self.cent[c]
                      + 0.05 * rng.standard_normal((len(a), dim)).astype(np.float32) / np.float32(np.sqrt(dim))).astype(np.float32)
        self.q_raw *= 2.5                                                            # un-normalised on purpose
        qn64 = oracle.normalize_c(self.q_raw)
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        coarse = oracle.scores(oracle.normalize_ref(self.cent).astype(np.float32), qn64, kind=oracle.KIND_F64)
        self.order = np.argsort(-coarse, axis=1, kind="stable")
        ranked = np.take_along_axis(coarse, self.order, axis=1)
        self.coarse_gap = ranked[:, :-1] - ranked[:, 1:]                             # [q, j]: between ranks j and j + 1

        # reference scores [q, n]: fp64 over the fp32 operands; for a bf16 slab the covered rows over the bf16-rounded operands
        f32 = oracle.scores(self.xn, qn64, kind=oracle.KIND_F64)
        b16 = f32.copy()
        b16[:, :COVERED] = oracle.scores(_bf16_round(self.xn[:COVERED]), _bf16_round(self.qn_gpu), kind=oracle.KIND_F64)
        self.ref = {"f32": f32, "bf16": b16}

        self.eng = Engine(0, dim)
        self.flat = self.eng.open_index("ivfm-src")            # covered rows + the delta
        self.flat0 = self.eng.open_index("ivfm-covered")       # the covered rows alone: what nprobe = nlist must reproduce
        self.flat.add(self.xn, tags=tags, normalize=False)
        self.flat0.add(self.xn[:COVERED], tags=tags[:COVERED], normalize=False)
        for r in self.pre_dead:
            self.flat.delete(int(r))
            self.flat0.delete(int(r))
        self.tags = tags.copy()
        self.tags[self.pre_dead] = -1
        self.tags[self.post_dead] = -1
        # every slab of this dim is built before the later deletes, so that those rows keep their slots in each of them
        from rassengine_amd.ivf import IvfIndex
        self.ivfs = {}
        cent = torch.from_numpy(self.cent).cuda()
        for slab in ("f32", "int8") + (("bf16",) if dim in BF16_DIMS else ()):
            ivf = IvfIndex.build(self.flat, nlist=NLIST, centroids=cent, dtype=slab, assign=self.assign, n_rows=COVERED)
            assert ivf.dtype == slab and ivf.nlist == NLIST and ivf.covered_rows == COVERED and ivf.rows == sum(LENS)
            self.ivfs[slab] = ivf
        for r in self.post_dead:
            self.flat.delete(int(r))
            self.flat0.delete(int(r))
            for ivf in self.ivfs.values():
                ivf.delete(int(r))

    def ivf(self, slab):
        return self.ivfs[slab]

    def close(self):
        for ivf in self.ivfs.values():
            ivf.close()
        self.eng.close()

    # ---- the reference
    def lists(self, q, nprobe):
        return self.order[q, :nprobe]

    def member(self, q, nprobe, qfilter=None, qmask=None, delta=False):
        ok = self.tags != -1
        inside = np.zeros(len(self.tags), dtype=bool)
        inside[:COVERED] = np.isin(self.assign, self.lists(q, nprobe))
        if delta:
            inside[COVERED:] = True
        ok &= inside
        if qfilter is not None and qfilter >= 0:
            ok &= ((self.tags & qmask) if qmask is not None else self.tags) == qfilter
        return np.flatnonzero(ok)

    def top(self, slab, q, k, nprobe, qfilter=None, qmask=None, delta=False):
        rows = self.member(q, nprobe, qfilter, qmask, delta)
        s = self.ref["bf16" if slab == "bf16" else "f32"][q, rows]
        order = np.lexsort((rows, -s))[:k]
        rs, ri = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
        rs[:len(order)], ri[:len(order)] = s[order], rows[order]
        return rs, ri

    def pick(self, slab, aims, k, nprobe, flt=None, delta=False):
        """One query per entry of ``aims`` (the list it must rank first; None = any): the first unused candidates whose
        coarse gaps at the boundaries of ``nprobe`` exceed COARSE_GAP and whose restricted reference is free of near-ties."""
        out, used = [], set()
        for j, aim in enumerate(aims):
            cands = range(len(self.aim)) if aim is None else np.flatnonzero(self.aim == aim)
            for q in cands:
                q = int(q)
                if q in used or (aim is not None and self.order[q, 0] != aim):
                    continue
                if nprobe < NLIST and self.coarse_gap[q, nprobe - 1] <= COARSE_GAP:
                    continue
                f, m = (None, None) if flt is None else flt(j)
                if no_near_ties(self.top(slab, q, k + 1, nprobe, f, m, delta)[0][None], TOL_F64):
                    out.append(q)
                    used.add(q)
                    break
            else:
                raise AssertionError(f"no candidate query for list {aim} (dim {self.dim}, nprobe {nprobe}, k {k})")
        return np.array(out)

    def scanned(self, qs, nprobe, delta=False):
        total = 0
        for g0 in range(0, len(qs), 32):
            union = np.unique(np.concatenate([self.lists(q, nprobe) for q in qs[g0:g0 + 32]]))
            total += int(self.slab_len[union].sum()) + (DELTA if delta else 0)
        return total

    # ---- the entry points: (scores, ids, scanned or None)
    def run(self, ivf, via, qs, k, nprobe, qfilter=None):
        torch = self.torch
        q = np.ascontiguousarray(self.q_raw[qs])
        if via == "host":
            return ivf.search(q, k, nprobe, q_filter=qfilter)
        nq = len(qs)
        dq = torch.from_numpy(q).cuda()
        df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter, dtype=np.int32)).cuda()
        os_ = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        oi = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        sc = torch.zeros(((nq + 31) // 32,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                       # the engine works on its own stream
        if via == "batch":
            ivf.search_device_batch(dq.data_ptr(), nq, k, nprobe, os_.data_ptr(), oi.data_ptr(), 0 if df is None else df.data_ptr(),
                                    sc.data_ptr())
        else:
            for g0 in range(0, nq, 32):
                g = min(32, nq - g0)
                ivf.search_device(dq[g0:g0 + g].data_ptr(), g, k, nprobe, os_[g0:g0 + g].data_ptr(), oi[g0:g0 + g].data_ptr(),
                                  0 if df is None else df[g0:g0 + g].data_ptr())
        self.eng.synchronize()
        return os_.cpu().numpy(), oi.cpu().numpy(), int(sc.sum().item()) if via == "batch" else None

    def check(self, slab, got, qs, k, nprobe, qfilter=None, qmask=None, delta=False, what=""):
        """The answer against the brute force over the live rows of exactly the probed lists (+ the delta)."""
        s, i, scanned = got
        assert s.shape == (len(qs), k) and i.shape == (len(qs), k), what
        if scanned is not None:
            assert scanned == self.scanned(qs, nprobe, delta), (what, scanned, self.scanned(qs, nprobe, delta))
        if slab == "int8":
            return                                      # held to the fp32 IVF bit for bit by the caller
        for j, q in enumerate(qs):
            f = None if qfilter is None else int(qfilter[j])
            m = None if qmask is None else int(qmask[j])
            rs, ri = self.top(slab, q, k + 1, nprobe, f, m, delta)
            assert no_near_ties(rs[None], TOL_F64), (what, j)
            rs, ri = rs[:k], ri[:k]
            assert np.array_equal(i[j], ri), (what, j, int(q), i[j].tolist(), ri.tolist())
            ok = ri >= 0
            assert np.all(np.abs(s[j][ok].astype(np.float64) - rs[ok]) <= TOL_F64), (what, j, np.abs(s[j][ok] - rs[ok]).max())
            assert np.all(np.isneginf(s[j][~ok])), (what, j)


def same(a, b, what):
    for u, v, name in zip(a, b, ("scores", "ids", "scanned")):
        if u is None or v is None:
            continue
        u, v = np.asarray(u), np.asarray(v)
        assert np.array_equal(_bits(u), _bits(v)), (what, name, np.argwhere(_bits(u) != _bits(v))[:5].tolist())


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


def _search(w, slab, qs, k, nprobe, what, via="host", qfilter=None):
    """One search, the probed lists first; an int8 slab is held to the fp32 IVF over the same lists bit for bit."""
    ivf = w.ivf(slab)
    want_lists = np.stack([w.lists(q, nprobe) for q in qs])
    assert np.array_equal(ivf.probe_lists(w.q_raw[qs], nprobe), want_lists), what       # the fp64 coarse ranking, exactly
    got = w.run(ivf, via, qs, k, nprobe, qfilter)
    w.check(slab, got, qs, k, nprobe, qfilter, what=what)
    if slab == "int8":
        same(got, w.run(w.ivf("f32"), via, qs, k, nprobe, qfilter), what + " int8 vs fp32 IVF")
    return got


def _lists(w, slab):
    k = 10
    # nprobe 1 at the empty lists: nothing to return, nothing scanned
    qs = w.pick(slab, [L_EMPTY, 11, L_EMPTY], k, 1)
    s, i, scanned = _search(w, slab, qs, k, 1, "empty list")
    assert np.all(i == -1) and np.all(np.isneginf(s)) and scanned == 0
    # ... at the 1-row list: one hit, then padding
    qs = w.pick(slab, [L_ONE], k, 1)
    s, i, scanned = _search(w, slab, qs, k, 1, "1-row list")
    assert i[0, 0] >= 0 and w.assign[i[0, 0]] == L_ONE and np.all(i[0, 1:] == -1) and scanned == 1
    # ... at the 33-row list (a full tile and one row; one of its rows deleted after the build)
    qs = w.pick(slab, [L_33, L_33], k, 1)
    s, i, scanned = _search(w, slab, qs, k, 1, "33-row list")
    assert np.all(w.assign[i.reshape(-1)] == L_33) and scanned == 33
    # ... at every short list in one call, k = 16: every one of them has fewer than k + 1 live rows or just above
    qs = w.pick(slab, [2, 3, 4, 5, 6, 7, 8, 9, 10], 16, 1)
    _search(w, slab, qs, 16, 1, "lists of 15 .. 65 rows, k 16")
    # nprobe 3
    qs = w.pick(slab, [None] * 20, k, 3)
    _search(w, slab, qs, k, 3, "nprobe 3")
    # 32 queries that all probe the same single list
    qs = np.resize(w.pick(slab, [L_500] * 6, k, 1), 32)            # six queries, repeated: all 32 bits of one work mask
    _, _, scanned = _search(w, slab, qs, k, 1, "32 queries, one list")
    assert scanned == 500
    # 32 queries whose best lists are 24 different ones: single-bit work masks
    qs = w.pick(slab, [j % NLIST for j in range(32)], k, 1)
    _, _, scanned = _search(w, slab, qs, k, 1, "32 queries, 24 lists")
    assert scanned == sum(LENS)
    # every list probed: the flat index over the covered rows, bit for bit (an fp32 or int8 slab)
    qs = w.pick(slab, [None] * 33, k, NLIST)
    got = _search(w, slab, qs, k, NLIST, "nprobe = nlist")
    assert got[2] == 2 * sum(LENS)
    if slab != "bf16":
        same(got[:2], w.flat0.search(w.q_raw[qs], k), "nprobe = nlist vs the flat index")


def _entries(w, slab):
    """search, search_device and search_device_batch (the grouped fine scan) at every query-count class, bit-identical."""
    k, nprobe = 10, 3
    keep = w.pick(slab, [None] * 70, k, nprobe)
    for nq in (1, 16, 17, 32, 33, 70):
        qs = keep[:nq]
        host = _search(w, slab, qs, k, nprobe, f"host nq {nq}")
        dev = _search(w, slab, qs, k, nprobe, f"device nq {nq}", via="device")
        batch = _search(w, slab, qs, k, nprobe, f"batch nq {nq}", via="batch")
        same(host, dev, f"host vs device nq {nq}")
        same(host, batch, f"host vs batch nq {nq}")
    qs = w.pick(slab, [j % NLIST for j in range(70)], k, 1)     # and with single-list probes, empty lists among them
    host = _search(w, slab, qs, k, 1, "host nprobe 1")
    same(host, _search(w, slab, qs, k, 1, "device nprobe 1", via="device"), "host vs device nprobe 1")
    same(host, _search(w, slab, qs, k, 1, "batch nprobe 1", via="batch"), "host vs batch nprobe 1")


def _filters(w, slab):
    k, nprobe, nq = 10, 3, 33
    ivf = w.ivf(slab)
    # a plain per-query filter: the exact tag, every third query unfiltered
    plain = lambda j: (None if j % 3 == 0 else int((j % 6) | ((j % 2 + 1) << DSHIFT)), None)
    qs = w.pick(slab, [None] * nq, k, nprobe, flt=plain)
    f = np.array([-1 if plain(j)[0] is None else plain(j)[0] for j in range(nq)], dtype=np.int32)
    for via in ("host", "device", "batch"):
        got = w.run(ivf, via, qs, k, nprobe, f)
        w.check(slab, got, qs, k, nprobe, f, what=f"plain filter {via}")
        if slab == "int8":
            same(got, w.run(w.ivf("f32"), via, qs, k, nprobe, f), f"plain filter {via} int8 vs fp32 IVF")
    # a masked filter (patient code / doc_type code) through search_delta: the EXT kernels, and the 45-row delta
    masked = lambda j: ((int(j % 6), PMASK) if j % 2 else (int((j % 4 // 2 + 1) << DSHIFT), DMASK))
    for nprobe in (1, 3):
        qs = w.pick(slab, [None] * nq, k, nprobe, flt=masked, delta=True)
        f = np.array([masked(j)[0] for j in range(nq)], dtype=np.int32)
        m = np.array([masked(j)[1] for j in range(nq)], dtype=np.int32)
        got = ivf.search_delta(w.flat, w.q_raw[qs], k, nprobe, f, m)
        w.check(slab, got, qs, k, nprobe, f, m, delta=True, what=f"masked filter + delta nprobe {nprobe}")
        if slab == "int8":
            same(got, w.ivf("f32").search_delta(w.flat, w.q_raw[qs], k, nprobe, f, m), "masked filter + delta int8 vs fp32 IVF")
    # no filter: the delta is always scanned, and every list probed + the delta is the flat index
    qs = w.pick(slab, [None] * nq, k, 1, delta=True)
    got = ivf.search_delta(w.flat, w.q_raw[qs], k, 1)
    w.check(slab, got, qs, k, 1, delta=True, what="delta nprobe 1")
    if slab != "bf16":
        qs = w.pick(slab, [None] * nq, k, NLIST, delta=True)
        got = ivf.search_delta(w.flat, w.q_raw[qs], k, NLIST)
        same(got[:2], w.flat.search(w.q_raw[qs], k), "nprobe = nlist + delta vs the flat index")


RUN = {"lists": _lists, "entries": _entries, "filters": _filters}


@pytest.mark.parametrize("dim,slab,case", CASES, ids=[f"{d}-{s}-{c}" for d, s, c in CASES])
def test_ivf_matrix(worlds, dim, slab, case):
    RUN[case](worlds(dim), slab)
