"""The stage in front of the IVF's fine scans — which lists are probed, and the work list they become — held to
tests/ivf_probe_ref.py: deep probes (nprobe > 32: a k = 32 scan per 32-centroid tile, a radix select, a threshold mask, the
plan from that mask), the batched plan's in-kernel merge at 8 coarse lists per query, more than 1 024 lists (two and 32 lists
per plan thread, a ragged last coarse tile, the 32 768-list limit), and ties between centroids.

The two rules, from ``rass_ivf_search`` in include/rass_engine.h ("nprobe <= 32 probes the first nprobe lists by (centroid
score desc, list id asc); nprobe > 32 probes every list whose coarse score is >= the nprobe-th best"):

  * nprobe <= 32, two centroids tie across the boundary: the LOWER list id alone is probed — by ``probe_lists``, ``search``,
    ``search_device`` and ``search_device_batch`` (host merge and in-kernel merge alike);
  * nprobe  > 32, the nprobe-th best ties with the next: BOTH are probed.

Every answer is compared with the brute force over the live rows of exactly the lists the reference says are probed: ids
equal (the queries are chosen free of near-ties), scores within TOL_F64 of fp64 (a bf16 slab: over the bf16-rounded operands),
an int8 slab bit for bit the fp32 IVF.  ``scanned`` is the slab length of the union of each 32-query group's probed lists
(+ the delta): the only window onto the mask the select produced, asserted per group wherever the entry point reports it per
group (``search_device_batch``; ``search`` reports the sum over groups).  tests/test_ivf_probe_ref_cpu.py vets the inputs: the
coarse gap at every nprobe boundary exceeds 1e-4 in fp64, 100 x what the engine's coarse scores differ from numpy's by.

``search_allowed_delta``'s ``scanned`` counts the rows of the tiles kept after the bitmap (``ivf_probe_ref.allowed_scanned``):
fewer than the probed lists hold, and again a function of exactly which lists were probed."""
import numpy as np
import pytest

import ivf_probe_ref as R
from test_gpu_ivf_matrix import World as MatrixWorld, same
from test_gpu_scan import TOL_F64
from tests.ivf_allow_ref import member_bits

pytestmark = pytest.mark.gpu

K = R.K
WIDE_CASES = [(d, s, c) for d in R.WIDE_DIMS for s in R.wide_slabs(d) for c in ("deep", "batch", "delta")]


class Gpu:
    """A world of ivf_probe_ref.py on the GPU: the source index (covered rows + delta), the covered rows alone, and an IVF per
    slab dtype built from the caller's centroids and the caller's assignment."""

    def __init__(self, torch, data, slabs, name):
        from rassengine_amd import ops
        from rassengine_amd.engine import Engine
        from rassengine_amd.ivf import IvfIndex
        self.torch, self.d = torch, data
        d = data
        self.eng = Engine(0, d.dim)
        self.flat = self.eng.open_index(name + "-src")
        self.flat0 = self.eng.open_index(name + "-covered")     # what nprobe >= nlist must reproduce
        self.flat.add(d.xn, tags=d.tags_raw, normalize=False)
        self.flat0.add(d.xn[:d.covered], tags=d.tags_raw[:d.covered], normalize=False)
        for r in d.pre_dead:
            self.flat.delete(int(r))
            self.flat0.delete(int(r))
        cent = torch.from_numpy(d.cent).cuda()
        self.ivfs = {}
        for slab in slabs:                                       # every slab before the later deletes: those rows keep their slots
            ivf = IvfIndex.build(self.flat, nlist=d.nlist, centroids=cent, dtype=slab, assign=d.assign, n_rows=d.covered)
            assert ivf.dtype == slab and ivf.nlist == d.nlist and ivf.covered_rows == d.covered and ivf.rows == int(d.slab_len.sum())
            self.ivfs[slab] = ivf
        for r in d.post_dead:
            self.flat.delete(int(r))
            self.flat0.delete(int(r))
            for ivf in self.ivfs.values():
                ivf.delete(int(r))
        d.use_gpu_queries(ops.normalize_rows(torch.from_numpy(d.q_raw).cuda()).cpu().numpy())

    def close(self):
        for ivf in self.ivfs.values():
            ivf.close()
        self.eng.close()

    # what MatrixWorld.check asks of its world
    def top(self, *a, **kw):
        return self.d.top(*a, **kw)

    def scanned(self, *a, **kw):
        return self.d.scanned(*a, **kw)

    check = MatrixWorld.check

    def run(self, slab, via, qs, k, nprobe, qfilter=None):
        """(scores, ids, rows scanned or None, the same per launch group or None)."""
        torch, ivf = self.torch, self.ivfs[slab]
        q = np.ascontiguousarray(self.d.q_raw[qs])
        if via == "host":
            return ivf.search(q, k, nprobe, q_filter=qfilter) + (None,)
        nq = len(qs)
        dq = torch.from_numpy(q).cuda()
        df = None if qfilter is None else torch.from_numpy(np.ascontiguousarray(qfilter, dtype=np.int32)).cuda()
        os_ = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        oi = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        sc = torch.full(((nq + 31) // 32,), -7, dtype=torch.int64, device="cuda")
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
        per = sc.cpu().numpy().tolist() if via == "batch" else None
        return os_.cpu().numpy(), oi.cpu().numpy(), None if per is None else sum(per), per

    def go(self, slab, via, qs, k, nprobe, qfilter=None, what=""):
        """One search against the oracle (an int8 slab: against the fp32 IVF bit for bit); returns (scores, ids, scanned)."""
        what = f"{what} {via} dim {self.d.dim} {slab} nprobe {nprobe} nq {len(qs)} filter {qfilter is not None}"
        got = self.run(slab, via, qs, k, nprobe, qfilter)
        self.check(slab, got[:3], qs, k, nprobe, qfilter, what=what)
        if got[3] is not None:
            assert got[3] == self.d.scanned_groups(qs, nprobe), (what, got[3], self.d.scanned_groups(qs, nprobe))
        if slab == "int8":
            same(got[:3], self.run("f32", via, qs, k, nprobe, qfilter)[:3], what + " int8 vs fp32 IVF")
        return got[:3]


def _filters(nq, flt):
    f = np.array([-1 if flt(j)[0] is None else flt(j)[0] for j in range(nq)], dtype=np.int32)
    m = None if flt(0)[1] is None else np.array([flt(j)[1] for j in range(nq)], dtype=np.int32)
    return f, m


@pytest.fixture(scope="module")
def wide(gpu):
    """dim -> (Gpu, the query sets), one world at a time: the cases of a dim are adjacent."""
    cur = {}

    def get(dim):
        if cur.get("dim") != dim:
            if "g" in cur:
                cur.pop("g").close()
            data = R.Wide(dim)
            cur["dim"], cur["plan"], cur["g"] = dim, R.wide_plan(data), Gpu(gpu, data, R.wide_slabs(dim), f"ivfp-{dim}")
        return cur["g"], cur["plan"]

    yield get
    if "g" in cur:
        cur["g"].close()


def _deep(g, plan, slab):
    """nprobe > 32 through all three entry points (the batch call goes group by group), with and without per-query filters."""
    d = g.d
    for nprobe, keep in plan["deep"].items():
        for nq in R.DEEP_NQS:
            qs = keep[:nq]
            for f in (None, _filters(nq, R.plain_filter)[0]):
                host = g.go(slab, "host", qs, K, nprobe, f, "deep")
                same(host, g.go(slab, "device", qs, K, nprobe, f, "deep"), f"deep host vs device {nprobe} {nq}")
                same(host, g.go(slab, "batch", qs, K, nprobe, f, "deep"), f"deep host vs batch {nprobe} {nq}")
                if nprobe >= d.nlist:
                    assert host[2] == -(-nq // 32) * int(d.slab_len.sum())
                    if slab != "bf16":                      # every list probed: the flat index over the covered rows
                        same(host[:2], g.flat0.search(d.q_raw[qs], K, q_filter=f), f"deep vs the flat index {nprobe} {nq}")


def _batch(g, plan, slab):
    """The batched plan at 8 coarse lists per query (8, 64, 136 and 256 candidates), and ``probe_lists``."""
    d = g.d
    for nprobe, keep in plan["batch"].items():
        assert R.batched_plan_fits(d.nlist, nprobe) and R.batch_coarse_lists(d.nlist, nprobe) == 8
        for nq in R.BATCH_NQS:
            qs = keep[:nq]
            for f in (None, _filters(nq, R.plain_filter)[0]):
                batch = g.go(slab, "batch", qs, K, nprobe, f, "batched plan")
                same(batch, g.go(slab, "device", qs, K, nprobe, f, "batched plan"), f"batch vs device {nprobe} {nq}")
        if nprobe in R.LISTS_NPROBES:
            qs = keep[:70]
            want = np.stack([R.probed_topn(d.order[q], nprobe) for q in qs])
            assert np.array_equal(g.ivfs[slab].probe_lists(d.q_raw[qs], nprobe), want), ("probe_lists", nprobe)


def _delta(g, plan, slab):
    """``search_delta`` under a masked filter and ``search_allowed_delta`` under per-query bitmaps at nprobe 40: both enter
    through the deep branch of the coarse stage."""
    from rassengine_amd.engine import pack_allow
    d, ivf, nprobe = g.d, g.ivfs[slab], R.DELTA_NPROBE
    qs = plan["delta"]
    f, m = _filters(len(qs), R.masked_filter)
    got = ivf.search_delta(g.flat, d.q_raw[qs], K, nprobe, f, m)
    g.check(slab, got, qs, K, nprobe, f, m, delta=True, what=f"masked filter + delta {slab}")
    if slab == "int8":
        same(got, g.ivfs["f32"].search_delta(g.flat, d.q_raw[qs], K, nprobe, f, m), "masked filter + delta int8 vs fp32 IVF")
    if slab != "f32":
        return                                              # the probe within a bitmap reads an fp32 slab
    qs = plan["allow"]
    bits = np.stack([R.allow_bits(d, j) for j in range(len(qs))])
    s, i, scanned = ivf.search_allowed_delta(g.flat, d.q_raw[qs], K, nprobe, pack_allow(bits))
    for j, q in enumerate(qs):
        rs, ri = d.top_of("f32", q, K, d.lists(q, nprobe), delta=True, allow=bits[j])
        assert np.array_equal(i[j], ri), ("allowed", j, i[j].tolist(), ri.tolist())
        assert np.all(ri >= 0) and np.all(np.abs(s[j].astype(np.float64) - rs) <= TOL_F64), ("allowed", j)
    inside = np.stack([member_bits(d.assign, d.lists(q, nprobe), d.covered, d.n) for q in qs])
    same((s, i), g.flat.search_allowed(d.q_raw[qs], K, pack_allow(bits & inside)), "allowed vs the flat allow scan")
    want = R.allowed_scanned(d, qs, nprobe, bits)          # the tiles kept after the bitmap, of exactly the probed lists
    print(f"allowed scanned dim {d.dim}: {scanned} (reference {want}, probed + delta {d.scanned(qs, nprobe, delta=True)})")
    assert scanned == want < d.scanned(qs, nprobe, delta=True), (scanned, want)


WIDE_RUN = {"deep": _deep, "batch": _batch, "delta": _delta}


@pytest.mark.parametrize("dim,slab,case", WIDE_CASES, ids=[f"{d}-{s}-{c}" for d, s, c in WIDE_CASES])
def test_wide(wide, dim, slab, case):
    g, plan = wide(dim)
    WIDE_RUN[case](g, plan, slab)


@pytest.mark.parametrize("slab", ("f32", "int8"))
def test_ties_between_centroids(wide, slab):
    """Bit-copied centroids at consecutive ranks r, r + 1, probed with nprobe = r, alone and inside a 32-query group."""
    g, plan = wide(R.TIE_DIM)
    d, ivf = g.d, g.ivfs[slab]
    assert len(plan["ties"]) >= 2 * len(R.TIE_PAIRS)
    for (lo, hi), q, r in plan["ties"]:
        lists = d.lists(q, r)
        if r + 1 <= 32:
            assert lo in lists and hi not in lists and len(lists) == r
        else:
            assert lo in lists and hi in lists and len(lists) == r + 1
        for qs in (np.array([q]), plan["tie_groups"][(q, r)]):
            what = f"tie {lo}={hi} rank {r}"
            if r <= 32:
                want = np.stack([R.probed_topn(d.order[x], r) for x in qs])
                assert np.array_equal(ivf.probe_lists(d.q_raw[qs], r), want), what
            host = g.go(slab, "host", qs, K, r, None, what)
            assert host[2] == d.scanned_of([d.lists(x, r) for x in qs])
            same(host, g.go(slab, "device", qs, K, r, None, what), what + " host vs device")
            same(host, g.go(slab, "batch", qs, K, r, None, what), what + " host vs batch")
        alone = g.run(slab, "host", np.array([q]), K, r)
        assert alone[2] == int(d.slab_len[lists].sum()), (what, alone[2])      # 17 or 33 rows, or both


# ---- the limit world: 32 768 lists
@pytest.fixture(scope="module")
def limit(gpu):
    data = R.Limit()
    g = Gpu(gpu, data, ("f32",), "ivfp-limit")
    yield g, R.limit_plan(data)
    g.close()


@pytest.mark.parametrize("nprobe", R.LIMIT_NPROBES)
def test_limit_probe(limit, nprobe):
    """32 lists per plan thread, 1 024 coarse tiles; nprobe 40 is the deep path with 1 024 coarse workgroups."""
    g, plan = limit
    for nq in (1, 33, R.LIMIT_BATCH_NQ):
        qs = plan["probe"][nprobe][:nq]
        if nprobe <= 32:
            want = np.stack([R.probed_topn(g.d.order[q], nprobe) for q in qs])
            assert np.array_equal(g.ivfs["f32"].probe_lists(g.d.q_raw[qs], nprobe), want)
        host = g.go("f32", "host", qs, K, nprobe, None, "limit")
        same(host, g.go("f32", "device", qs, K, nprobe, None, "limit"), f"limit host vs device {nprobe} {nq}")


def test_limit_every_list_probed_equals_flat(limit):
    g, plan = limit
    qs = plan["full"]
    host = g.go("f32", "host", qs, K, R.LIMIT_NLIST, None, "limit full")
    assert host[2] == 2 * int(g.d.slab_len.sum())
    same(host, g.go("f32", "device", qs, K, R.LIMIT_NLIST, None, "limit full"), "limit full host vs device")
    same(host[:2], g.flat0.search(g.d.q_raw[qs], K), "limit full vs the flat index")


@pytest.mark.parametrize("nprobe", R.LIMIT_BATCH_NPROBES)
def test_limit_batch(limit, nprobe):
    """``search_device_batch`` at the limit.  nprobe 1: the batched plan, 137 216 bytes of LDS.  nprobe 32: the batched plan
    would need 200 704 bytes, more than a CU's 163 840, so the host plans group by group — the same answer either way."""
    g, plan = limit
    assert R.batched_plan_fits(R.LIMIT_NLIST, nprobe) == (nprobe == 1)
    qs = plan["probe"][nprobe][:R.LIMIT_BATCH_NQ]
    batch = g.go("f32", "batch", qs, K, nprobe, None, "limit batch")
    same(batch, g.go("f32", "device", qs, K, nprobe, None, "limit batch"), f"limit batch vs device {nprobe}")
