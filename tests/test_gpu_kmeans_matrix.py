"""The k-means kernels of the IVF build (csrc/kmeans.hip) at every row-stride class against the oracle.

``kmeans_assign_f32_kernel<CH>`` is compiled once per stride class (CH = stride / 128 = 1 .. 8; the slot at which the previous
tile pair is ranked differs for every CH) and ``kmeans_accumulate_kernel`` guards every column of a dim that ends inside its
stride.  This file runs both at one dim per class, five of them ragged, three with dim % 4 != 0:

    101 (128), 200 (256), 384, 498 (512), 640, 703 (768), 896, 1024

One world per dim (tests/kmeans_ref.py): (2 CUs + 37) * 32 - 27 rows in an index opened with exactly that capacity (its last
32-row block has 5 rows and its second half lies outside the slab; with a grid of CUs workgroups some walk two row blocks
and some three, with the LDS buffer parity carried over), added in two calls that meet inside a 16-row block; a pool of 200
centroids with exact copies (3 = 20 = 35 = 70, 40 = 66) and an all-zero one, of which a case uses the first nlist, nlist in
1, 7, 17, 32, 33, 49, 65, 96, 97, 200 (1 .. 7 centroid tiles, both parities of ceil(tiles / 2), slabs that end on a half
tile); block ranges (0, 1), (0, 3), (2, 3), (5, 1).

References.  The bits the index stores (``get_rows``) and the bits of the centroid slab the assignment streamed
(``ops.unpack_rows``) go through the oracle's emulation of the scan's summation order (KIND_F32_MFMA), once per dim:
``best`` equals its row maximum BIT FOR BIT and ``assign`` is the lowest list that attains it, exact ties included, for
every processed row; the fp64 score (KIND_F64) of the chosen list is within TOL_F64 of the fp64 maximum.  Sums: within the
worst-case bound of a list's fp32 adds of the fp64 sums, counts equal.  Every output buffer lies between two sentinel-filled
guard regions that must come back untouched.  What the assertions rest on (at least 50 exact-tie rows at every nlist >= 21,
rows won by every duplicate group, ...) is asserted on the reference before the kernel under test is launched, and without
a GPU in tests/test_kmeans_world_cpu.py.

The Python layer (``ivf.train_centroids``, ``assign_rows``) at the ragged dims 101 and 703, and its handling of tombstoned
rows, is at the end.
"""
import ctypes

import numpy as np
import pytest

import kmeans_ref as KR
from test_gpu_scan import TOL_F64

pytestmark = pytest.mark.gpu

GUARD = 1024                                   # sentinel entries in front of and behind every output
# The sentinel is INT32_MIN: no list, and as fp32 bits -0.0, which is no score the kernel can give (its sums start from +0.0)
# and which ANY fp32 add changes, that of a padding column's +0.0 included (-0.0 + +0.0 = +0.0).  The slab's padding columns
# are zero, so an accumulate that lost one of its tail guards (c + 1 < dim, ...) adds only zeros into the next list's first
# columns, and past the end of ``sums`` behind the last list: the guard region behind ``sums`` is where that shows.
SENT_I = -0x80000000
INVALID, UNSUPPORTED = -1, -5                  # RASS_ERR_INVALID, RASS_ERR_UNSUPPORTED
FAMILIES = ("assign", "ranges", "accumulate", "tombstones")
CASES = [(d, f) for d in KR.DIMS for f in FAMILIES]


class Guarded:
    """A device buffer of ``n`` 4-byte entries between two guard regions, all of it filled with SENT_I: ``ptr`` is what the
    C ABI gets, ``intact()`` says whether both guards still hold the sentinel.  As ``sums`` / ``counts`` of an accumulation
    the payload is zero (-0.0), and a cell that nothing was added to still says so."""

    def __init__(self, torch, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT_I).all()) and bool((self.buf[GUARD + self.n:] == SENT_I).all())

    def i32(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy()

    def f32(self):
        return self.i32().view(np.float32)


class World:
    """Rows, centroid pool, both score matrices and the live index of one dim."""

    def __init__(self, torch, oracle, dim):
        from rassengine_amd import ivf, ops
        from rassengine_amd.engine import Engine
        self.torch, self.oracle, self.dim, self.ivf, self.ops = torch, oracle, dim, ivf, ops
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.n = n = KR.n_rows(cus)
        self.total_blocks = -(-n // 32)
        x, cent, self.owner, self.special = KR.make_world(dim, cus)
        self.dead = KR.dead_rows(cus)
        self.eng = Engine(0, dim)
        self.idx = idx = self.eng.open_index("kmeans-matrix", capacity_rows=n)
        assert idx.add(x[:KR.SPLIT], normalize=True) == 0 and idx.add(x[KR.SPLIT:], normalize=True) == KR.SPLIT
        assert idx.rows == n and idx.row_stride == -(-dim // 128) * 128
        self.cent = torch.from_numpy(cent).cuda()
        with ivf._engine_on_torch_stream(idx):
            slab = ivf._pack_centroids(self.cent, idx.row_stride)
            self.cb = ops.unpack_rows(slab, KR.POOL, dim).cpu().numpy()
        self.xb = idx.get_rows(0, n)
        # the stored bits are the normalised rows (pack / unpack at dim % 4 != 0 included): the C restatement to fp32 rounding
        assert np.abs(self.xb.astype(np.float64) - oracle.normalize_c(x)).max() <= 1e-6
        assert np.abs(self.cb.astype(np.float64) - oracle.normalize_c(cent)).max() <= 1e-6
        for grp in KR.DUP_GROUPS:
            for j in grp[1:]:
                assert np.array_equal(self.cb[j].view(np.uint32), self.cb[grp[0]].view(np.uint32))
        assert not self.cb[KR.ZERO_CENTROID].any() and not self.xb[self.special["zero"]].any()
        self.x64 = self.xb.astype(np.float64)
        self.s32 = KR.emulated(oracle, self.cb, self.xb)                        # [n, 200]
        self.s64 = oracle.scores(self.cb, self.xb, kind=oracle.KIND_F64)        # [n, 200]
        assert np.abs(self.s64 - self.s32).max() <= TOL_F64                     # the two references agree with each other
        self.ties = KR.check_world(self.s32, self.owner, self.special)
        print(f"dim {dim}: {n} rows, exact-tie rows per nlist {self.ties}")

    def close(self):
        self.eng.close()

    def assign_abi(self, slab, nlist, first, step, n_blocks):
        """rass_kmeans_assign into guarded buffers -> (assign i32, best f32 bits as u32), guards checked."""
        from rassengine_amd import _native as N
        a, b = Guarded(self.torch, n_blocks * 32), Guarded(self.torch, n_blocks * 32)
        with self.ivf._engine_on_torch_stream(self.idx):
            N.check("rass_kmeans_assign",
                    N.lib().rass_kmeans_assign(self.idx._h, first, step, n_blocks, ctypes.c_void_p(slab.data_ptr()), nlist,
                                               a.ptr, b.ptr))
        assert a.intact() and b.intact(), (nlist, first, step, n_blocks)
        return a.i32(), b.i32().view(np.uint32)

    def accumulate_abi(self, assign, nlist, first, step, n_blocks):
        """rass_kmeans_accumulate of a host int32 assignment into guarded buffers of -0.0 -> (sums [nlist, dim], counts)."""
        from rassengine_amd import _native as N
        s, c = Guarded(self.torch, nlist * self.dim), Guarded(self.torch, nlist)
        d_assign = self.torch.from_numpy(np.ascontiguousarray(assign, dtype=np.int32)).cuda()
        with self.ivf._engine_on_torch_stream(self.idx):
            N.check("rass_kmeans_accumulate",
                    N.lib().rass_kmeans_accumulate(self.idx._h, first, step, n_blocks, ctypes.c_void_p(d_assign.data_ptr()),
                                                   s.ptr, c.ptr, nlist))
        assert s.intact() and c.intact(), (nlist, first, step, n_blocks)
        return s.f32().reshape(nlist, self.dim), c.f32()

    def check_assign(self, got, nlist, first, step, n_blocks, what):
        assign, best_bits = got
        rows = KR.range_rows(first, step, n_blocks)
        ok = rows < self.n
        assert ok[(n_blocks - 1) * 32], what
        assert np.all((assign >= 0) & (assign < nlist)), what                  # entries past rows() included
        ref_a, ref_b = KR.expect(self.s32, nlist)
        r = rows[ok]
        bad = np.flatnonzero(best_bits[ok] != ref_b[r].view(np.uint32))
        assert len(bad) == 0, (what, "best", len(bad), r[bad][:5].tolist(), best_bits[ok][bad][:5].view(np.float32).tolist(),
                               ref_b[r][bad][:5].tolist())
        bad = np.flatnonzero(assign[ok] != ref_a[r])
        assert len(bad) == 0, (what, "assign", len(bad), r[bad][:5].tolist(), assign[ok][bad][:5].tolist(),
                               ref_a[r][bad][:5].tolist())
        chosen = self.s64[r, assign[ok]]
        top = self.s64[r, :nlist].max(axis=1)
        assert np.all(top - chosen <= TOL_F64), (what, float((top - chosen).max()))
        assert np.all(np.abs(best_bits[ok].view(np.float32).astype(np.float64) - top) <= TOL_F64), what

    def check_accumulate(self, got, assign, nlist, first, step, n_blocks, what, guarded=True):
        sums, counts = got
        rows = KR.range_rows(first, step, n_blocks)
        ref_c, ref_s, bound = KR.accumulate_ref(self.x64, rows, assign, nlist, self.n)
        assert np.array_equal(counts.astype(np.float64), ref_c), what
        err = np.abs(sums.astype(np.float64) - ref_s)
        over = np.argwhere(err > bound)
        assert len(over) == 0, (what, len(over), over[:5].tolist(), [float(err[l, c]) for l, c in over[:5]],
                                [float(bound[l, c]) for l, c in over[:5]])
        empty = (ref_c == 0) & guarded                          # nothing, not even a padding column's zero, was added there
        assert np.all(sums[empty].view(np.int32) == SENT_I) and np.all(counts[empty].view(np.int32) == SENT_I), what


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


def _assign(w):
    """Every nlist over all blocks: through ivf.kmeans_assign, and again through the C ABI into guarded buffers."""
    for nlist in KR.NLISTS:
        with w.ivf._engine_on_torch_stream(w.idx):
            a, b, slab = w.ivf.kmeans_assign(w.idx, w.cent[:nlist], with_best=True)
            cb = w.ops.unpack_rows(slab, nlist, w.dim).cpu().numpy()
            got = (a.cpu().numpy(), b.cpu().numpy().view(np.uint32))
        assert np.array_equal(cb.view(np.uint32), w.cb[:nlist].view(np.uint32))     # the slab streamed IS the pool's prefix
        assert got[0].shape == (w.total_blocks * 32,)
        w.check_assign(got, nlist, 0, 1, w.total_blocks, f"nlist {nlist}")
        again = w.assign_abi(slab, nlist, 0, 1, w.total_blocks)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]), nlist
        with w.ivf._engine_on_torch_stream(w.idx):                                  # d_best may be NULL
            only, _slab = w.ivf.kmeans_assign(w.idx, w.cent[:nlist])
            assert np.array_equal(only.cpu().numpy(), got[0])


def _ranges(w):
    for nlist in KR.RANGE_NLISTS:
        with w.ivf._engine_on_torch_stream(w.idx):
            slab = w.ivf._pack_centroids(w.cent[:nlist], w.idx.row_stride)
        for first, step, n_blocks in KR.block_ranges(w.total_blocks)[1:]:
            what = f"nlist {nlist} range ({first}, {step}) x {n_blocks}"
            got = w.assign_abi(slab, nlist, first, step, n_blocks)
            w.check_assign(got, nlist, first, step, n_blocks, what)
            again = w.assign_abi(slab, nlist, first, step, n_blocks)
            assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]), what
            with w.ivf._engine_on_torch_stream(w.idx):                              # the Python wrapper passes the range on
                a, b, _slab = w.ivf.kmeans_assign(w.idx, w.cent[:nlist], first, step, n_blocks, with_best=True)
                assert np.array_equal(a.cpu().numpy(), got[0]) and np.array_equal(b.cpu().numpy().view(np.uint32), got[1])
            if first > 0:                                                           # ... and sizes it when n_blocks is left out
                with w.ivf._engine_on_torch_stream(w.idx):
                    a, _slab = w.ivf.kmeans_assign(w.idx, w.cent[:nlist], first, step)
                    assert np.array_equal(a.cpu().numpy(), got[0]), what


def _accumulate(w):
    ranges = KR.block_ranges(w.total_blocks)
    for nlist, which in ((1, (0,)), (33, (0, 2)), (97, (3,)), (200, (0, 1))):
        with w.ivf._engine_on_torch_stream(w.idx):
            slab = w.ivf._pack_centroids(w.cent[:nlist], w.idx.row_stride)
        for first, step, n_blocks in (ranges[i] for i in which):
            what = f"nlist {nlist} range ({first}, {step}) x {n_blocks}"
            own = w.assign_abi(slab, nlist, first, step, n_blocks)[0]
            w.check_accumulate(w.accumulate_abi(own, nlist, first, step, n_blocks), own, nlist, first, step, n_blocks,
                               what + " own")
            rows = KR.range_rows(first, step, n_blocks)
            theirs = KR.caller_assignment(nlist, rows, w.n, seed=43000 + nlist + first)
            w.check_accumulate(w.accumulate_abi(theirs, nlist, first, step, n_blocks), theirs, nlist, first, step, n_blocks,
                               what + " caller's")
            if first == 0 and step == 1:                                            # the Python wrapper: the same numbers
                with w.ivf._engine_on_torch_stream(w.idx):
                    s, c = w.ivf.kmeans_accumulate(w.idx, w.torch.from_numpy(theirs).cuda(), nlist, first, step, n_blocks)
                    got = (s.cpu().numpy(), c.cpu().numpy())
                w.check_accumulate(got, theirs, nlist, first, step, n_blocks, what + " wrapper", guarded=False)


def _tombstones(w):
    """The primitives compute a tombstoned row like any other: deleting 40 rows changes no output of either."""
    nlist = 97
    first, step, n_blocks = 0, 1, w.total_blocks
    with w.ivf._engine_on_torch_stream(w.idx):
        slab = w.ivf._pack_centroids(w.cent[:nlist], w.idx.row_stride)
    before = w.assign_abi(slab, nlist, first, step, n_blocks)
    theirs = KR.caller_assignment(nlist, KR.range_rows(first, step, n_blocks), w.n, seed=44000)
    acc_before = w.accumulate_abi(theirs, nlist, first, step, n_blocks)
    for r in w.dead:
        w.idx.delete(int(r))
    assert w.idx.count == w.n - KR.N_DEAD and w.idx.rows == w.n
    after = w.assign_abi(slab, nlist, first, step, n_blocks)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    w.check_assign(after, nlist, first, step, n_blocks, "after 40 deletes")
    acc_after = w.accumulate_abi(theirs, nlist, first, step, n_blocks)
    assert np.array_equal(acc_after[1], acc_before[1])
    w.check_accumulate(acc_after, theirs, nlist, first, step, n_blocks, "after 40 deletes")    # the dead rows are IN the sums
    assert np.array_equal(w.idx.get_rows(0, w.n).view(np.uint32), w.xb.view(np.uint32))


RUN = {"assign": _assign, "ranges": _ranges, "accumulate": _accumulate, "tombstones": _tombstones}


@pytest.mark.parametrize("dim,family", CASES, ids=[f"{d}-{f}" for d, f in CASES])
def test_matrix(worlds, dim, family):
    RUN[family](worlds(dim))


def test_refusals(gpu):
    """What the two entry points refuse, and the empty range they accept without touching anything."""
    torch = gpu
    from rassengine_amd import _native as N
    from rassengine_amd import ops
    from rassengine_amd.engine import Engine
    L = N.lib()
    rng = np.random.default_rng(45000)

    def both(idx, slab, nlist, first, step, n_blocks, entries=4096):
        a, b = Guarded(torch, entries), Guarded(torch, entries)
        s, c = Guarded(torch, 4096 * 8), Guarded(torch, 4096)
        torch.cuda.synchronize()                  # the engine works on its own stream here
        rc_a = L.rass_kmeans_assign(idx._h, first, step, n_blocks, ctypes.c_void_p(slab.data_ptr()), nlist, a.ptr, b.ptr)
        rc_c = L.rass_kmeans_accumulate(idx._h, first, step, n_blocks, a.ptr, s.ptr, c.ptr, nlist)
        idx.engine.synchronize()
        untouched = all(bool((g.buf == SENT_I).all()) for g in (a, b, s, c))
        return rc_a, rc_c, untouched

    for dim, dtype, want in ((256, "bf16", UNSUPPORTED), (1100, "f32", UNSUPPORTED)):
        eng = Engine(0, dim)
        try:
            idx = eng.open_index("kmeans-refused", dtype=dtype)
            idx.add(rng.standard_normal((100, dim), dtype=np.float32), normalize=True)
            slab = torch.zeros((16, idx.row_stride), dtype=torch.float32, device="cuda")
            assert both(idx, slab, 4, 0, 1, 4) == (want, want, True), (dim, dtype)
        finally:
            eng.close()
    eng = Engine(0, 200)
    try:
        idx = eng.open_index("kmeans-ranges")
        idx.add(rng.standard_normal((100, 200), dtype=np.float32), normalize=True)           # blocks 0 .. 3, the last of 4 rows
        slab = ops.pack_rows(torch.from_numpy(rng.standard_normal((8, 200), dtype=np.float32)).cuda(), normalize=True,
                             row_stride=idx.row_stride)
        assert both(idx, slab, 0, 0, 1, 4) == (INVALID, INVALID, True)
        assert both(idx, slab, 65537, 0, 1, 4)[::2] == (INVALID, True)       # (accumulate has no upper limit of its own)
        for first, step, n_blocks in ((0, 1, 5), (4, 1, 1), (1, 3, 2), (-1, 1, 2), (0, 0, 2), (0, 1, -1)):
            assert both(idx, slab, 8, first, step, n_blocks) == (INVALID, INVALID, True), (first, step, n_blocks)
        assert both(idx, slab, 8, 0, 1, 0) == (0, 0, True)                    # n_blocks = 0: a no-op
        assert both(idx, slab, 8, 7, 5, 0) == (0, 0, True)
        rc_a, rc_c, untouched = both(idx, slab, 8, 0, 1, 4)                    # ... and what is in range runs
        assert (rc_a, rc_c) == (0, 0) and not untouched
    finally:
        eng.close()


# ---------------------------------------------------------------------------------- the Python layer at ragged dims

def _planted(rng, dim, n=6000, clusters=20):
    centres = rng.standard_normal((clusters, dim)).astype(np.float32)
    return (centres[rng.integers(0, clusters, size=n)] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)


def _lloyd_step(torch, ivf, idx, xn, c0, live):
    """One spherical Lloyd step of the rows ``xn[live]`` from the centroids ``c0`` in fp64 -> (unit means f32, list sizes).
    A row whose two best fp64 scores are within 2 TOL_F64 of each other may go to either of the two in fp32, and one such
    row moves a mean of 300 rows by more than the 1e-5 the means are compared at: there, and only there, the list is the
    one the primitive chose among the two (its own exactness is the matrix's subject); everywhere else the primitive must
    agree with the fp64 arg max."""
    s = xn.double() @ c0.double().T
    top = s.topk(2, dim=1)
    lab = top.indices[:, 0].clone()
    near = (top.values[:, 0] - top.values[:, 1]) <= 2 * TOL_F64
    with ivf._engine_on_torch_stream(idx):
        prim = ivf.kmeans_assign(idx, c0.cuda())[0][:idx.rows].cpu().long()
    assert torch.equal(prim[~near], lab[~near])
    assert float(near.float().mean()) < 0.01
    assert bool(((prim[near] == top.indices[near, 0]) | (prim[near] == top.indices[near, 1])).all())
    lab[near] = prim[near]
    lab, xs = lab[live], xn[live].double()
    sums = torch.zeros((c0.shape[0], xn.shape[1]), dtype=torch.float64).index_add_(0, lab, xs)
    return (sums / (sums.norm(dim=1, keepdim=True) + 1e-9)).float(), torch.bincount(lab, minlength=c0.shape[0])


@pytest.mark.parametrize("dim", (101, 703))
def test_train_centroids_at_ragged_dims(gpu, dim):
    """train_centroids(iters=1) is a torch Lloyd step from the iters=0 seeds, centroids are unit, and assign_rows is the
    primitive's output, at dims that end inside their stride with dim % 4 = 1 and 3."""
    torch = gpu
    from rassengine_amd import ivf
    from rassengine_amd.engine import Engine
    x = _planted(np.random.default_rng(46000 + dim), dim)
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("km-ragged")
        idx.add(x, normalize=True)
        xn = torch.from_numpy(idx.get_rows(0, idx.rows))
        c0 = ivf.train_centroids(idx, nlist=20, iters=0, seed=3, seeding="random", fine_factor=1).cpu()
        c1 = ivf.train_centroids(idx, nlist=20, iters=1, seed=3, seeding="random", fine_factor=1).cpu()
        for c in c0:                                                   # a seed is a stored row, bit for bit
            assert bool((xn == c).all(dim=1).any())
        ref, sizes = _lloyd_step(torch, ivf, idx, xn, c0, torch.ones(idx.rows, dtype=torch.bool))
        assert bool((sizes > 0).all())                                 # a seed wins itself: no list is empty
        assert torch.allclose(c1, ref, atol=1e-5), float((c1 - ref).abs().max())
        assert torch.allclose(c1.norm(dim=1), torch.ones(20), atol=1e-5)
        got = ivf.assign_rows(idx, c1.cuda())
        with ivf._engine_on_torch_stream(idx):
            prim, _slab = ivf.kmeans_assign(idx, c1.cuda())
            prim = prim.cpu().numpy()
        assert got.shape == (6000,) and got.dtype == np.int32 and np.array_equal(got, prim[:6000])
        s = xn.double() @ torch.nn.functional.normalize(c1.double(), dim=1).T
        top2 = s.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1] > 2 * TOL_F64).numpy()
        assert clear.mean() > 0.99 and np.array_equal(got[clear], s.argmax(dim=1).numpy()[clear])
    finally:
        eng.close()


@pytest.mark.parametrize("dim", (101, 703))
def test_training_leaves_tombstoned_rows_out(gpu, dim):
    """A far-off cluster Z holds 30 % of the rows and every row of it is deleted before training: no seed, no mean, no
    empty-list re-seed and no repair draw may come from Z."""
    torch = gpu
    from rassengine_amd import ivf
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(47000 + dim)
    keep = _planted(rng, dim)
    nz = 2571                                                          # 30 % of 8 571
    zc = rng.standard_normal(dim).astype(np.float32)
    z = (zc + 0.3 * rng.standard_normal((nz, dim))).astype(np.float32)
    perm = rng.permutation(6000 + nz)
    x = np.concatenate([keep, z])[perm]
    is_z = (np.arange(6000 + nz) >= 6000)[perm]
    zc_t = torch.nn.functional.normalize(torch.from_numpy(zc), dim=0)
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("km-tombstones")
        idx.add(x, normalize=True)
        for r in np.flatnonzero(is_z):
            idx.delete(int(r))
        assert idx.count == 6000 and idx.rows == 6000 + nz
        xn = torch.from_numpy(idx.get_rows(0, idx.rows))
        live = torch.from_numpy(~is_z)
        assert float((xn[live] @ zc_t).max()) < 0.5 < float((xn[~live] @ zc_t).min())

        def from_live_rows(c):
            """every centroid of ``c`` is a stored LIVE row, bit for bit"""
            return all(bool((xn[live] == v).all(dim=1).any()) for v in c)

        c0 = ivf.train_centroids(idx, nlist=20, iters=0, seed=3, seeding="random", fine_factor=1).cpu()
        assert float((c0 @ zc_t).max()) < 0.5 and from_live_rows(c0)
        assert len({tuple(v.tolist()) for v in c0}) == 20              # distinct rows
        c1 = ivf.train_centroids(idx, nlist=20, iters=1, seed=3, seeding="random", fine_factor=1).cpu()
        ref, sizes = _lloyd_step(torch, ivf, idx, xn, c0, live)
        assert bool((sizes > 0).all())
        assert torch.allclose(c1, ref, atol=1e-5), float((c1 - ref).abs().max())
        assert torch.allclose(c1.norm(dim=1), torch.ones(20), atol=1e-5)

        # empty lists: 20 exact copies of centroid 0 behind the 20 seeds win nothing (ties go to the lowest list) and are
        # re-seeded; _repair: the copies' means coincide with their original's, they yield and are drawn anew
        n_blocks = -(-idx.rows // 32)
        dup = torch.cat([c0, c0[:1].expand(20, dim)]).cuda()
        g = torch.Generator(device="cpu")
        g.manual_seed(5)
        with ivf._engine_on_torch_stream(idx):
            reseeded, counts = ivf._lloyd(idx, dup, 1, 1, n_blocks, g, False, None)
            reseeded, counts = reseeded.cpu(), counts.cpu()
        assert bool((counts[20:] == 0).all()) and float(counts.sum()) == 6000.0
        assert torch.allclose(reseeded[:20], ref, atol=1e-5)
        assert float((reseeded[20:] @ zc_t).max()) < 0.5 and from_live_rows(reseeded[20:])
        with ivf._engine_on_torch_stream(idx):
            _a, best, _slab = ivf.kmeans_assign(idx, dup, 0, 1, n_blocks, with_best=True)
            sizes_d = torch.cat([sizes.float(), torch.zeros(20)]).cuda()
            repaired, n_fixed = ivf._repair(idx, dup, sizes_d, best, 1, n_blocks, g, dup.device)
            repaired = repaired.cpu()
        changed = (repaired != dup.cpu()).any(dim=1)      # the 20 copies, and seeds that share a planted cluster (cosine 0.92)
        assert bool(changed[20:].all()) and n_fixed == int(changed.sum())
        assert float((repaired[changed] @ zc_t).max()) < 0.5 and from_live_rows(repaired[changed])
    finally:
        eng.close()
