"""The list plan of an IVF build on the GPU (rassengine_amd/csrc/ivf_build.hip), the build from a device-resident
assignment (rass_ivf_build_device) and an IVF extended over appended rows without retraining (rass_ivf_absorb).

Everything here is data movement plus the kernels a host-planned build already runs, so every comparison is EQUALITY: the
plan against ``np.argsort(kind="stable")`` restated with the tile padding, the new builders' ``rass_ivf_save`` files against
``rass_ivf_build_prefix``'s from the same centroids and assignment byte for byte, searches id for id and score for score.

One comparison is narrower than "all three slab dtypes": an IVF probed with nprobe = nlist equals the FLAT index bit for bit
over an fp32 slab only — that is what include/rass_engine.h promises and tests/test_gpu_ivf_delta.py pins for a build (a bf16
slab scores rounded rows, an int8 slab re-ranks 32 candidates).  For bf16 / int8 the absorbed IVF is held to its fresh
build instead: the same file, the same answers."""
import ctypes
import filecmp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEAD = -1             # RASS_ROW_TAG_DELETED
INVALID, UNSUPPORTED = -1, -5
PM, DM = 0x00FFFFFF, 0x7F000000


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ 1. the plan
def _plan_ref(assign, tags, nlist, tile_rows):
    n = assign.shape[0]
    rows = np.flatnonzero(tags != DEAD)
    keys = assign[rows].astype(np.int64)
    order = np.argsort(keys, kind="stable")
    rows, keys = rows[order], keys[order]
    length = np.bincount(keys, minlength=nlist).astype(np.int64)
    tiles = (length + tile_rows - 1) // tile_rows
    tile0, start = np.cumsum(tiles) - tiles, np.cumsum(length) - length
    total = int(tiles.sum())
    pos = tile0[keys] * tile_rows + (np.arange(rows.shape[0]) - start[keys])
    slab_ids = np.full(max(total, 1) * tile_rows, -1, dtype=np.int64)
    slab_ids[pos] = rows
    pos_of = np.full(n, -1, dtype=np.int32)
    pos_of[rows] = pos
    return length.astype(np.int32), tile0.astype(np.int32), total, slab_ids, pos_of


def _run_plan(torch, assign, tags, nlist, tile_rows, capacity=None):
    from rassengine_amd import _native as N
    L = N.lib()
    n = int(assign.shape[0])
    cap = int(capacity if capacity is not None else (n // tile_rows + nlist + 1) * tile_rows)
    d_assign, d_tags = torch.from_numpy(assign).cuda(), torch.from_numpy(tags).cuda()
    d_len = torch.full((nlist,), -7, dtype=torch.int32, device="cuda")
    d_tile0 = torch.full((nlist,), -7, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    d_ids = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
    d_pos = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    d_status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.rass_ivf_plan_workspace_bytes(n, nlist))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    N.check("rass_ivf_plan_lists",
            L.rass_ivf_plan_lists(_p(d_assign), _p(d_tags), n, nlist, tile_rows, _p(d_len), _p(d_tile0), _p(d_total), _p(d_ids),
                                  cap, _p(d_pos), _p(d_status), _p(ws), ws_bytes,
                                  ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    return (d_len.cpu().numpy(), d_tile0.cpu().numpy(), int(d_total.item()), d_ids.cpu().numpy(), d_pos.cpu().numpy()[:n],
            int(d_status.item()))


def _plan_inputs(n, nlist, rng):
    """name -> (assign, tags): ~10 % tombstones over random lists / every row tombstoned / every row in one list."""
    tags = rng.integers(0, 1 << 30, size=n).astype(np.int32)
    some = tags.copy()
    some[rng.random(n) < 0.1] = DEAD
    uniform = rng.integers(0, nlist, size=n).astype(np.int32)
    return {"random": (uniform, some), "all-dead": (uniform, np.full(n, DEAD, dtype=np.int32)),
            "one-list": (np.full(n, nlist - 1 - (nlist > 1), dtype=np.int32), some)}


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4_097, 100_000, 3_000_000])
def test_plan_equals_a_stable_argsort_with_tile_padding(gpu, n):
    rng = np.random.default_rng(n)
    for nlist in (1, 7, 256, 257, 4_096, 32_768):
        for name, (assign, tags) in _plan_inputs(n, nlist, rng).items():
            for tile_rows in (32, 64):
                got = _run_plan(gpu, assign, tags, nlist, tile_rows)
                ref = _plan_ref(assign, tags, nlist, tile_rows)
                where = (n, nlist, name, tile_rows)
                assert got[5] == 0, where
                assert got[2] == ref[2], where
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), where
                slab_rows = max(ref[2], 1) * tile_rows
                assert np.array_equal(got[3][:slab_rows], ref[3]), where
                assert np.all(got[3][slab_rows:] == -7), where              # nothing written past the slab
                assert np.array_equal(got[4], ref[4]), where


def test_plan_status_and_determinism(gpu):
    rng = np.random.default_rng(77)
    n, nlist = 100_000, 300
    assign, tags = _plan_inputs(n, nlist, rng)["random"]
    live, dead = np.flatnonzero(tags != DEAD), np.flatnonzero(tags == DEAD)
    a = _run_plan(gpu, assign, tags, nlist, 32)
    b = _run_plan(gpu, assign, tags, nlist, 32)
    assert a[5] == b[5] == 0 and a[2] == b[2]
    for x, y in zip(a[:2] + a[3:5], b[:2] + b[3:5]):
        assert x.tobytes() == y.tobytes()                                   # two runs: identical bytes
    for bad in (nlist, -1, 1 << 20):
        on_dead = assign.copy()
        on_dead[dead[:5]] = bad                                             # a tombstoned row's id is never read as a list
        got = _run_plan(gpu, on_dead, tags, nlist, 32)
        assert got[5] == 0 and np.array_equal(got[3], a[3]) and np.array_equal(got[4], a[4])
        on_live = assign.copy()
        on_live[live[len(live) // 2]] = bad
        assert _run_plan(gpu, on_live, tags, nlist, 32)[5] & 1
    # a slab_ids array that is too short is never written past its end
    short = _run_plan(gpu, assign, tags, nlist, 32, capacity=1024)
    assert short[5] & 4 and np.array_equal(short[3], a[3][:1024])


# ------------------------------------------------------------------------------------------------ shared fixtures
def _clustered(rng, n, centres, sigma=1.0):
    dim = centres.shape[1]
    lab = rng.integers(0, centres.shape[0], size=n)
    return (centres[lab] + sigma * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)).astype(np.float32)


def _tags(rng, n):
    return (rng.integers(1, 5, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)


def _device_assign(index, centroids):
    """``rass_kmeans_assign`` of every row against ``centroids``: the padded device tensor."""
    from rassengine_amd.ivf import _engine_on_torch_stream, kmeans_assign
    with _engine_on_torch_stream(index):
        d_assign, _slab = kmeans_assign(index, centroids)
    return d_assign


def _saved(ivf, path):
    ivf.save(path)
    return path


def _same_file(a, b):
    return os.path.getsize(a) == os.path.getsize(b) and filecmp.cmp(a, b, shallow=False)


def _answers(ivf, flat, q, k, nprobes):
    """Plain, filtered and masked searches through ``rass_ivf_search_delta`` at every nprobe."""
    nq = q.shape[0]
    qf = np.array([(r % 4 + 1) | ((r % 2 + 1) << 24) for r in range(nq)], dtype=np.int32)
    pv, pm = np.array([r % 4 + 1 for r in range(nq)], dtype=np.int32), np.full(nq, PM, dtype=np.int32)
    out = []
    for nprobe in nprobes:
        out.append(ivf.search_delta(flat, q, k, nprobe)[:2])
        out.append(ivf.search_delta(flat, q, k, nprobe, qf)[:2])
        out.append(ivf.search_delta(flat, q, k, nprobe, pv, pm)[:2])
    return out


def _flat_answers(flat, q, k):
    from rassengine_amd.engine import FlatIndex
    nq = q.shape[0]
    qf = np.array([(r % 4 + 1) | ((r % 2 + 1) << 24) for r in range(nq)], dtype=np.int32)
    pv, pm = np.array([r % 4 + 1 for r in range(nq)], dtype=np.int32), np.full(nq, PM, dtype=np.int32)
    return [FlatIndex.search(flat, q, k), FlatIndex.search(flat, q, k, qf), FlatIndex.search(flat, q, k, pv, pm)]


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 2. device build == host build
@pytest.mark.parametrize("n,dim", [(40_000, 256), (20_000, 1024)])
def test_device_build_equals_host_build(gpu, tmp_path, n, dim):
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import IvfIndex
    torch = gpu
    rng = np.random.default_rng(dim)
    nlist = 128
    centres = rng.standard_normal((nlist, dim)).astype(np.float32)
    x, tags = _clustered(rng, n + 13, centres), _tags(rng, n + 13)          # 13: "all rows" is not a multiple of 32
    q = _clustered(rng, 40, centres, sigma=0.7)
    eng = Engine(0, dim)
    try:
        flat = eng.open_index("build-device")
        flat.add(x, tags=tags)
        for r in (0, 5, 31, 32, 4_000, n - 1, n + 12):
            flat.delete(r)
        cent = torch.from_numpy(centres + 0.05 * rng.standard_normal(centres.shape).astype(np.float32)).cuda()
        d_assign = _device_assign(flat, cent)
        h_assign = d_assign[:flat.rows].cpu().numpy()
        for dtype in ("f32", "bf16", "int8"):
            for n_rows in (-1, n // 2 // 32 * 32):
                host = IvfIndex.build(flat, nlist=nlist, centroids=cent, dtype=dtype, assign=h_assign, n_rows=n_rows)
                dev = IvfIndex.build_device(flat, cent, d_assign, dtype=dtype, n_rows=n_rows)
                try:
                    where = (dtype, n_rows)
                    assert dev.covered_rows == host.covered_rows and dev.rows == host.rows and dev.dtype == dtype, where
                    assert _same_file(_saved(host, str(tmp_path / "host.ivf")), _saved(dev, str(tmp_path / "dev.ivf"))), where
                    assert np.array_equal(dev.assign, host.assign) and np.array_equal(dev.list_sizes, host.list_sizes)
                    want = _answers(host, flat, q, 10, (1, 4, 128))
                    assert _equal(_answers(dev, flat, q, 10, (1, 4, 128)), want), where
                    hits = want[-3][1]                                      # plain search, every list probed
                    assert np.all(hits >= 0), where                         # 10 live rows exist for every query
                    covered_hits = hits[(hits >= 0) & (hits < host.covered_rows)]
                    victim = int(covered_hits[0])                           # the first hit that lies in the slab, not in the delta
                    host.delete(victim)                                     # pos_of: the slab position of a source row
                    dev.delete(victim)
                    after = _answers(dev, flat, q, 10, (128,))
                    assert _equal(after, _answers(host, flat, q, 10, (128,))), where
                    assert victim not in after[0][1].reshape(-1).tolist() and dev.rows == host.rows
                finally:
                    host.close()
                    dev.close()
        # without an assignment the builder assigns on the GPU itself; a list id outside [0, nlist) is refused as by the host
        auto = IvfIndex.build_device(flat, cent)
        ref = IvfIndex.build(flat, nlist=nlist, centroids=cent, assign=h_assign)
        assert _same_file(_saved(auto, str(tmp_path / "auto.ivf")), _saved(ref, str(tmp_path / "ref.ivf")))
        auto.close()
        ref.close()
        bad = d_assign.clone()
        bad[1] = nlist
        with pytest.raises(Exception, match="outside"):
            IvfIndex.build_device(flat, cent, bad)
        bad[1], bad[5] = d_assign[1], nlist                                 # row 5 is tombstoned: its id is never read
        IvfIndex.build_device(flat, cent, bad).close()
    finally:
        eng.close()


def test_both_builds_agree_on_degenerate_slabs(gpu, tmp_path):
    """97 rows (no multiple of a tile) over 3 lists of which one stays empty, down to a prefix whose every row is dead: zero
    tiles, the slab is the single padding tile.  At dim 128 a bf16 slab is refused, by both builders alike."""
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import IvfIndex
    torch = gpu
    dim, nlist, n = 128, 3, 97
    rng = np.random.default_rng(97)
    centres = rng.standard_normal((nlist, dim)).astype(np.float32)
    x, tags = _clustered(rng, n, centres), _tags(rng, n)
    q = _clustered(rng, 8, centres, sigma=0.7)
    h_assign = rng.choice(np.array([0, 2], dtype=np.int32), size=n)          # list 1 receives no row
    eng = Engine(0, dim)
    try:
        flat = eng.open_index("degenerate")
        flat.add(x, tags=tags)
        dead = {3, 40, 63, 64, 96}
        for r in sorted(dead):
            flat.delete(r)
        cent = torch.from_numpy(centres).cuda()
        d_assign = torch.zeros(128, dtype=torch.int32, device="cuda")
        d_assign[:n] = torch.from_numpy(h_assign).cuda()
        for n_rows in (-1, 64, 32):
            if n_rows == 32:
                for r in sorted(set(range(32)) - dead):                      # every covered row is dead
                    flat.delete(r)
            for dtype in ("f32", "bf16", "int8"):
                where = (dtype, n_rows)
                if dtype == "bf16":
                    with pytest.raises(Exception, match="multiple of 256"):
                        IvfIndex.build(flat, nlist=nlist, centroids=cent, dtype=dtype, assign=h_assign, n_rows=n_rows)
                    with pytest.raises(Exception, match="multiple of 256"):
                        IvfIndex.build_device(flat, cent, d_assign, dtype=dtype, n_rows=n_rows)
                    continue
                host = IvfIndex.build(flat, nlist=nlist, centroids=cent, dtype=dtype, assign=h_assign, n_rows=n_rows)
                dev = IvfIndex.build_device(flat, cent, d_assign, dtype=dtype, n_rows=n_rows)
                try:
                    assert dev.covered_rows == host.covered_rows == (n if n_rows < 0 else n_rows), where
                    assert dev.rows == host.rows and np.array_equal(dev.list_sizes, host.list_sizes), where
                    if n_rows == 32:
                        assert host.rows == 0, where
                    host_path = _saved(host, str(tmp_path / "host.ivf"))
                    assert _same_file(host_path, _saved(dev, str(tmp_path / "dev.ivf"))), where
                    for nprobe in (1, 3):
                        a, b = host.search_delta(flat, q, 5, nprobe), dev.search_delta(flat, q, 5, nprobe)
                        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]), (where, nprobe)
                    back = IvfIndex.load(eng, host_path)
                    try:
                        assert _same_file(_saved(back, str(tmp_path / "back.ivf")), host_path), where
                    finally:
                        back.close()
                finally:
                    host.close()
                    dev.close()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. / 4. absorb == fresh build
def test_absorb_equals_a_fresh_build_from_the_same_assignment(gpu, tmp_path):
    from rassengine_amd.engine import Engine, FlatIndex
    from rassengine_amd.ivf import IvfIndex
    torch = gpu
    dim, nlist, n0, n80, n = 256, 128, 12_000, 16_000, 20_011
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((150, dim)).astype(np.float32)
    x, tags = _clustered(rng, n, centres), _tags(rng, n)
    q = _clustered(rng, 40, centres, sigma=0.7)
    q[5], q[6] = x[n - 3], x[100]                                           # a late row, and a row that gets tombstoned
    eng = Engine(0, dim)
    try:
        flat = eng.open_index("absorb")
        flat.add(x[:n0], tags=tags[:n0])
        for r in (3, 64, n0 - 1):
            flat.delete(r)                                                  # tombstones BEFORE the build: never enter the slab
        cent = torch.from_numpy(centres[:nlist] + 0.05 * rng.standard_normal((nlist, dim)).astype(np.float32)).cuda()
        old_assign = _device_assign(flat, cent)[:n0].cpu().numpy()
        ivfs = {d: IvfIndex.build(flat, nlist=nlist, centroids=cent, dtype=d, assign=old_assign) for d in ("f32", "bf16", "int8")}
        loaded_path = _saved(ivfs["f32"], str(tmp_path / "before.ivf"))

        def delete(r):                                                      # rass_index_delete + rass_ivf_delete, as IvfBackedIndex
            flat.delete(r)
            for v in ivfs.values():
                v.delete(r)
        for r in (100, 7_777, n0 - 2):
            delete(r)
        flat.add(x[n0:], tags=tags[n0:])
        for r in (n0, n0 + 5, n80 - 1, n80, n - 1):
            delete(r)                                                       # on both sides of both boundaries
        # what a fresh build is built FROM: the old rows' lists, and the nearest centroid of every row appended since
        assign = np.concatenate([old_assign, _device_assign(flat, cent)[n0:n].cpu().numpy()])
        loaded = IvfIndex.load(eng, loaded_path)
        for r in (100, 7_777, n0 - 2):
            loaded.delete(r)                                                # (the file was written before these deletes)
        loaded_files = []
        for step, upto in enumerate((n80, -1)):
            covered = n if upto < 0 else upto
            if step == 1:
                for r in (200, n80 + 7):
                    delete(r)                                               # tombstoned between the two absorbs
                    loaded.delete(r)
            for dtype in ("f32", "bf16", "int8"):
                k = 10
                before = _answers(ivfs[dtype], flat, q, k, (4,))
                new = ivfs[dtype].absorb(flat, upto)
                fresh = IvfIndex.build(flat, nlist=nlist, centroids=cent, dtype=dtype, assign=assign, n_rows=upto)
                where = (step, dtype)
                assert new.covered_rows == fresh.covered_rows == covered and new.rows == fresh.rows and new.dtype == dtype, where
                assert _same_file(_saved(new, str(tmp_path / "new.ivf")), _saved(fresh, str(tmp_path / "fresh.ivf"))), where
                assert _equal(_answers(ivfs[dtype], flat, q, k, (4,)), before), where      # the old IVF is untouched
                if dtype == "f32":
                    # 4. the IVF that came from rass_ivf_load absorbs to the same file as the one that was saved
                    again = loaded.absorb(flat, upto)
                    loaded.close()
                    loaded = again
                    loaded_files.append(_same_file(_saved(loaded, str(tmp_path / "loaded.ivf")), str(tmp_path / "new.ivf")))
                got = _answers(new, flat, q, k, (1, 4, nlist))
                assert _equal(got, _answers(fresh, flat, q, k, (1, 4, nlist))), where
                if dtype == "f32":                                          # every list probed + the delta == the flat scan
                    assert _equal(got[-3:], _flat_answers(flat, q, k)), where
                    assert got[-3][1][5, 0] == n - 3 and 100 not in got[-3][1][6].tolist()
                live_assign = new.assign
                in_slab = live_assign >= 0
                assert np.array_equal(live_assign[in_slab], assign[:covered][in_slab]), where
                assert np.array_equal(new.list_sizes, np.bincount(live_assign[in_slab], minlength=nlist)), where
                assert int(in_slab.sum()) == new.rows
                # the slab position of a source row travels with the absorb: a delete hides the row in both
                victim = int(got[-3][1][1, 0])
                if victim < covered:
                    new.delete(victim)
                    fresh.delete(victim)
                    assert _equal(_answers(new, flat, q, k, (nlist,)), _answers(fresh, flat, q, k, (nlist,))), where
                    flat.delete(victim)
                    for v in list(ivfs.values()) + [loaded]:
                        v.delete(victim)
                fresh.close()
                ivfs[dtype].close()
                ivfs[dtype] = new
        assert loaded_files == [True, True]
        assert ivfs["f32"].covered_rows == n == flat.rows
        assert _equal(_answers(ivfs["f32"], flat, q, 32, (nlist,)), _flat_answers(flat, q, 32))
        loaded.close()
        for v in ivfs.values():
            v.close()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. many workgroups per pass
def test_absorb_at_a_million_rows_and_4096_lists(gpu, tmp_path):
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import IvfIndex
    torch = gpu
    dim, nlist, n0, n1 = 128, 4096, 800_000, 200_003          # 1 000 003 rows: 245 workgroups per digit pass, the last ragged
    eng = Engine(0, dim)
    try:
        flat = eng.open_index("absorb-1m")
        flat.fill_synthetic(n0, seed=11)
        g = torch.Generator(device="cpu")
        g.manual_seed(5)
        cent = torch.randn((nlist, dim), generator=g).cuda()
        for r in (0, 4_095, 4_096, 399_999):
            flat.delete(r)
        old_assign = _device_assign(flat, cent)[:n0].cpu().numpy()
        ivf = IvfIndex.build_device(flat, cent, torch.from_numpy(old_assign).cuda())
        flat.fill_synthetic(n1, seed=12, row_id_base=n0)
        for r in (n0 - 1, n0, n0 + n1 - 1, 123_456):
            flat.delete(r)
            ivf.delete(r)
        assign = np.concatenate([old_assign, _device_assign(flat, cent)[n0:n0 + n1].cpu().numpy()])
        new = ivf.absorb(flat)
        ivf.close()
        fresh = IvfIndex.build(flat, nlist=nlist, centroids=cent, assign=assign)
        assert new.covered_rows == fresh.covered_rows == n0 + n1 and new.rows == fresh.rows == n0 + n1 - 8
        assert _same_file(_saved(new, str(tmp_path / "new.ivf")), _saved(fresh, str(tmp_path / "fresh.ivf")))
        new.close()
        fresh.close()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_both_inputs_as_they_were(gpu):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import IvfIndex
    torch = gpu
    L = N.lib()
    dim, nlist, n0 = 256, 32, 4_096
    rng = np.random.default_rng(9)
    centres = rng.standard_normal((nlist, dim)).astype(np.float32)
    x = _clustered(rng, n0 + 1_000, centres)
    q = _clustered(rng, 8, centres)
    eng, wide = Engine(0, dim), Engine(0, 1536)
    try:
        flat = eng.open_index("refuse")
        flat.add(x[:n0])
        cent = torch.from_numpy(centres).cuda()
        ivf = IvfIndex.build_device(flat, cent)
        flat.add(x[n0:])
        want = ivf.search(q, 5, 8)[:2]
        want_delta = ivf.search_delta(flat, q, 5, 8)[:2]

        def refused(src, n_rows, code, text):
            out = ctypes.c_void_p(1)
            assert L.rass_ivf_absorb(ivf._h, src._h, n_rows, ctypes.byref(out)) == code, text
            assert out.value is None and text.encode() in L.rass_last_error(), L.rass_last_error()
            got = ivf.search(q, 5, 8)[:2]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert ivf.covered_rows == n0

        refused(flat, n0 - 32, INVALID, "below the rows")
        refused(flat, n0 + 1_001, INVALID, "exceeds the rows")
        refused(flat, n0 + 100, INVALID, "multiple of 32")
        b16 = eng.open_index("refuse-bf16", dtype="bf16")
        b16.add(x)
        refused(b16, -1, UNSUPPORTED, "fp32 source")
        w = wide.open_index("refuse-wide")
        w.add(rng.standard_normal((64, 1536)).astype(np.float32))
        refused(w, -1, UNSUPPORTED, "wide rows")
        got = ivf.search_delta(flat, q, 5, 8)[:2]
        assert np.array_equal(got[0], want_delta[0]) and np.array_equal(got[1], want_delta[1])
        assert flat.rows == n0 + 1_000 and flat.count == n0 + 1_000
        # a compaction renumbers the rows: the IVF's ids are stale ordinals
        flat.delete(10)
        ivf.delete(10)
        want = ivf.search(q, 5, 8)[:2]
        flat.compact()
        refused(flat, -1, INVALID, "compacted")
        ivf.close()
    finally:
        eng.close()
        wide.close()


# ------------------------------------------------------------------------------------------------ 7. behind the boundary
def _drive(gpu, monkeypatch, tmp_path, absorb_fraction):
    """256-row uploads up to 4 096 rows with deletes and searches in between; (builds, covered, trainings) after every
    upload.  Every search with nprobe = nlist must equal the flat scan."""
    from rassengine_amd import ivf as M
    from rassengine_amd.engine import Engine, FlatIndex
    dim, nlist = 256, 64
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((100, dim)).astype(np.float32)
    x, tags = _clustered(rng, 4_096, centres), _tags(rng, 4_096)
    q = _clustered(rng, 33, centres, sigma=0.7)
    trainings = []
    real_train = M.train_centroids
    monkeypatch.setattr(M, "train_centroids", lambda index, *a, **kw: (trainings.append(index.rows), real_train(index, *a, **kw))[1])
    eng = Engine(0, dim)
    try:
        policy = M.IvfPolicy(nlist=nlist, nprobe=nlist, min_rows=2_048, absorb_fraction=absorb_fraction, iters=4)
        idx = M.IvfBackedIndex(eng.open_index("boundary"), policy)
        seen, dead = [], set()
        for a in range(0, 4_096, 256):
            idx.add(x[a:a + 256], tags=tags[a:a + 256])
            seen.append((idx.builds, idx.covered, len(trainings)))
            for r in (a + 3, a // 2 + 1, max(0, a - 40)):                   # fresh rows, long-covered rows, rows near the boundary
                if r not in dead:
                    idx.delete(r)
                    dead.add(r)
            for got, want in zip((idx.search(q, 10), idx.search(q, 10, np.full(33, 2, dtype=np.int32), np.full(33, PM, dtype=np.int32))),
                                 (FlatIndex.search(idx, q, 10), FlatIndex.search(idx, q, 10, np.full(33, 2, dtype=np.int32),
                                                                                 np.full(33, PM, dtype=np.int32)))):
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), a
                assert not set(got[1].reshape(-1).tolist()) & dead
        assert idx.count == 4_096 - len(dead)
        path = str(tmp_path / f"boundary-{absorb_fraction}.rass")
        idx.save(path)
        back = M.IvfBackedIndex.load(eng, "boundary-restored", path, policy)
        assert back.rows == idx.rows and back.count == idx.count and back.covered == idx.covered == back.trained_rows
        a, b = idx.search(q, 10), back.search(q, 10)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
        return seen
    finally:
        eng.close()


def test_behind_the_boundary_the_delta_is_absorbed_without_training(gpu, monkeypatch, tmp_path):
    seen = _drive(gpu, monkeypatch, tmp_path, 0.05)
    rows = list(range(256, 4_097, 256))
    # trained at 2 048 rows; every 256-row upload is > 5 % of the covered rows and is absorbed; retrained once the index has
    # grown by more than a quarter since the last training (2 816 > 1.25 x 2 048, 3 584 > 1.25 x 2 816)
    assert [s[2] for s in seen] == [0] * 7 + [1] * 3 + [2] * 3 + [3] * 3, seen
    assert [s[0] for s in seen] == [0] * 7 + list(range(1, 10)), seen
    assert [s[1] for s in seen] == [0] * 7 + rows[7:], seen                 # covered follows the rows: no delta is left


def test_behind_the_boundary_without_absorb_fraction_the_builds_are_todays(gpu, monkeypatch, tmp_path):
    seen = _drive(gpu, monkeypatch, tmp_path, 0.0)
    # the parent's rule: built at 2 048 rows, rebuilt (trained) whenever the delta exceeds a quarter of the covered rows
    assert [s[0] for s in seen] == [0] * 7 + [1] * 3 + [2] * 3 + [3] * 3, seen
    assert [s[1] for s in seen] == [0] * 7 + [2_048] * 3 + [2_816] * 3 + [3_584] * 3, seen
    assert [s[2] for s in seen] == [s[0] for s in seen], seen               # every build trains
