"""Compaction of a flat index on the GPU (rass_index_compact, rassengine_amd/csrc/compact.hip), through the C ABI.

Rows are only moved, so everything about the stored bits is held to EQUALITY: the plan against numpy.cumsum, the whole new
slab against rass_pack_rows_f32 of the surviving rows into a zeroed slab, search results before (ids sent through the
returned map) against after.  The comparison with the CPU oracle uses test_gpu_scan.py's tolerances for that comparison
(2e-6 up to 1 024 columns, 3e-6 above: fp32 fmaf chain vs fp64)."""
import ctypes
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_F64 = 2e-6        # tests/test_gpu_scan.py
TOL_F64_WIDE = 3e-6
DEAD = -1             # RASS_ROW_TAG_DELETED


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(torch):
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _patterns(n, rng):
    """name -> bool[n] (True = dead): none / all / random / whole 16-row blocks / the first / the last row."""
    out = {"none": np.zeros(n, dtype=bool)}
    if n == 0:
        return out
    out["all"] = np.ones(n, dtype=bool)
    out["random"] = rng.random(n) < 0.3
    out["whole-block"] = (np.arange(n) // 16) % 2 == 1 if n > 16 else np.ones(n, dtype=bool)
    first = np.zeros(n, dtype=bool)
    first[0] = True
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    out["first"], out["last"] = first, last
    return out


def _plan_ref(tags):
    live = tags != DEAD
    new_row = np.where(live, np.cumsum(live) - live, -1).astype(np.int64)
    return new_row, np.flatnonzero(live).astype(np.int64)


def _run_plan(torch, tags):
    from rassengine_amd import _native as N
    L = N.lib()
    n = int(tags.shape[0])
    d_tags = torch.from_numpy(tags).cuda() if n else torch.empty(0, dtype=torch.int32, device="cuda")
    d_new = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    d_src = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    d_n = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws_bytes = int(L.rass_compact_plan_workspace_bytes(n))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    N.check("rass_compact_plan", L.rass_compact_plan(_p(d_tags), n, _p(d_new), _p(d_src), _p(d_n), _p(ws), ws_bytes,
                                                     _stream(torch)))
    torch.cuda.synchronize()
    return d_new.cpu().numpy()[:n], d_src.cpu().numpy(), int(d_n.item()), (d_src, d_n)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1_000_003])
def test_plan_equals_numpy_cumsum(gpu, n):
    rng = np.random.default_rng(n + 5)
    for name, dead in _patterns(n, rng).items():
        tags = rng.integers(0, 1 << 30, size=n).astype(np.int32)
        tags[dead] = DEAD
        new_row, src_row, n_live, _ = _run_plan(gpu, tags)
        ref_new, ref_src = _plan_ref(tags)
        assert n_live == ref_src.shape[0], (n, name)
        assert np.array_equal(new_row, ref_new), (n, name)
        assert np.array_equal(src_row[:n_live], ref_src), (n, name)
        assert np.all(src_row[n_live:] == -7), (n, name)          # nothing written past n_live


def test_plan_refuses_a_short_workspace(gpu):
    from rassengine_amd import _native as N
    torch = gpu
    L = N.lib()
    n = 100_000
    t = torch.zeros(n, dtype=torch.int32, device="cuda")
    o = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(8, dtype=torch.uint8, device="cuda")
    assert L.rass_compact_plan(_p(t), n, _p(o), _p(o), _p(o), _p(ws), 8, _stream(torch)) == -1
    assert b"workspace" in L.rass_last_error()


def _unpack_all(torch, slab_ptr, stride, rows):
    """Every element of `rows` rows of a tile16 slab (padding columns included), row-major, as uint32."""
    from rassengine_amd import _native as N
    out = torch.empty((rows, stride), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    N.check("unpack", N.lib().rass_unpack_rows_f32(ctypes.c_void_p(slab_ptr), stride, 0, rows, stride, _p(out), stride,
                                                   _stream(torch)))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _expected_slab(torch, rows_rm, stride, cap):
    """rass_pack_rows_f32 (normalize = 0) of row-major `rows_rm` [n, dim] into a zeroed slab of `cap` rows."""
    from rassengine_amd import _native as N
    slab = torch.zeros((cap, stride), dtype=torch.float32, device="cuda")
    n, dim = rows_rm.shape
    if n:
        src = torch.from_numpy(np.ascontiguousarray(rows_rm)).cuda()
        torch.cuda.synchronize()
        N.check("pack", N.lib().rass_pack_rows_f32(_p(src), dim, _p(slab), stride, 0, n, dim, 0, _stream(torch)))
    torch.cuda.synchronize()
    return _unpack_all(torch, slab.data_ptr(), stride, cap)


@pytest.mark.parametrize("stride,dim", [(128, 100), (384, 384), (1024, 1024), (1536, 1530), (2048, 2048)])
def test_gather_whole_slab_equals_pack_of_the_survivors(gpu, stride, dim):
    torch = gpu
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(stride)
    eng = Engine(0, dim)
    try:
        for n in (1, 17, 1000):
            for name, dead in _patterns(n, rng).items():
                # arbitrary bit patterns that are finite floats: any arithmetic on the way would show
                x = rng.standard_normal((n, dim)).astype(np.float32) * np.float32(1e3)
                tags = rng.integers(0, 1000, size=n).astype(np.int32)
                idx = eng.open_index(f"g-{stride}-{n}-{name}")
                idx.add(x, tags=tags, normalize=False)
                assert idx.row_stride == stride
                before = idx.get_rows(0, n).view(np.uint32)
                assert np.array_equal(before, x.view(np.uint32))
                for r in np.flatnonzero(dead):
                    idx.delete(int(r))
                new_row = idx.compact()
                live = int((~dead).sum())
                ref_new, _ = _plan_ref(np.where(dead, DEAD, 0).astype(np.int32))
                assert np.array_equal(new_row, ref_new), (n, name)
                assert idx.rows == idx.count == live, (n, name)
                if live:
                    assert np.array_equal(idx.get_rows(0, live).view(np.uint32), before[~dead]), (n, name)
                if dead.any():      # a compaction that moved rows sized the slab itself: max(round_up(live, 16), 1024) rows
                    cap = max((live + 15) // 16 * 16, 1024)
                    got = _unpack_all(torch, idx.device_rows_ptr, stride, cap)
                    want = _expected_slab(torch, x[~dead], stride, cap)
                    assert np.array_equal(got, want), (n, name)
                eng.drop_index(idx.name)
    finally:
        eng.close()


def test_stateless_gather_launcher(gpu):
    """rass_compact_rows_f32 on caller-owned slabs: the tail rows of the last block are zeroed, an out-of-range source is a
    zero row, and nothing outside round_up(n_dst, 16) rows is written."""
    torch = gpu
    from rassengine_amd import _native as N
    L = N.lib()
    stride, n = 256, 100
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, stride)).astype(np.float32)
    src = torch.zeros((112, stride), dtype=torch.float32, device="cuda")
    d_x = torch.from_numpy(x).cuda()
    pick = np.array([5, 99, 0, 1000, 42, -3, 17], dtype=np.int64)
    d_pick = torch.from_numpy(pick).cuda()
    dst = torch.full((32, stride), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    N.check("pack", L.rass_pack_rows_f32(_p(d_x), stride, _p(src), stride, 0, n, stride, 0, _stream(torch)))
    N.check("compact_rows", L.rass_compact_rows_f32(_p(src), _p(dst), stride, _p(d_pick), len(pick), n, _stream(torch)))
    torch.cuda.synchronize()
    got = _unpack_all(torch, dst.data_ptr(), stride, 32).view(np.float32)
    want = np.zeros((32, stride), dtype=np.float32)
    for j, s in enumerate(pick):
        if 0 <= s < n:
            want[j] = x[s]
    want[16:] = 7.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert L.rass_compact_rows_f32(_p(src), _p(dst), 100, _p(d_pick), 1, n, _stream(torch)) == -1


def test_bf16_index_compacts_to_its_own_rows(gpu):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(8)
    dim, n = 512, 3000
    q = rng.standard_normal((5, dim)).astype(np.float32)
    eng = Engine(0, dim)
    try:
        for name, dead in _patterns(n, rng).items():
            idx = eng.open_index(f"b16-{name}", dtype="bf16")
            idx.add(rng.standard_normal((n, dim)).astype(np.float32))
            before = idx.get_rows(0, n).view(np.uint32)
            for r in np.flatnonzero(dead):
                idx.delete(int(r))
            s0, i0 = idx.search(q, 10)
            new_row = idx.compact()
            live = int((~dead).sum())
            assert idx.rows == idx.count == live, name
            assert np.array_equal(new_row, _plan_ref(np.where(dead, DEAD, 0).astype(np.int32))[0]), name
            if live:
                assert np.array_equal(idx.get_rows(0, live).view(np.uint32), before[~dead]), name
            s1, i1 = idx.search(q, 10)
            assert np.array_equal(np.where(i0 >= 0, new_row[np.maximum(i0, 0)], -1), i1), name
            assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), name
            eng.drop_index(idx.name)
    finally:
        eng.close()


def _map_ids(ids, new_row):
    return np.where(ids >= 0, new_row[np.maximum(ids, 0)], -1)


def _oracle_check(oracle, xn, tags, q, k, s, i, qf, qm, tol):
    qn = oracle.normalize_ref(q).astype(np.float32)
    rs, ri = oracle.search(xn, qn, k, tags=tags, qfilter=qf, qmask=qm)
    valid = ri >= 0
    assert np.array_equal(i >= 0, valid)
    all64 = qn.astype(np.float64) @ xn.astype(np.float64).T
    for qq, e in zip(*np.nonzero(valid & (i != ri))):     # swapped ids only where fp64 cannot tell them apart
        assert abs(all64[qq, i[qq, e]] - all64[qq, ri[qq, e]]) <= 2 * tol
    got64 = np.take_along_axis(all64, np.maximum(i, 0), axis=1)
    assert np.all(np.abs(s[valid].astype(np.float64) - got64[valid]) <= tol)


@pytest.mark.parametrize("n,dim", [(20000, 1024), (6000, 1536), (6000, 200)])
def test_search_is_the_same_before_and_after(gpu, oracle, n, dim):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(dim)
    tol = TOL_F64 if dim <= 1024 else TOL_F64_WIDE
    x = rng.standard_normal((n, dim)).astype(np.float32)
    tags = (rng.integers(1, 4, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)
    dead = rng.random(n) < 0.3
    q = rng.standard_normal((33, dim)).astype(np.float32)
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("s")
        idx.add(x, tags=tags)
        for r in np.flatnonzero(dead):
            idx.delete(int(r))
        xn = idx.get_rows(0, n)
        cases = []
        for k in (10, 32, 70):
            for nq in (1, 32, 33):
                qf = rng.integers(1, 4, size=nq).astype(np.int32)
                qm = np.full(nq, 0x00FFFFFF, dtype=np.int32)
                for f, m in ((None, None), (qf, qm)):
                    cases.append((k, nq, f, m, idx.search(q[:nq], k, f, m)))
        epoch = idx.layout_epoch
        new_row = idx.compact()
        assert idx.layout_epoch == epoch + 1 and idx.rows == idx.count == int((~dead).sum())
        assert np.array_equal(new_row, _plan_ref(np.where(dead, DEAD, 0).astype(np.int32))[0])
        for k, nq, f, m, (s0, i0) in cases:
            s1, i1 = idx.search(q[:nq], k, f, m)
            assert np.array_equal(_map_ids(i0, new_row), i1), (k, nq, f is not None)
            assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), (k, nq, f is not None)
            _oracle_check(oracle, xn[~dead], tags[~dead], q[:nq], k, s1, i1, f, m, tol)
    finally:
        eng.close()


@pytest.mark.parametrize("mode,kmax", [("bf16", 16), ("int8", 16), ("int8_exact", 32)])
def test_prefilter_modes_set_before_the_compaction(gpu, mode, kmax):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(kmax)
    n, dim = 20000, 1024
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("p")
        idx.add(rng.standard_normal((n, dim)).astype(np.float32), tags=rng.integers(1, 4, size=n).astype(np.int32))
        idx.set_prefilter(mode)
        dead = rng.random(n) < 0.3
        for r in np.flatnonzero(dead):
            idx.delete(int(r))
        q = rng.standard_normal((33, dim)).astype(np.float32)
        qf = rng.integers(1, 4, size=33).astype(np.int32)
        cases = [(k, nq, f, idx.search(q[:nq], k, f)) for k in (10, kmax) for nq in (1, 33) for f in (None, qf[:nq])]
        new_row = idx.compact()
        assert idx.prefilter_mode == mode and idx.rows == idx.count
        for k, nq, f, (s0, i0) in cases:
            s1, i1 = idx.search(q[:nq], k, f)
            assert np.array_equal(_map_ids(i0, new_row), i1), (mode, k, nq)
            assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), (mode, k, nq)
        if mode == "int8_exact":
            st0 = idx.certify_stats()
            idx.search(q[:16], 10)
            st1 = idx.certify_stats()
            assert st1["queries"] == st0["queries"] + 16
            assert st1["certified"] + st1["fallbacks"] == st1["queries"] and st1["certified"] > st0["certified"]
            assert st1["R"] >= st0["R"] > 0 and st1["V"] >= st0["V"] > 0
    finally:
        eng.close()


def test_caller_assigned_ids_travel_with_their_rows(gpu):
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(12)
    n, dim = 4000, 256
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("gid")
        idx.add(rng.standard_normal((n // 2, dim)).astype(np.float32), first_global_id=1000)
        idx.add(rng.standard_normal((n // 2, dim)).astype(np.float32), first_global_id=900000)
        for r in np.flatnonzero(rng.random(n) < 0.3):
            idx.delete(int(r))
        q = rng.standard_normal((8, dim)).astype(np.float32)
        s0, i0 = idx.search(q, 20)
        idx.compact()
        assert idx.has_global_ids and idx.rows == idx.count
        s1, i1 = idx.search(q, 20)
        assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
        assert i1.min() >= 1000
    finally:
        eng.close()


def test_lifecycle(gpu, tmp_path):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(2)
    n, dim = 3000, 384
    x = rng.standard_normal((n + 10, dim)).astype(np.float32)
    eng = Engine(0, dim)
    try:
        idx = eng.open_index("life")
        idx.add(x[:n], normalize=False)
        assert idx.layout_epoch == 0 and idx.epoch == (n, 0, 0)
        assert np.array_equal(idx.compact(), np.arange(n)) and idx.layout_epoch == 0     # no tombstone: identity
        dead = rng.random(n) < 0.4
        for r in np.flatnonzero(dead):
            idx.delete(int(r))
        live = int((~dead).sum())
        # a map that is too small: refused, nothing changes
        small = np.empty(n - 1, dtype=np.int64)
        rb, ra = ctypes.c_int64(-1), ctypes.c_int64(-1)
        rc = N.lib().rass_index_compact(idx._h, small.ctypes.data_as(ctypes.c_void_p), n - 1, ctypes.byref(rb), ctypes.byref(ra))
        assert rc == -1 and b"map_capacity" in N.lib().rass_last_error()
        assert idx.rows == n and idx.count == live and idx.layout_epoch == 0
        idx.compact()
        assert idx.rows == idx.count == live and idx.layout_epoch == 1 and idx.epoch == (live, 0, 1)
        assert np.array_equal(idx.compact(), np.arange(live)) and idx.layout_epoch == 1   # twice: a no-op
        # an add lands at ordinal `live` and is found; a delete of a new ordinal works
        assert idx.add(x[n:], normalize=False) == live and idx.rows == live + 10
        s, i = idx.search(x[n:n + 3], 1)
        assert i[:, 0].tolist() == [live, live + 1, live + 2]
        idx.delete(live + 1)
        assert idx.search(x[n + 1:n + 2], 1)[1][0, 0] != live + 1 and idx.count == live + 9
        # save / load round trip of the compact index: epoch 0 again, same rows, same tombstone
        path = str(tmp_path / "life.rass")
        idx.save(path)
        back = eng.load_index("life-back", path)
        assert back.rows == live + 10 and back.count == live + 9 and back.layout_epoch == 0
        assert np.array_equal(back.get_rows(0, back.rows).view(np.uint32), idx.get_rows(0, idx.rows).view(np.uint32))
        assert np.array_equal(back.get_rows(0, live).view(np.uint32), x[:n][~dead].view(np.uint32))
        # every row dead: an empty index that accepts appends
        for r in range(back.rows):
            back.delete(r)
        m = back.compact()
        assert np.all(m == -1) and back.rows == back.count == 0 and back.layout_epoch == 1
        assert np.all(back.search(x[:2], 3)[1] == -1)
        assert back.add(x[:5], normalize=False) == 0 and back.search(x[3:4], 1)[1][0, 0] == 3
    finally:
        eng.close()


def test_ivf_backed_index_drops_and_rebuilds_and_a_stale_ivf_is_refused(gpu):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import IvfBackedIndex, IvfIndex, IvfPolicy
    rng = np.random.default_rng(31)
    n, dim, nlist = 6000, 256, 16
    eng = Engine(0, dim)
    try:
        idx = IvfBackedIndex(eng.open_index("ivf-c"), IvfPolicy(nlist=nlist, nprobe=nlist, min_rows=1000, iters=4))
        idx.add(rng.standard_normal((n, dim)).astype(np.float32), tags=rng.integers(1, 4, size=n).astype(np.int32))
        assert idx.ivf is not None and idx.builds == 1
        stale = IvfIndex.build(idx, nlist=nlist, iters=4)
        for r in np.flatnonzero(rng.random(n) < 0.3):
            idx.delete(int(r))
        q = rng.standard_normal((9, dim)).astype(np.float32)
        s0, i0 = idx.search(q, 10, exact=True)
        builds, ep = idx.builds, idx.epoch
        new_row = idx.compact()
        assert idx.builds == builds + 2 and idx.ivf is not None          # dropped, then rebuilt over the compacted rows
        assert idx.covered == idx.rows // 32 * 32 and idx.rows == idx.count
        assert idx.epoch != ep and idx.epoch[3] == 1
        s1, i1 = idx.search(q, 10)                                       # nprobe = nlist: the flat answer
        s2, i2 = idx.search(q, 10, exact=True)
        assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
        assert np.array_equal(_map_ids(i0, new_row), i2) and np.array_equal(s0.view(np.uint32), s2.view(np.uint32))
        with pytest.raises(N.RassError) as e:
            stale.search_delta(idx, q, 10, nlist)
        assert e.value.code == -1 and "compacted" in str(e.value)
        stale.close()
    finally:
        eng.close()


def test_one_layout_per_answer_under_concurrent_compactions(gpu, oracle):
    """Two threads search through the host API (k = 10: launch groups; k = 70: launch groups x passes; 40 queries per call)
    while a third tombstones predetermined rows and compacts three times, keeping for every layout epoch the map from its
    ordinals back to the original rows.  An answer read under one epoch (the same before and after the call) must be an
    answer of THAT layout.  Each compaction can straddle at most one call per thread, so with 3 compactions and >= 100
    calls per thread at most 3 % of a thread's calls may be discarded by construction; the test allows a quarter."""
    from rassengine_amd.engine import Engine
    rng = np.random.default_rng(99)
    n, dim, nq, rounds, min_calls = 20000, 256, 40, 3, 100
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    victims = [np.sort(rng.choice(np.arange(c, n, rounds), size=1500, replace=False)) for c in range(rounds)]
    eng = Engine(0, dim)
    errors, counts, discarded = [], {10: 0, 70: 0}, {10: 0, 70: 0}
    try:
        idx = eng.open_index("layouts")
        idx.add(x)
        xn = idx.get_rows(0, n)
        qn = oracle.normalize_ref(q).astype(np.float32)
        all64 = qn.astype(np.float64) @ xn.astype(np.float64).T
        # the pre-compaction search's score of every row that can ever be in a top-70 of the survivors
        sb, ib = idx.search(q, 1024)
        base = [dict(zip(ib[j].tolist(), sb[j].view(np.uint32).tolist())) for j in range(nq)]
        maps = {0: np.arange(n)}                     # layout epoch -> original row of every ordinal
        dead_before = {0: np.zeros(n, dtype=bool)}   # layout epoch -> original rows deleted before it began
        stop = threading.Event()

        def searcher(k):
            try:
                while not stop.is_set() or counts[k] < min_calls:
                    e0 = idx.layout_epoch
                    s, i = idx.search(q, k)
                    e1 = idx.layout_epoch
                    counts[k] += 1
                    if e0 != e1:
                        discarded[k] += 1
                        continue
                    t0 = time.time()
                    while e0 not in maps:            # the writer publishes the map right after its compact() returns
                        assert time.time() - t0 < 30
                        time.sleep(0.001)
                    assert np.all(i >= 0) and np.all(i < maps[e0].shape[0])
                    orig = maps[e0][i]
                    assert not dead_before[e0][orig].any(), "a row deleted before this layout began"
                    for j in range(nq):
                        assert len(set(orig[j].tolist())) == k
                        bits = s[j].view(np.uint32)
                        assert [base[j][r] for r in orig[j].tolist()] == bits.tolist(), "not the pre-compaction score"
                        assert np.all(np.abs(s[j].astype(np.float64) - all64[j, orig[j]]) <= TOL_F64)
                        d = np.diff(s[j])
                        assert np.all((d < 0) | ((d == 0) & (np.diff(i[j]) > 0))), "not (score desc, id asc)"
            except Exception as e:  # noqa: BLE001
                errors.append((f"searcher k={k}", repr(e)))

        def writer():
            try:
                for c in range(rounds):
                    t0 = time.time()
                    while min(counts.values()) < (c + 1) * 25 and not errors:
                        assert time.time() - t0 < 60
                        time.sleep(0.002)
                    e = idx.layout_epoch
                    inv = np.full(n, -1, dtype=np.int64)
                    inv[maps[e]] = np.arange(maps[e].shape[0])
                    for r in victims[c]:
                        idx.delete(int(inv[r]))
                    dead = dead_before[e].copy()
                    dead[victims[c]] = True
                    dead_before[e + 1] = dead
                    new_row = idx.compact()
                    keep = new_row >= 0
                    assert np.array_equal(maps[e][keep], np.flatnonzero(~dead))
                    maps[e + 1] = maps[e][keep]
            except Exception as e:  # noqa: BLE001
                errors.append(("writer", repr(e)))
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(k,)) for k in (10, 70)] + [threading.Thread(target=writer)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=240)
        assert not any(t.is_alive() for t in threads), "threads did not finish"
        assert not errors, errors[:3]
        assert idx.layout_epoch == rounds and idx.rows == idx.count == n - rounds * 1500
        for k in (10, 70):
            print(f"k={k}: {counts[k]} calls, {discarded[k]} discarded")
            assert counts[k] >= min_calls and discarded[k] <= counts[k] // 4, (k, counts[k], discarded[k])
    finally:
        eng.close()
