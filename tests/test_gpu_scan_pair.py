"""The 64-query pair kernel of the batched exact fp32 flat scan (scan_topk_f32_pair_kernel, two consecutive full launch
groups per corpus pass): rass_index_search_device_batch must still equal rass_index_search_device on consecutive groups of
32 queries BIT FOR BIT (ids, and scores compared as uint32) — pairs, an odd last full group, a ragged tail; every eligible
row stride; per-query filters with rare and absent tags, tombstones, caller-assigned ids, id_base, strided outputs; exact
score ties across the two 16-row blocks of a tile and across workgroups (order: score desc, id asc); tiny row counts; and
the switches RASS_SCAN_BATCH_PAIR / RASS_SCAN_SAMPLE_FLOOR, each in a fresh child process (the former is read once).

The full-size case (1 M x 1024, 1 024 queries, the bench step) is tests/test_gpu_batch_search.py::
test_batch_full_size_equals_groups, which runs through the pair kernel by default.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_group(torch, ix, q, k, filt=None, id_base=0):
    n = q.shape[0]
    s = torch.empty((n, k), dtype=torch.float32, device="cuda")
    i = torch.empty((n, k), dtype=torch.int64, device="cuda")
    for g in range(0, n, 32):
        b = min(32, n - g)
        ix.search_device(q[g:g + b].data_ptr(), b, k, s[g:g + b].data_ptr(), i[g:g + b].data_ptr(), id_base=id_base,
                         d_q_filter_ptr=filt[g:g + b].data_ptr() if filt is not None else 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _batch(torch, ix, q, k, filt=None, id_base=0):
    n = q.shape[0]
    s = torch.empty((n, k), dtype=torch.float32, device="cuda")
    i = torch.empty((n, k), dtype=torch.int64, device="cuda")
    ix.search_device_batch(q.data_ptr(), n, k, s.data_ptr(), i.data_ptr(), id_base=id_base,
                           d_q_filter_ptr=filt.data_ptr() if filt is not None else 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _with_floor_modes(fn):
    """fn() without and with the sample floor (forced: the slabs here are smaller than the default threshold)."""
    for mode in ("0", "force"):
        os.environ["RASS_SCAN_SAMPLE_FLOOR"] = mode
        try:
            fn(mode)
        finally:
            os.environ.pop("RASS_SCAN_SAMPLE_FLOOR", None)


def _queries(torch, nq, dim, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn((nq, dim), generator=g, device="cuda")


def _launches(eng, fn):
    """What kernel_timing_end reports: launch GROUPS scanned (a 64-query pair pass counts as two)."""
    eng.kernel_timing_begin(256)
    fn()
    return eng.kernel_timing_end()[1]


@pytest.fixture(scope="module")
def small(gpu):
    from rassengine_amd.engine import Engine
    torch = gpu
    rng = np.random.default_rng(7)
    n, dim = 40_000, 1024
    x = rng.standard_normal((n, dim)).astype(np.float32)
    tags = rng.integers(1, 50, size=n).astype(np.int32)
    tags[12_345] = 777          # a rare tag: one row of the slab
    eng = Engine(0, dim)
    eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
    ix = eng.open_index("pair")
    ix.add(x, tags=tags)
    for r in (0, 15, 16, 31, 32, 39_999, 20_000):
        ix.delete(r)
    yield torch, eng, ix
    eng.close()


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("nq", [64, 96, 100, 128, 1024, 4096])
def test_pairs_odd_group_and_ragged_tail_equal_groups(small, nq, k):
    torch, eng, ix = small
    q = _queries(torch, nq, 1024, nq * 31 + k)
    ref = _per_group(torch, ix, q, k)

    def run(mode):
        assert _same(_batch(torch, ix, q, k), ref), mode
    _with_floor_modes(run)


def test_kernel_timing_counts_launch_groups(small):
    """bench.py's roofline line stays in launch-group units: bytes_per_launch x launches / ms is the rate at which corpus
    bytes are SERVED to 32-query groups, pair pass or not."""
    torch, eng, ix = small
    for nq in (64, 96, 100, 128, 1024, 33):
        q = _queries(torch, nq, 1024, nq)
        assert _launches(eng, lambda: _batch(torch, ix, q, 10)) == (nq + 31) // 32, nq


# every eligible stride (CH = stride / 128 = 1..8), two dims that are not multiples of 128 among them
@pytest.mark.parametrize("dim", [100, 256, 384, 512, 640, 700, 896, 1024])
def test_every_eligible_stride(gpu, dim):
    from rassengine_amd.engine import Engine
    torch = gpu
    rng = np.random.default_rng(dim)
    n = 20_000
    x = rng.standard_normal((n, dim)).astype(np.float32)
    tags = rng.integers(0, 9, size=n).astype(np.int32)
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        ix = eng.open_index("stride")
        ix.add(x, tags=tags)
        ix.delete(5)
        ix.delete(19_999)
        assert ix.row_stride == (dim + 127) // 128 * 128
        q = _queries(torch, 100, dim, dim + 1)
        filt = torch.randint(-1, 9, (100,), dtype=torch.int32, device="cuda")
        ref = _per_group(torch, ix, q, 10)
        ref_f = _per_group(torch, ix, q, 10, filt=filt)

        def run(mode):
            assert _same(_batch(torch, ix, q, 10), ref), mode
            assert _same(_batch(torch, ix, q, 10, filt=filt), ref_f), mode
        _with_floor_modes(run)
        assert _launches(eng, lambda: _batch(torch, ix, q, 10)) == 4    # launch groups: one pair, one full group, the ragged tail
        # and no row is lost by BOTH paths alike: every row that beats the fp64 k-th best by more than fp32 noise is reported
        xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
        qh = q.cpu().numpy().astype(np.float64)
        S = (qh / np.linalg.norm(qh, axis=1, keepdims=True)) @ xn.T
        S[:, [5, 19_999]] = -np.inf
        kth = np.sort(S, axis=1)[:, -10]
        for row in range(100):
            must = np.nonzero(S[row] > kth[row] + 1e-5)[0]
            assert set(must) <= set(ref[1][row]), (row, must, ref[1][row])
    finally:
        eng.close()


def test_filters_rare_and_absent_tags_and_id_base(small):
    torch, eng, ix = small
    nq = 160
    q = _queries(torch, nq, 1024, 99)
    filt = torch.randint(1, 50, (nq,), dtype=torch.int32, device="cuda")
    filt[3] = -1
    filt[40] = 777      # one matching row
    filt[41] = 9999     # matches nothing
    filt[70] = 777
    filt[100] = 9999
    ref = _per_group(torch, ix, q, 10, filt=filt, id_base=7_000_000)

    def run(mode):
        a = _batch(torch, ix, q, 10, filt=filt, id_base=7_000_000)
        assert _same(a, ref), mode
        assert np.all(a[1][41] == -1) and np.all(a[1][100] == -1)
        assert a[1][40, 0] == 7_000_000 + 12_345 and np.all(a[1][40, 1:] == -1)
        assert a[1][3, 0] >= 7_000_000
    _with_floor_modes(run)


def test_caller_assigned_ids_and_strided_outputs(gpu):
    from rassengine_amd.engine import Engine
    torch = gpu
    rng = np.random.default_rng(21)
    dim, k, nq = 512, 10, 128
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        ix = eng.open_index("gid")
        ix.add(rng.standard_normal((9_000, dim)).astype(np.float32), first_global_id=5_000_000)
        ix.add(rng.standard_normal((7_000, dim)).astype(np.float32), first_global_id=100)
        ix.delete(8_999)
        assert ix.has_global_ids
        q = _queries(torch, nq, dim, 4)
        ref = _per_group(torch, ix, q, k)
        assert _same(_batch(torch, ix, q, k), ref)
        assert ref[1].max() >= 5_000_000 and ref[1].min() >= 100
        # strided outputs: group g's block of 32 * k at g * stride, the gaps untouched
        ss, si = 32 * k + 24, 32 * k + 40
        groups = nq // 32
        s = torch.full((groups * ss,), -7.0, dtype=torch.float32, device="cuda")
        i = torch.full((groups * si,), -7, dtype=torch.int64, device="cuda")
        ix.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), out_scores_group_stride=ss,
                               out_ids_group_stride=si)
        torch.cuda.synchronize()
        s, i = s.cpu().numpy().reshape(groups, ss), i.cpu().numpy().reshape(groups, si)
        assert np.array_equal(s[:, :32 * k].reshape(nq, k).view(np.uint32), ref[0].view(np.uint32))
        assert np.array_equal(i[:, :32 * k].reshape(nq, k), ref[1])
        assert np.all(s[:, 32 * k:] == -7.0) and np.all(i[:, 32 * k:] == -7)
    finally:
        eng.close()


@pytest.mark.parametrize("n", [5_000, 40_000])
def test_duplicate_rows_tie_by_id(gpu, n):
    """7 distinct vectors repeated down the slab: every score occurs ~n/7 times, in both 16-row blocks of a tile, in
    consecutive tiles and in every workgroup (5 000 rows: fewer tiles than workgroups).  Ties resolve by ascending id."""
    from rassengine_amd.engine import Engine
    torch = gpu
    rng = np.random.default_rng(n)
    dim, k = 1024, 32
    base = rng.standard_normal((7, dim)).astype(np.float32)
    x = base[np.arange(n) % 7]
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        ix = eng.open_index("dups")
        ix.add(x)
        for r in (0, 7, 16, 23):
            ix.delete(r)
        q = _queries(torch, 96, dim, 8)
        ref = _per_group(torch, ix, q, k)

        def run(mode):
            s, i = _batch(torch, ix, q, k)
            assert _same((s, i), ref), mode
            for row in range(96):
                # (score desc, id asc): scores never increase, ids increase inside a run of equal scores
                assert np.all(s[row, 1:] <= s[row, :-1])
                eq = s[row, 1:] == s[row, :-1]
                assert np.all(i[row, 1:][eq] > i[row, :-1][eq])
                # the best vector's copies come first, smallest live ids first
                best = i[row, 0] % 7
                live = [r for r in range(7 * 40) if r % 7 == best and r not in (0, 7, 16, 23)][:k]
                assert list(i[row]) == live
        _with_floor_modes(run)
    finally:
        eng.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, 1000])
def test_tiny_and_ragged_row_counts(gpu, n):
    from rassengine_amd.engine import Engine
    torch = gpu
    rng = np.random.default_rng(100 + n)
    dim, k = 1024, 10
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        ix = eng.open_index("tiny")
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        for nq in (64, 100):
            q = _queries(torch, nq, dim, n + nq)
            a, b = _batch(torch, ix, q, k), _per_group(torch, ix, q, k)
            assert _same(a, b), nq
            assert np.all((a[1] >= 0).sum(axis=1) == min(n, k))
    finally:
        eng.close()


# ---- the switches, each in a fresh child process -------------------------------------------------------------------------

def _child(out_path):
    """600 000 synthetic rows (the sample floor is on by default from 32 samples of 64 * grid rows), 128 + 32 + 5 queries."""
    import torch
    from rassengine_amd.engine import Engine
    eng = Engine(0, 1024)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        ix = eng.open_index("child", capacity_rows=600_000)
        ix.fill_synthetic(600_000, seed=5)
        ix.delete(3)
        q = _queries(torch, 165, 1024, 17)
        for _ in range(3):      # warm-up: code objects, clocks
            _batch(torch, ix, q, 10)
        eng.kernel_timing_begin(64)
        for _ in range(5):
            s, i = _batch(torch, ix, q, 10)
        ms, launches = eng.kernel_timing_end()
        np.savez(out_path, s=s.view(np.uint32), i=i, launches=np.int64(launches // 5), ms=np.float64(ms / 5))
    finally:
        eng.close()


def _run_child(tmp_path, name, env_extra):
    out = str(tmp_path / (name + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in ("RASS_SCAN_BATCH_PAIR", "RASS_SCAN_SAMPLE_FLOOR")}
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=env, cwd=ROOT, timeout=600)
    return np.load(out)


def test_switches_do_not_change_results(gpu, tmp_path):
    base = _run_child(tmp_path, "default", {})
    assert int(base["launches"]) == 6                             # launch groups: two pairs, the odd full group, the ragged tail
    for name, env in (("pair0", {"RASS_SCAN_BATCH_PAIR": "0"}), ("floor0", {"RASS_SCAN_SAMPLE_FLOOR": "0"}),
                      ("floor_force", {"RASS_SCAN_SAMPLE_FLOOR": "force"})):
        got = _run_child(tmp_path, name, env)
        assert int(got["launches"]) == 6, name
        print("%s: %.3f ms of scan kernels per 165-query call (default %.3f)" % (name, float(got["ms"]), float(base["ms"])))
        if name == "pair0":
            # the pair kernel really runs by default: 4 of the 6 groups share two corpus passes instead of taking four, and
            # a 64-query pass is shorter than two 32-query passes (-14 %), so the call's scan time is lower
            assert float(base["ms"]) < float(got["ms"]), (float(base["ms"]), float(got["ms"]))
        assert np.array_equal(got["i"], base["i"]) and np.array_equal(got["s"], base["s"]), name


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
