"""The step kernel of the batched exact fp32 flat scan (scan_step.hip, scan_topk_f32_step_kernel: a run of up to 16 consecutive
query pairs in one launch, the pairs x tiles work items dealt round-robin to the workgroups).

rass_index_search_device_batch must equal, ids and score BITS, both itself under RASS_SCAN_BATCH_STEP=0 (one launch per pair,
the path it replaces; the switch is read per call) and rass_index_search_device on consecutive groups of 32 queries — without
the sample floor, with the default rule and with the floor forced (RASS_SCAN_SAMPLE_FLOOR, read per call).

Shapes, the smallest at which the item sequence can go wrong: 33 rows (2 tiles, 2 workgroups), 1 000 (32 tiles: fewer than
workgroups on a full device, the last one ragged), 8 200 (257 tiles: a remainder of one on 256 workgroups) and 40 000 (1 250
tiles: pairs x tiles no multiple of the grid, and the smallest slab that takes the sample stage when forced); 128 queries (two
pairs: the shortest run), 160 (pairs and an odd group), 165 (and a ragged tail), 1 024 (a full step: 16 pairs, one launch),
2 112 (33 pairs: two step launches and a single pair, which keeps the pair kernel); k = 1, 10, 32; dim 100, 512, 1 024
(CH = 1, 4, 8).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQS = (128, 160, 165, 1024, 2112)
KS = (1, 10, 32)
FLOOR_MODES = ("0", None, "force")   # RASS_SCAN_SAMPLE_FLOOR: off, the default rule, forced


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


def _batch(torch, ix, q, k, filt=None, id_base=0, step=True):
    n = q.shape[0]
    s = torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    i = torch.full((n, k), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with _Env(RASS_SCAN_BATCH_STEP=None if step else "0"):
        ix.search_device_batch(q.data_ptr(), n, k, s.data_ptr(), i.data_ptr(), id_base=id_base,
                               d_q_filter_ptr=filt.data_ptr() if filt is not None else 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _queries(torch, nq, dim, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn((nq, dim), generator=g, device="cuda")


def _check_all_paths(torch, ix, q, k, filt=None, id_base=0, what=""):
    """Step launches == one launch per pair == group by group, in every floor mode; returns the group-by-group answer."""
    ref = _per_group(torch, ix, q, k, filt=filt, id_base=id_base)
    for mode in FLOOR_MODES:
        with _Env(RASS_SCAN_SAMPLE_FLOOR=mode):
            got = _batch(torch, ix, q, k, filt=filt, id_base=id_base)
            assert _same(got, _batch(torch, ix, q, k, filt=filt, id_base=id_base, step=False)), (what, mode, "vs one launch per pair")
            assert _same(got, ref), (what, mode, "vs group by group")
    return ref


def _engine(torch, dim, name, x, tags=None, dead=()):
    from rassengine_amd.engine import Engine
    eng = Engine(0, dim)
    eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
    ix = eng.open_index(name)
    ix.add(x, tags=tags)
    for r in dead:
        ix.delete(int(r))
    return eng, ix


@pytest.mark.parametrize("dim", [100, 512, 1024])
@pytest.mark.parametrize("rows", [33, 1_000, 8_200, 40_000])
def test_step_equals_pair_launches_and_groups(gpu, rows, dim):
    torch = gpu
    rng = np.random.default_rng(rows * 7 + dim)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    dead = sorted({0, rows - 1, rows // 2})
    eng, ix = _engine(torch, dim, "step", x, dead=dead)
    try:
        q_all = _queries(torch, max(NQS), dim, rows + dim)
        for nq in NQS:
            q = q_all[:nq].contiguous()
            for k in KS:
                ref = _check_all_paths(torch, ix, q, k, what=(rows, dim, nq, k))
                assert np.all((ref[1] >= 0).sum(axis=1) == min(rows - len(dead), k)), (nq, k)
        if dim in (100, 1024):
            # and no row is lost by ALL paths alike: every row that beats the fp64 k-th best by more than fp32 noise is reported
            nq, k = 165, 10
            ref = _per_group(torch, ix, q_all[:nq].contiguous(), k)
            xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
            qh = q_all[:nq].cpu().numpy().astype(np.float64)
            S = (qh / np.linalg.norm(qh, axis=1, keepdims=True)) @ xn.T
            S[:, dead] = -np.inf
            kk = min(k, rows - len(dead))
            kth = np.sort(S, axis=1)[:, -kk]
            for row in range(nq):
                must = np.nonzero(S[row] > kth[row] + 1e-5)[0]
                assert set(must) <= set(ref[1][row]), (row, must, ref[1][row])
    finally:
        eng.close()


@pytest.fixture(scope="module")
def tagged(gpu):
    """40 000 x 1024 with tags: a rare tag on one row, tombstones in both 16-row blocks of a tile, across a tile boundary, a
    WHOLE tombstoned tile (rows 640..671) and the last row."""
    torch = gpu
    rng = np.random.default_rng(7)
    n, dim = 40_000, 1024
    x = rng.standard_normal((n, dim)).astype(np.float32)
    tags = rng.integers(1, 50, size=n).astype(np.int32)
    tags[12_345] = 777
    dead = [0, 15, 16, 31, 32, 20_000, 39_999] + list(range(640, 672))
    eng, ix = _engine(torch, dim, "step-tagged", x, tags=tags, dead=dead)
    yield torch, eng, ix, x, tags, dead
    eng.close()


def test_kernel_timing_counts_launch_groups(tagged):
    """bench.py's roofline line stays in launch-group units: a step launch over p pairs counts as 2 p groups, its time once."""
    torch, eng, ix = tagged[:3]
    for nq in NQS:
        q = _queries(torch, nq, 1024, nq)
        eng.kernel_timing_begin(256)
        _batch(torch, ix, q, 10)
        assert eng.kernel_timing_end()[1] == (nq + 31) // 32, nq


def test_tombstones_filters_and_id_base(tagged):
    torch, eng, ix, x, tags, dead = tagged
    nq = 165
    q = _queries(torch, nq, 1024, 99)
    filt = torch.randint(1, 50, (nq,), dtype=torch.int32, device="cuda")
    filt[3] = -1
    filt[40] = 777      # a tag on one row
    filt[41] = 9999     # a tag on none
    filt[70] = 777
    filt[130] = 9999
    filt[164] = 777
    ref = _check_all_paths(torch, ix, q, 10, filt=filt, id_base=7_000_000, what="filters")
    assert np.all(ref[1][41] == -1) and np.all(ref[1][130] == -1)
    for qq in (40, 70, 164):
        assert ref[1][qq, 0] == 7_000_000 + 12_345 and np.all(ref[1][qq, 1:] == -1)
    assert ref[1][3, 0] >= 7_000_000
    ref = _check_all_paths(torch, ix, q, 32, what="tombstones")
    assert not (set(ref[1].ravel()) & set(dead))


def test_strided_outputs(tagged):
    torch, eng, ix = tagged[:3]
    nq, k = 160, 10
    q = _queries(torch, nq, 1024, 4)
    ref = _per_group(torch, ix, q, k)
    ss, si = 32 * k + 24, 32 * k + 40       # group g's block of 32 * k at g * stride, the gaps untouched
    groups = nq // 32
    s = torch.full((groups * ss,), -7.0, dtype=torch.float32, device="cuda")
    i = torch.full((groups * si,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), out_scores_group_stride=ss, out_ids_group_stride=si)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy().reshape(groups, ss), i.cpu().numpy().reshape(groups, si)
    assert np.array_equal(s[:, :32 * k].reshape(nq, k).view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(i[:, :32 * k].reshape(nq, k), ref[1])
    assert np.all(s[:, 32 * k:] == -7.0) and np.all(i[:, 32 * k:] == -7)


def test_identical_rows_across_workgroups_tie_by_id(gpu):
    """7 distinct vectors in blocks of 100 identical rows: a block spans 4-5 tiles, which consecutive workgroups hold, and every
    score occurs ~5 700 times down the slab.  Ties resolve by ascending id, within a workgroup's list and across them."""
    torch = gpu
    rng = np.random.default_rng(11)
    n, dim, k = 40_000, 1024, 32
    base = rng.standard_normal((7, dim)).astype(np.float32)
    x = base[(np.arange(n) // 100) % 7]
    dead = [0, 7, 16, 23, 100, 131]
    eng, ix = _engine(torch, dim, "step-dups", x, dead=dead)
    try:
        q = _queries(torch, 160, dim, 8)
        s, i = _check_all_paths(torch, ix, q, k, what="ties")
        for row in range(160):
            assert np.all(s[row, 1:] <= s[row, :-1])
            eq = s[row, 1:] == s[row, :-1]
            assert np.all(i[row, 1:][eq] > i[row, :-1][eq])
            best = (i[row, 0] // 100) % 7            # the best vector's copies come first, smallest live ids first
            live = [r for r in range(1400) if (r // 100) % 7 == best and r not in dead][:k]
            assert list(i[row]) == live
    finally:
        eng.close()


def test_nan_row_and_zero_query(gpu):
    """A NaN row never ranks and a zero query ranks every live row at score 0 by ascending id, on every path alike."""
    torch = gpu
    rng = np.random.default_rng(13)
    n, dim, k = 8_200, 512, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[777, 5] = np.nan
    from rassengine_amd.engine import Engine
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        ix = eng.open_index("step-nan")
        ix.add(x, normalize=False)
        q = _queries(torch, 165, dim, 3)
        q[5] = 0.0
        q[100] = 0.0
        s, i = _check_all_paths(torch, ix, q, k, what="nan")
        assert 777 not in set(i.ravel())
        for qq in (5, 100):
            assert list(i[qq]) == [r for r in range(k + 1) if r != 777][:k] and np.all(s[qq] == 0.0)
        assert np.all(np.isfinite(s))
    finally:
        eng.close()
