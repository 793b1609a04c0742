"""The pair kernel's ranking schedule (scan_topk_f32_pair_kernel: rank_load ahead of an MFMA chunk, rank_use behind it, the
registers of a part live across the chunk, two parts per slot at CH = 1) at the shapes where it can go wrong and that
tests/test_gpu_scan_pair.py does not force.  The yardstick is rass_index_search_device on consecutive 32-query groups (the
32-query kernel); ids and scores (as uint32) must be equal bit for bit, without and with the sample floor.

Shape: 24 593 rows = 768 full tiles (3 per workgroup at 256 workgroups) + a ragged last tile of 17 rows; dims 100 (CH = 1),
256 (CH = 2) and 1024 (CH = 8); 64 and 128 queries; k in {1, 10, 32}.

Corpora: row i = cos(t_i) u + sin(t_i) w_i with unit w_i orthogonal to u and to v; query j = +-u + e_j v.  So the exact score
of (query j, row i) is +-cos(t_i) / sqrt(1 + e_j^2): ONE order of the rows for every query.
  * ascending: t falls from 1.4 to 0.4 along the row index, score steps of >= sin(0.4) / 24 592 = 1.58e-5 (fp32 noise of a
    unit-vector dot product is ~1e-7): every row is a new best of every query, every lane inserts in every part of every tile
  * descending: the same rows in reverse order: only a workgroup's first tile inserts
  * alternating: odd queries are -u + e_j v: the two halves of a wave and the two groups of a pair see opposite corpora
  * filter: tags that only rows of the ragged last tile carry, per-query filters on them, tombstones in and out of that tile
The ascending case is also held against an fp64 ranking by the rule of test_gpu_scan_pair.py (every row that beats the fp64
k-th best by more than 1e-5 is reported); with the step above that set is exactly the k - 1 best rows, which is asserted on
the CPU before anything is searched.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 768 * 32 + 17
LAST_TILE = 768 * 32
T_HI, T_LO = 1.4, 0.4
KS = (1, 10, 32)
NQS = (64, 128)


def corpus(dim, seed):
    """(x ascending [N_ROWS, dim] float32, u, v): row i = cos(t_i) u + sin(t_i) w_i, t falling from T_HI to T_LO."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    v = rng.standard_normal(dim)
    v -= (v @ u) * u
    v /= np.linalg.norm(v)
    w = rng.standard_normal((N_ROWS, dim))
    w -= np.outer(w @ u, u)
    w -= np.outer(w @ v, v)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    t = np.linspace(T_HI, T_LO, N_ROWS)
    x = np.cos(t)[:, None] * u + np.sin(t)[:, None] * w
    return x.astype(np.float32), u, v


def queries(u, v, nq, alternating):
    e = 0.01 * (1.0 + np.arange(nq)) / nq
    sign = np.where((np.arange(nq) % 2 == 1) & alternating, -1.0, 1.0)
    return (sign[:, None] * u + e[:, None] * v).astype(np.float32)


def fp64_scores(x, q):
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    qh = q.astype(np.float64)
    return (qh / np.linalg.norm(qh, axis=1, keepdims=True)) @ xn.T


def must_report(S, k):
    """Per query: the rows that beat the fp64 k-th best by more than 1e-5 (the rule of test_gpu_scan_pair.py)."""
    kth = np.sort(S, axis=1)[:, -k]
    return [np.nonzero(S[row] > kth[row] + 1e-5)[0] for row in range(S.shape[0])]


def _per_group(torch, ix, q, k, filt=None):
    n = q.shape[0]
    s = torch.empty((n, k), dtype=torch.float32, device="cuda")
    i = torch.empty((n, k), dtype=torch.int64, device="cuda")
    for g in range(0, n, 32):
        ix.search_device(q[g:g + 32].data_ptr(), 32, k, s[g:g + 32].data_ptr(), i[g:g + 32].data_ptr(),
                         d_q_filter_ptr=filt[g:g + 32].data_ptr() if filt is not None else 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _batch(torch, ix, q, k, filt=None):
    n = q.shape[0]
    s = torch.empty((n, k), dtype=torch.float32, device="cuda")
    i = torch.empty((n, k), dtype=torch.int64, device="cuda")
    ix.search_device_batch(q.data_ptr(), n, k, s.data_ptr(), i.data_ptr(),
                           d_q_filter_ptr=filt.data_ptr() if filt is not None else 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _batch_equals(torch, ix, q, k, ref, what, filt=None):
    for mode in ("0", "force"):
        os.environ["RASS_SCAN_SAMPLE_FLOOR"] = mode
        try:
            assert _same(_batch(torch, ix, q, k, filt=filt), ref), (what, k, q.shape[0], mode)
        finally:
            os.environ.pop("RASS_SCAN_SAMPLE_FLOOR", None)


# Tags of the filter case: every row carries 1, the 17 rows of the ragged last tile 100 + (row % 3).
DEAD = (0, 31, 12_000, LAST_TILE + 2, LAST_TILE + 3, N_ROWS - 1)


@pytest.fixture(scope="module", params=[100, 256, 1024])
def slabs(gpu, request):
    """One engine per dim: the ascending corpus, its reverse, and the ascending corpus with tags and tombstones."""
    from rassengine_amd.engine import Engine
    torch = gpu
    dim = request.param
    x, u, v = corpus(dim, dim)
    tags = np.ones(N_ROWS, dtype=np.int32)
    tags[LAST_TILE:] = 100 + np.arange(LAST_TILE, N_ROWS) % 3
    eng = Engine(0, dim)
    eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
    asc = eng.open_index("asc")
    asc.add(x)
    desc = eng.open_index("desc")
    desc.add(x[::-1])
    filt = eng.open_index("filt")
    filt.add(x, tags=tags)
    for r in DEAD:
        filt.delete(r)
    assert asc.row_stride == (dim + 127) // 128 * 128
    yield torch, dim, x, u, v, tags, asc, desc, filt
    eng.close()


def test_ascending_corpus_every_lane_inserts(slabs):
    torch, dim, x, u, v, tags, asc, desc, filt = slabs
    for nq in NQS:
        qh = queries(u, v, nq, alternating=False)
        S = fp64_scores(x, qh)
        q = torch.from_numpy(qh).cuda()
        for k in KS:
            # the fp64 side first, on the CPU: the rows that must be reported are exactly the k - 1 last ones
            must = must_report(S, k)
            for row in range(nq):
                assert list(must[row]) == list(range(N_ROWS - k + 1, N_ROWS)), (k, row, must[row])
            ref = _per_group(torch, asc, q, k)
            for row in range(nq):
                assert set(must[row]) <= set(ref[1][row]), (k, row, ref[1][row])
            assert np.array_equal(ref[1], np.tile(np.arange(N_ROWS - 1, N_ROWS - 1 - k, -1), (nq, 1))), k
            _batch_equals(torch, asc, q, k, ref, "ascending")


def test_descending_corpus_only_the_first_tile_inserts(slabs):
    torch, dim, x, u, v, tags, asc, desc, filt = slabs
    for nq in NQS:
        q = torch.from_numpy(queries(u, v, nq, alternating=False)).cuda()
        for k in KS:
            ref = _per_group(torch, desc, q, k)
            assert np.array_equal(ref[1], np.tile(np.arange(k), (nq, 1))), k
            _batch_equals(torch, desc, q, k, ref, "descending")


def test_alternating_queries_see_opposite_corpora(slabs):
    torch, dim, x, u, v, tags, asc, desc, filt = slabs
    for nq in NQS:
        q = torch.from_numpy(queries(u, v, nq, alternating=True)).cuda()
        for k in KS:
            ref = _per_group(torch, asc, q, k)
            assert np.array_equal(ref[1][0::2], np.tile(np.arange(N_ROWS - 1, N_ROWS - 1 - k, -1), (nq // 2, 1))), k
            assert np.array_equal(ref[1][1::2], np.tile(np.arange(k), (nq // 2, 1))), k
            _batch_equals(torch, asc, q, k, ref, "alternating")


def test_filter_matching_only_the_ragged_last_tile(slabs):
    torch, dim, x, u, v, tags, asc, desc, filt = slabs
    live = np.ones(N_ROWS, dtype=bool)
    live[list(DEAD)] = False
    for nq in NQS:
        qf = np.array([(100, 101, 102, 999, -1)[j % 5] for j in range(nq)], dtype=np.int32)   # 999: no row carries it
        d_qf = torch.from_numpy(qf).cuda()
        for alternating in (False, True):
            q = torch.from_numpy(queries(u, v, nq, alternating)).cuda()
            for k in KS:
                ref = _per_group(torch, filt, q, k, filt=d_qf)
                for row in range(nq):
                    got = ref[1][row][ref[1][row] >= 0]
                    if qf[row] == 999:
                        assert got.size == 0, (k, row, got)
                    elif qf[row] >= 0:
                        want = np.nonzero(live & (tags == qf[row]))[0]      # 4 to 6 rows, all in the last tile
                        assert want.min() >= LAST_TILE and 4 <= want.size <= 6
                        best_first = want if (alternating and row % 2 == 1) else want[::-1]
                        assert list(got) == list(best_first[:k]), (k, row, got, want)
                    else:
                        assert got.size == k and np.all(live[got]), (k, row, got)
                _batch_equals(torch, filt, q, k, ref, "filter, alternating=%s" % alternating, filt=d_qf)
