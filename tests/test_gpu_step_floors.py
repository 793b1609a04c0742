"""One sample floor per query, computed once per batch call (sample_rep.hip, step_floors_kernel) for the step kernel
(scan_step.hip), where the other scans select it in every wave's prologue.

Through the parity hook ``rass_index_step_floors_device``, floor[q] must be a numpy restatement of that selection — the largest
value of the top 20 bits of the order-preserving score keys that at least k of the query's keys reach — over the 32 scores that
``rass_index_sample_floor_device`` returns for the same call; it is at most the k-th largest of them and below it by less than
2^-11 of its value; it is -inf where fewer than k of them are above -inf (a filter tag that is rare in, or absent from, the
sample).  And it is what the pair path selects in effect: the batch's results are bit-identical under RASS_SCAN_BATCH_STEP=0.

Shapes: 40 000 x 1024 with RASS_SCAN_SAMPLE_FLOOR=force (the smallest slab that takes the sample stage at 256 CUs), 64 queries
(one pair) and 1 024 (a full step).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR_BITS = 20     # scan_core.h, kFloorBits


def _score_key(s):
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _key_score(key):
    k = np.uint32(key)
    return (np.uint32(k ^ np.uint32(0x80000000)) if k & np.uint32(0x80000000) else np.uint32(~k)).view(np.float32)


def _floor_ref(scores32, k):
    keys = np.where(scores32 == -np.inf, np.uint32(0), _score_key(scores32))
    t = 0
    for b in range(31, 31 - FLOOR_BITS, -1):
        cand = t | (1 << b)
        if int((keys >= np.uint32(cand)).sum()) >= k:
            t = cand
    return _key_score(t) if t else np.float32(-np.inf)


@pytest.fixture(scope="module")
def case(gpu):
    from rassengine_amd.engine import Engine
    torch = gpu
    rng = np.random.default_rng(3)
    n, dim = 40_000, 1024
    x = rng.standard_normal((n, dim)).astype(np.float32)
    tags = rng.integers(1, 30, size=n).astype(np.int32)
    tags[[10, 700, 5_000, 9_000]] = 38          # rare in the sample: 4 rows of its 16 384
    tags[[20_000, 25_000, 39_000]] = 39         # absent from the sample
    eng = Engine(0, dim)
    eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
    ix = eng.open_index("floors")
    ix.add(x, tags=tags)
    ix.delete(5)
    old = os.environ.get("RASS_SCAN_SAMPLE_FLOOR")
    os.environ["RASS_SCAN_SAMPLE_FLOOR"] = "force"
    yield torch, eng, ix
    if old is None:
        os.environ.pop("RASS_SCAN_SAMPLE_FLOOR", None)
    else:
        os.environ["RASS_SCAN_SAMPLE_FLOOR"] = old
    eng.close()


def _filters(nq):
    f = np.random.default_rng(nq).integers(1, 30, size=nq).astype(np.int32)
    f[0] = -1
    f[3] = 38       # 4 representatives at the most
    f[7] = 39       # none
    f[40] = 4242    # a tag nobody carries
    f[nq - 1] = 39
    return f


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("nq", [64, 1024])
def test_floor_is_the_truncated_key_selection_of_the_32_scores(case, nq, k):
    torch, eng, ix = case
    g = torch.Generator(device="cuda")
    g.manual_seed(nq + k)
    q = torch.randn((nq, 1024), generator=g, device="cuda")
    for filt in (None, _filters(nq)):
        rows, scores = ix.sample_floor_device(q, k, q_filter=filt)
        floors = ix.step_floors_device(q, k, q_filter=filt).cpu().numpy()
        scores = scores.cpu().numpy()
        assert floors.shape == (nq,) and scores.shape == (nq, 32)
        want = np.array([_floor_ref(scores[qq], k) for qq in range(nq)], dtype=np.float32)
        assert np.array_equal(floors.view(np.uint32), want.view(np.uint32))
        finite = (scores > -np.inf).sum(axis=1)
        kth = -np.sort(-scores, axis=1)[:, k - 1]
        assert np.all(floors[finite < k] == -np.inf) and np.all(floors[finite >= k] > -np.inf)
        ok = finite >= k
        assert np.all(floors[ok] <= kth[ok])
        assert np.all(kth[ok] - floors[ok] <= np.abs(kth[ok]) * 2.0 ** -11)      # 20 of a key's 32 bits: 11 of the mantissa's 23
        if filt is not None:
            assert finite[3] <= 4 and finite[7] == 0 and finite[40] == 0 and finite[nq - 1] == 0
            assert floors[7] == -np.inf and floors[40] == -np.inf
            assert (floors[3] == -np.inf) == (k > finite[3])
        # what the pair path selects in effect: the same results, bit for bit, with one launch per pair
        df = None if filt is None else torch.from_numpy(filt).cuda()
        out = []
        for step in (None, "0"):
            s = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
            i = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if step is None:
                os.environ.pop("RASS_SCAN_BATCH_STEP", None)
            else:
                os.environ["RASS_SCAN_BATCH_STEP"] = step
            try:
                ix.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), d_q_filter_ptr=df.data_ptr() if df is not None else 0)
            finally:
                os.environ.pop("RASS_SCAN_BATCH_STEP", None)
            torch.cuda.synchronize()
            out.append((s.cpu().numpy().view(np.uint32), i.cpu().numpy()))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
