"""The fused fp32 batch's sample stage (sample_rep.hip): bf16 MFMAs choose one representative row per (query, block of the
sample prefix), the fp32 fmaf chain scores it, and the k-th largest of a query's 32 scores is its floor.

Two kinds of checks, both against the CPU oracle's emulation of the scan's fmaf order (``KIND_F32_MFMA``) for the queries as the
GPU normalised them; no expectation comes from the engine:

* the parity hook ``rass_index_sample_floor_device``: every score is the oracle's score of its representative bit for bit,
  every representative lies in its block and may rank for its query, it is within ``2^-7 |q| max|x|`` of its block's best
  eligible row (twice the Cauchy-Schwarz bound of rounding both operands to bf16, 2 * 2^-8 |q| |x|: a wrong slot-to-column map
  misses the block maxima of ~0.1-0.3 by more than that at once), and a block without an eligible row reports -1 / -inf;
* the results of ``rass_index_search_device_batch``: ids and scores bit-identical under the default stage,
  ``RASS_SCAN_BATCH_SAMPLE=f32`` (the fp32 sample launch) and ``RASS_SCAN_SAMPLE_FLOOR=0`` (no floor), and equal to the ranking
  of the oracle's scores (score desc, row asc), on corpora that stress the choice of representatives.

Shapes: 40 000 rows (39 987 at dim 100: a ragged last tile) with ``RASS_SCAN_SAMPLE_FLOOR=force`` are the smallest that reach the
stage: a 16 384-row sample at 256 CUs, 512-row blocks.  64 queries (one pair of launch groups) and 96 (a pair and an odd group).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)


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


MODES = {
    "rep": dict(RASS_SCAN_SAMPLE_FLOOR="force", RASS_SCAN_BATCH_SAMPLE=None),
    "f32": dict(RASS_SCAN_SAMPLE_FLOOR="force", RASS_SCAN_BATCH_SAMPLE="f32"),
    "off": dict(RASS_SCAN_SAMPLE_FLOOR="0", RASS_SCAN_BATCH_SAMPLE=None),
}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


class Case:
    """One corpus on the GPU with its queries, filters and the oracle's score matrix: built once, never changed by a test."""

    def __init__(self, torch, oracle, name, n, dim, nq, seed, edit=None):
        from rassengine_amd import ops
        from rassengine_amd.engine import Engine
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.nq = n, dim, nq
        self.x = _unit(rng.standard_normal((n, dim), dtype=np.float32))
        self.tags = rng.integers(1, 40, size=n).astype(np.int32)
        self.q_raw = rng.standard_normal((nq, dim), dtype=np.float32) * 3.0     # un-normalised on purpose
        self.qfilter = None
        self.dead = np.zeros(0, dtype=np.int64)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.grid = min((n + 31) // 32, cus)
        assert self.grid % 32 == 0 and n >= 2 * 64 * self.grid, "the shapes of this file assume the sample stage is taken"
        self.block = 2 * self.grid
        if edit is not None:
            edit(self, rng)
        self.eng = Engine(0, dim)
        self.ix = self.eng.open_index("sample-rep-" + name)
        self.ix.add(self.x, tags=self.tags, normalize=False)
        for r in self.dead:
            self.ix.delete(int(r))
        self.tags_live = self.tags.copy()
        self.tags_live[self.dead] = -1
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        with np.errstate(all="ignore"):
            self.scores = oracle.scores(self.x, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)

    def eligible(self, q):
        ok = self.tags_live != -1
        if self.qfilter is not None and self.qfilter[q] >= 0:
            ok = ok & (self.tags_live == self.qfilter[q])
        return ok

    def expect(self, k):
        """The flat scan's answer from the oracle's scores: eligible rows with a score above -inf, (score desc, row asc)."""
        es = np.full((self.nq, k), NEG_INF, dtype=np.float32)
        ei = np.full((self.nq, k), -1, dtype=np.int64)
        for q in range(self.nq):
            s = self.scores[q]
            with np.errstate(all="ignore"):
                rows = np.flatnonzero(self.eligible(q) & (s > NEG_INF))    # (a NaN compares false)
            if len(rows) > 4 * k:   # the k best are among the rows at or above the k-th largest score
                kth = np.partition(s[rows], len(rows) - k)[len(rows) - k]
                rows = rows[s[rows] >= kth]
            order = np.lexsort((rows, -s[rows]))[:k]
            es[q, :len(order)], ei[q, :len(order)] = s[rows[order]], rows[order]
        return es, ei

    def search(self, torch, k, mode):
        dq = torch.from_numpy(self.q_raw).cuda()
        df = None if self.qfilter is None else torch.from_numpy(self.qfilter).cuda()
        s = torch.full((self.nq, k), 7.0, dtype=torch.float32, device="cuda")
        i = torch.full((self.nq, k), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                        # the engine works on its own stream
        with _Env(**MODES[mode]):
            self.ix.search_device_batch(dq.data_ptr(), self.nq, k, s.data_ptr(), i.data_ptr(),
                                        d_q_filter_ptr=df.data_ptr() if df is not None else 0)
        self.eng.synchronize()
        return s.cpu().numpy(), i.cpu().numpy()

    def hook(self, torch, k):
        with _Env(**MODES["rep"]):
            rows, scores = self.ix.sample_floor_device(torch.from_numpy(self.q_raw).cuda(), k, q_filter=self.qfilter)
        return rows.cpu().numpy(), scores.cpu().numpy()


# ---- the corpora ------------------------------------------------------------------------------------------------------------

def _edit_filters_and_tombstones(c, rng):
    """Block 3 of the sample wholly tombstoned, 300 scattered tombstones, and per-query filters: none, a common tag, a tag that
    is rare in the sample (8 rows of it, in 5 blocks), one that only rows outside the sample carry, one nobody carries."""
    c.tags[c.tags >= 38] = 1
    rare = np.array([10, 700, 701, 5000, 5001, 5002, 9000, 16_000])
    c.tags[rare] = 38
    c.tags[np.array([20_000, 25_000, 39_000])] = 38
    c.tags[np.arange(30_000, 30_020)] = 39
    c.dead = np.unique(np.concatenate([np.arange(3 * c.block, 4 * c.block), rng.choice(c.n, 300, replace=False)]))
    c.dead = c.dead[~np.isin(c.dead, rare)]
    f = rng.integers(1, 38, size=c.nq).astype(np.int32)
    f[0::4] = -1
    f[1], f[2], f[3] = 38, 39, 1000
    c.qfilter = f


def _edit_twice(c, rng):
    """Every row stored twice, one copy inside the sample and one outside it, and adjacent copies inside a block."""
    c.x[20_000:36_000] = c.x[:16_000]
    c.x[1:8_000:2] = c.x[0:8_000:2]
    c.q_raw[5] = c.x[100] * 2.0


def _edit_cluster(c, rng):
    """64 sample rows within 1e-4 of one direction (bf16, 8 significant bits, cannot order them), which four queries aim at."""
    v = c.x[0].copy()
    c.x[1000:1064] = _unit(v[None, :] + 1e-4 * rng.standard_normal((64, c.dim), dtype=np.float32))
    c.q_raw[:4] = v[None, :] + 1e-3 * rng.standard_normal((4, c.dim), dtype=np.float32)


def _edit_zero_query(c, rng):
    c.q_raw[7] = 0.0


def _edit_nan_inf(c, rng):
    """One NaN row and one +Inf row inside the sample (neither may become a floor, and a NaN never ranks)."""
    c.x[2222, 5] = np.nan
    c.x[4444, 9] = np.inf


CASES = {
    # name: (rows, dim, queries, seed, edit)
    "iid100": (39_987, 100, 96, 11, _edit_filters_and_tombstones),
    "iid384": (40_000, 384, 64, 12, _edit_filters_and_tombstones),
    "iid1024": (40_000, 1024, 96, 13, _edit_filters_and_tombstones),
    "plain": (40_000, 256, 64, 14, None),
    "twice": (40_000, 256, 64, 15, _edit_twice),
    "cluster": (40_000, 256, 64, 16, _edit_cluster),
    "zero": (40_000, 256, 64, 17, _edit_zero_query),
    "naninf": (40_000, 256, 64, 18, _edit_nan_inf),
}
CASES.update({"stride%d" % d: (40_000, d, 64, 100 + d, None) for d in range(128, 1025, 128)})


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    built = {}

    def get(name):
        if name not in built:
            n, dim, nq, seed, edit = CASES[name]
            built[name] = Case(gpu, oracle, name, n, dim, nq, seed, edit)
        return built[name]

    yield get
    for c in built.values():
        c.eng.close()


# ---- the parity hook ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["iid100", "iid384", "iid1024"])
def test_hook_representatives_and_scores(gpu, cases, name):
    c = cases(name)
    rows, scores = c.hook(gpu, 10)
    assert rows.shape == (c.nq, 32) and scores.shape == (c.nq, 32)
    bound = 2.0 ** -7 * np.abs(c.x[:32 * c.block]).max()      # |q| = 1, max|x| <= 1
    worst, empty = 0.0, 0
    for q in range(c.nq):
        ok = c.eligible(q)
        for b in range(32):
            lo, hi = b * c.block, (b + 1) * c.block
            r = int(rows[q, b])
            if not ok[lo:hi].any():
                assert r == -1 and scores[q, b] == NEG_INF, (q, b)
                empty += 1
                continue
            assert lo <= r < hi and ok[r], (q, b, r)
            assert scores[q, b].view(np.uint32) == c.scores[q, r].view(np.uint32), (q, b, r)
            gap = float(c.scores[q, lo:hi][ok[lo:hi]].max()) - float(scores[q, b])
            worst = max(worst, gap)
            assert gap <= bound, (q, b, r, gap)
    print("%s: worst block maximum - representative = %.3e (bound %.3e), %d empty (query, block) pairs" % (name, worst, bound, empty))
    assert empty >= c.nq // 4      # block 3 is tombstoned for everyone; the rare and absent tags leave most blocks empty


def test_hook_refuses_what_the_batch_would_not_sample(gpu, cases):
    from rassengine_amd import _native as N
    c = cases("plain")
    q = gpu.from_numpy(c.q_raw).cuda()
    for env in (dict(RASS_SCAN_SAMPLE_FLOOR="0"), dict(RASS_SCAN_SAMPLE_FLOOR="force", RASS_SCAN_BATCH_SAMPLE="f32"),
                dict(RASS_SCAN_SAMPLE_FLOOR="force", RASS_SCAN_BATCH_SAMPLE="groups")):
        with _Env(**env), pytest.raises(N.RassError):
            c.ix.sample_floor_device(q, 10)
    with _Env(**MODES["rep"]), pytest.raises(N.RassError):
        c.ix.sample_floor_device(q[:40].contiguous(), 10)       # a ragged last group samples group by group


# ---- the results -------------------------------------------------------------------------------------------------------------

def _check_results(torch, c, k):
    es, ei = c.expect(k)
    got = {m: c.search(torch, k, m) for m in MODES}
    for m in ("f32", "off"):
        assert np.array_equal(got[m][1], got["rep"][1]), m
        assert np.array_equal(got[m][0].view(np.uint32), got["rep"][0].view(np.uint32)), m
    s, i = got["rep"]
    assert np.array_equal(i, ei)
    assert np.array_equal(s.view(np.uint32), es.view(np.uint32))


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("name", ["iid1024", "iid100", "plain", "twice", "cluster", "zero", "naninf"])
def test_results_identical_and_equal_to_oracle(gpu, cases, name, k):
    _check_results(gpu, cases(name), k)


@pytest.mark.parametrize("dim", list(range(128, 1025, 128)))
def test_every_stride(gpu, cases, dim):
    _check_results(gpu, cases("stride%d" % dim), 10)
