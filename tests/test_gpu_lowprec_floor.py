"""The sample floor of the bf16 and int8 scans (scan_bf16.hip / scan_i8.hip prologues, api_internal.h sample_prelaunch,
api_scan.hip i8_sample_floor) and the bf16 scan at every stride it is built for (256 / 512 / 768 / 1024 = CHB 1..4).

A sample launch over the slab's first 64 * grid rows gives each query one best score per workgroup; the k-th largest of them
is a score k rows reach, and the scan drops rows below it before the sorted insertion.  It must never change a result.  Here:
RASS_I8_SAMPLE_FLOOR = 0 / force / 1 (read at every call) return the same ids and score bits, and the forced result equals the
CPU oracle — the fp64 ranking of the bf16-rounded operands for the bf16 scans (ids up to ties, scores within TOL, the
yardstick of test_gpu_bf16_corpus.py), oracle.candidates_i8 bit for bit for the int8 scan, and the prefilter-off flat scan of
the same index for the re-ranked answers.

The corpus (40 000 rows: the smallest at which the forced floor engages on a 256-CU part — grid 256, sample 16 384 rows,
limit 32 768) carries the traps relative to the sample (sample workgroup g scans rows 64g .. 64g + 63):
  * rows 30 000 .. 30 399 duplicate sample rows 100 .. 499: exact ties with scores the floor is made of;
  * ~20 rows per patient (rare in the sample); patient 5 owns rows 0 .. 63 (one sample tile), patient 6 only rows
    20 000 .. 20 039 (outside the sample), patient 9 owns 30 % of all rows (a filter under which the floor really engages),
    99 999 matches nothing;
  * ~50 tombstones, some in the sample prefix, one a duplicated sample row, one the last row;
  * three planted directions u10 / u24 / u32 with exactly k = 10 / 24 / 32 near-copies (cosine 0.98 .. 0.71, distinct), one
    per sample tile in k different tiles and nowhere else, every other row far below: the top-k of such a query is exactly
    its planted rows and the floor is the score of the lowest of them — a floor one rank too high loses that row.  (32 of
    them because the candidate scans of the prefilter modes keep 32 entries whatever the caller's k.)
Every test asserts that the floor's size rule holds on the part it runs on, instead of passing with the floor off."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 2e-6                       # tests/test_gpu_bf16_corpus.py's, measured at 1 024 columns: fewer columns cannot need more
N = 40_000
BF16_DIMS = [200, 512, 700, 1024]     # strides 256 / 512 / 768 / 1024; 200 and 700 end inside a 32-column chunk
I8_DIMS = [384, 1024, 1536]           # int8 strides 512 / 1024 / 1536
MODES = ("0", "force", "1")
PM, DM = 0x00FFFFFF, 0x7F000000
P5, P6, P9, P9B, NOBODY = 5 | (1 << 24), 6 | (1 << 24), 9 | (1 << 24), 9 | (2 << 24), 99_999
PLANT_AT = {24: (0, 9, 20), 32: (1, 10, 16, 29), 10: (2, 40)}     # query positions of the planted directions


class _Floor:
    def __init__(self, mode):
        self.mode = mode          # None: the variable unset (the default rule)

    def __enter__(self):
        self.old = os.environ.get("RASS_I8_SAMPLE_FLOOR")
        if self.mode is None:
            os.environ.pop("RASS_I8_SAMPLE_FLOOR", None)
        else:
            os.environ["RASS_I8_SAMPLE_FLOOR"] = self.mode

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("RASS_I8_SAMPLE_FLOOR", None)
        else:
            os.environ["RASS_I8_SAMPLE_FLOOR"] = self.old


def _swaps_are_ties(i_gpu, i_ref, all64):
    for q in range(i_ref.shape[0]):
        for a, b in zip(i_gpu[q], i_ref[q]):
            if a != b and (a < 0 or b < 0 or abs(all64[q, a] - all64[q, b]) > 2 * TOL):
                return False
    return True


def _bf16_round(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _grid(torch, n, kept):
    """Workgroups of a scan of n rows that keeps `kept` entries per workgroup (api_scan.hip scan_grid)."""
    return min(-(-n // 64), torch.cuda.get_device_properties(0).multi_processor_count, 8192 // kept)


def _assert_forced_floor_engages(torch, n, kept):
    grid = _grid(torch, n, kept)
    assert grid <= 256 and n >= 2 * 64 * grid, f"the forced floor does not engage: {n} rows, grid {grid}"


def _same_bits(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


class _Corpus:
    def __init__(self, torch, oracle, dim):
        from rassengine_amd.engine import Engine
        self.torch, self.oracle, self.dim = torch, oracle, dim
        rng = np.random.default_rng(1000 + dim)
        x = rng.standard_normal((N, dim)).astype(np.float32)
        x[30_000:30_400] = x[100:500]
        self.plants = {}
        for k, tile0, step, off in ((10, 10, 20, 7), (24, 11, 10, 33), (32, 12, 7, 50)):     # tiles 10 .. 241: sample tiles
            u = rng.standard_normal(dim)
            u /= np.linalg.norm(u)
            rows = 64 * (tile0 + step * np.arange(k)) + off
            for j, r in enumerate(rows):
                e = rng.standard_normal(dim)
                e -= (e @ u) * u
                e /= np.linalg.norm(e)
                x[r] = ((u + (0.2 + 0.8 * j / (k - 1)) * e) * rng.uniform(0.5, 3.0)).astype(np.float32)   # cos 0.98 .. 0.71
            self.plants[k] = (u.astype(np.float32), rows)
        planted = np.concatenate([r for _, r in self.plants.values()])
        assert len(set(planted.tolist())) == 66 and planted.min() >= 500 and planted.max() < 64 * 256
        patient = rng.integers(1000, 3000, size=N).astype(np.int32)
        patient[rng.random(N) < 0.3] = 9
        doctype = rng.integers(1, 3, size=N).astype(np.int32)
        patient[:64], doctype[:64] = 5, 1
        patient[20_000:20_040], doctype[20_000:20_040] = 6, 1
        self.tags = (patient | (doctype << 24)).astype(np.int32)
        keep = set(planted.tolist()) | {120, 30_020}
        dead = [int(r) for r in rng.choice(N, 60, replace=False) if int(r) not in keep][:46]
        self.dead = sorted(set(dead) | {3, 130, 16_383, N - 1})
        self.tags_live = self.tags.copy()
        self.tags_live[self.dead] = -1
        self.x = x
        self.eng = Engine(0, dim)
        self.f32 = self._index("f32", "f32")
        self.xn = self.f32.get_rows(0, N)               # the stored fp32 rows: what the converters and the quantiser saw
        self._b16 = None
        # 45 queries; their prefixes of 1 / 16 / 17 / 32 are the smaller batches (one reference serves them all)
        q = rng.standard_normal((45, dim)).astype(np.float32)
        for k, at in PLANT_AT.items():
            for j, p in enumerate(at):
                q[p] = self.plants[k][0] * (1.0 + j)
        q[3] = x[120] * 3.0            # best rows: a sample row and its duplicate outside the sample
        q[4] = x[N - 1]                # the last row is a tombstone
        self.q = q
        qf = self.tags[rng.integers(0, N, size=45)].astype(np.int32)
        qf[[p for at in PLANT_AT.values() for p in at]] = -1
        qf[3:8] = P5, P6, NOBODY, P9, P9B
        qf[17:20] = P9, P5, P6
        qf[30], qf[41] = NOBODY, P9
        self.qf = qf
        self.qm = np.full(45, PM, dtype=np.int32)        # the masked variant: patient only, one query by doc type only
        self.qfm = np.where(qf < 0, -1, qf & PM).astype(np.int32)
        self.qm[8], self.qfm[8] = DM, 1 << 24
        self._cache = {}

    def _index(self, name, dtype):
        ix = self.eng.open_index(name, dtype=dtype)
        ix.add(self.x, tags=self.tags)
        for r in self.dead:
            ix.delete(r)
        return ix

    @property
    def b16(self):
        if self._b16 is None:
            self._b16 = self._index("b16", "bf16")
            # a bf16 corpus stores bf16(the fp32 index's row): one reference serves the corpus and the mode-1 candidates
            assert np.array_equal(self._b16.get_rows(0, N), self.xb)
        return self._b16

    @property
    def xb(self):
        if "xb" not in self._cache:
            self._cache["xb"] = _bf16_round(self.xn)
        return self._cache["xb"]

    def filters(self, kind, nq=45):
        """(q_filter, q_filter_mask) of the GPU call and the oracle's (tags, qfilter, qmask)."""
        if kind == "none":
            return (None, None), dict(tags=np.where(self.tags_live == -1, -1, 0).astype(np.int32))
        if kind == "plain":
            return (self.qf[:nq], None), dict(tags=self.tags_live, qfilter=self.qf[:nq])
        return (self.qfm[:nq], self.qm[:nq]), dict(tags=self.tags_live, qfilter=self.qfm[:nq], qmask=self.qm[:nq])

    def qn_gpu(self):
        """The queries as the engine normalises them (within 2 ulp of numpy's, which can cross a bf16 rounding boundary)."""
        if "qn" not in self._cache:
            from rassengine_amd import ops
            t = self.torch
            self._cache["qn"] = ops.normalize_rows(t.from_numpy(self.q).cuda()).cpu().numpy()
        return self._cache["qn"]

    def ref_bf16(self, kind, nq=32, k=32):
        """fp64 oracle on the bf16-rounded rows and queries: (scores [nq, k], ids, all scores [nq, N]); computed once."""
        key = ("bf16", kind, nq, k)
        if key not in self._cache:
            O = self.oracle
            qb = _bf16_round(self.qn_gpu()[:nq])
            rs, ri = O.search(self.xb, qb, k, kind=O.KIND_F64, **self.filters(kind, nq)[1])
            if ("all64", nq) not in self._cache:
                self._cache[("all64", nq)] = O.scores(self.xb, qb)
            self._cache[key] = (rs, ri, self._cache[("all64", nq)])
            self._assert_planted(ri, rs, nq, k)
        return self._cache[key]

    def _assert_planted(self, ri, rs, nq, k_ref):
        """The corpus's own precondition, from the oracle alone: the top-k of a planted query is its k planted rows, distinct
        in score at the low end, and the next row is far below."""
        for k, at in PLANT_AT.items():
            rows = set(self.plants[k][1].tolist())
            for p in at:
                if p < nq and k <= k_ref:
                    assert set(ri[p, :k].tolist()) == rows, (k, p)
                    assert rs[p, k - 2] - rs[p, k - 1] > 1e-3
                    if k < k_ref:
                        assert rs[p, k - 1] - rs[p, k] > 0.2, (k, p, rs[p, k - 1], rs[p, k])

    def ref_i8(self, kind, nq=32, n_cand=32):
        key = ("i8", kind, nq, n_cand)
        if key not in self._cache:
            O = self.oracle
            kw = self.filters(kind, nq)[1]
            self._cache[key] = O.candidates_i8(self.xn, O.normalize_c(self.q[:nq]), n_cand, tags=kw["tags"], qfilter=kw.get("qfilter"))
        return self._cache[key]

    def topk_inside_candidates(self, mode, kind, k=16):
        """Proved on the CPU, from the oracle alone: for every one of the 45 queries, every row of the exact top-k (and every
        row tying with its last within the fp32 error) is inside the oracle's candidate top-32 on the rounded (mode bf16) or
        quantised (mode int8) operands, clear of the list's end.  Only then must the re-ranked answer equal the flat scan's."""
        key = ("inside", mode, kind)
        if key not in self._cache:
            O = self.oracle
            kw = self.filters(kind)[1]
            if mode == "bf16":
                qn = self.qn_gpu()
                cs, ci = O.search(self.xb, _bf16_round(qn), 33, kind=O.KIND_F64, **kw)
                margin = 2 * TOL
            else:
                qn = O.normalize_c(self.q)
                cs, ci = O.candidates_i8(self.xn, qn, 33, tags=kw["tags"], qfilter=kw.get("qfilter"))
                cs, margin = cs.astype(np.float64), 0.0
            fs, fi = O.search(self.xn, qn, k + 8, kind=O.KIND_F64, **kw)
            left_out = 0
            for q in range(45):
                # (scores descend: what k = 16 needs includes what every smaller k needs)
                need = [int(r) for s, r in zip(fs[q], fi[q]) if r >= 0 and s >= fs[q, k - 1] - 2 * TOL]
                assert len(need) < k + 8                      # the tie group at the k-th place ends inside what was asked for
                end = cs[q, 32]                                # -inf: fewer than 33 rows match, nothing can be cut off
                for r in need:
                    at = np.flatnonzero(ci[q, :32] == r)
                    left_out += 0 if len(at) == 1 and cs[q, at[0]] > end + margin else 1
            self._cache[key] = left_out
        return self._cache[key]

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def corpora(gpu, oracle):
    """One corpus per dimension, built when the first test asks for it and shared, with its references, by the rest."""
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = _Corpus(gpu, oracle, dim)
        return made[dim]
    yield get
    for c in made.values():
        c.close()


def _three_ways(call):
    out = {}
    for mode in MODES:
        with _Floor(mode):
            out[mode] = call()
    for mode in ("force", "1"):
        assert _same_bits(out[mode], out["0"]), mode
    return out["force"]


def _check_against_bf16_oracle(s, i, rs, ri, all64, what):
    assert _swaps_are_ties(i, ri, all64), what
    valid = ri >= 0
    assert np.array_equal(i >= 0, valid), what
    assert np.all(np.isneginf(s[~valid])), what
    got = np.take_along_axis(all64, np.clip(i, 0, None), 1)
    err = np.abs(s[valid].astype(np.float64) - got[valid])
    assert np.all(err <= TOL), (what, err.max())


# ---- a. the bf16 corpus, flat
@pytest.mark.parametrize("kind", ["none", "plain", "masked"])
@pytest.mark.parametrize("dim", BF16_DIMS)
def test_bf16_corpus_matches_oracle_with_every_floor_setting(corpora, dim, kind):
    """k = 24 and 32 run with the floor (plain filters keep it, masks are the EXT variant without one), k = 10 is the
    control without; 1 / 16 / 17 / 32 queries = NT 1 and 2 and both half-waves of the query map."""
    c = corpora(dim)
    _assert_forced_floor_engages(c.torch, N, 24)
    _assert_forced_floor_engages(c.torch, N, 32)
    rs, ri, all64 = c.ref_bf16(kind)
    ix = c.b16
    for nq in (1, 16, 17, 32):
        (f, m), _ = c.filters(kind, nq)
        for k in (10, 24, 32):
            s, i = _three_ways(lambda: ix.search(c.q[:nq], k, q_filter=f, q_filter_mask=m))
            _check_against_bf16_oracle(s, i, rs[:nq, :k], ri[:nq, :k], all64[:nq], (c.dim, kind, nq, k))
            for p in PLANT_AT[k]:
                if p < nq:
                    assert set(i[p].tolist()) == set(c.plants[k][1].tolist()), (c.dim, kind, nq, k, p)
    if kind == "none":
        assert list(i[3, :2]) == [120, 30_020] and s[3, 0] == s[3, 1]        # exact ties come back id-ascending
        assert N - 1 not in i[4]
    else:
        patient = c.tags & PM
        assert np.all(patient[i[3]] == 5) and np.all(patient[i[4]] == 6) and np.all(patient[i[6]] == 9)
        assert np.all(i[5] == -1) and np.all(i[30] == -1)
        assert set(i[4][i[4] >= 0].tolist()) <= set(range(20_000, 20_040))


# ---- b. bf16 prefilter (mode 1): the candidate lists
@pytest.mark.parametrize("kind", ["none", "plain"])
@pytest.mark.parametrize("dim", BF16_DIMS)
def test_bf16_candidates_match_oracle_with_every_floor_setting(corpora, dim, kind):
    c = corpora(dim)
    t = c.torch
    _assert_forced_floor_engages(t, N, 32)
    rs, ri, all64 = c.ref_bf16(kind)
    c.f32.set_prefilter("bf16")
    try:
        for nq in (1, 16, 17, 32):
            (f, _), _ = c.filters(kind, nq)
            qd = t.from_numpy(c.q[:nq]).cuda().contiguous()

            def cand():
                s, r = c.f32.candidates_device(qd, f)
                return s.cpu().numpy(), r.cpu().numpy()
            s, r = _three_ways(cand)
            _check_against_bf16_oracle(s, r, rs[:nq], ri[:nq], all64[:nq], (c.dim, kind, nq))
            for p in PLANT_AT[32]:
                if p < nq:
                    assert set(r[p].tolist()) == set(c.plants[32][1].tolist()), (c.dim, kind, nq, p)
        if kind == "plain":
            assert np.all(r[5] == -1) and np.all(np.isneginf(s[5]))              # a filter that matches nothing
            short = 0                                                             # filters that match fewer than 32 rows
            for p in range(32):
                n_match = int(np.sum(c.tags_live == c.qf[p])) if c.qf[p] >= 0 else N
                if n_match < 32:
                    short += n_match > 0
                    assert np.all(r[p, :n_match] >= 0) and np.all(r[p, n_match:] == -1) and np.all(np.isneginf(s[p, n_match:]))
            assert short >= 5
    finally:
        c.f32.set_prefilter(False)


# ---- c. bf16 and int8 prefilter: the re-ranked answers
PREFILTER_CASES = [(d, "bf16") for d in BF16_DIMS] + [(d, "int8") for d in I8_DIMS]


@pytest.mark.parametrize("kind", ["none", "plain"])
@pytest.mark.parametrize("dim,mode", PREFILTER_CASES)
def test_prefilter_answers_equal_the_flat_scan_with_every_floor_setting(corpora, dim, mode, kind):
    """Equal ids and score bits, as tests/test_gpu_prefilter.py asserts at 1 024 columns — which holds where the exact top-k
    lies inside the candidate top-32: proved first, for all 45 queries (none left out), from the oracle alone."""
    c = corpora(dim)
    _assert_forced_floor_engages(c.torch, N, 32)
    assert c.topk_inside_candidates(mode, kind) == 0
    ix = c.f32
    try:
        for nq in (1, 17, 32, 45):
            (f, _), _ = c.filters(kind, nq)
            for k in (1, 10, 16):
                ix.set_prefilter(False)
                flat = ix.search(c.q[:nq], k, q_filter=f)
                ix.set_prefilter(mode)
                got = _three_ways(lambda: ix.search(c.q[:nq], k, q_filter=f))
                assert np.array_equal(got[1], flat[1]), (c.dim, mode, kind, nq, k)
                assert np.array_equal(got[0], flat[0]), (c.dim, mode, kind, nq, k)
                if k == 10:
                    for p in PLANT_AT[10]:
                        if p < nq:
                            assert set(got[1][p].tolist()) == set(c.plants[10][1].tolist())
    finally:
        ix.set_prefilter(False)


# ---- d. int8 candidates with the floor on
@pytest.mark.parametrize("kind", ["none", "plain"])
@pytest.mark.parametrize("dim", I8_DIMS)
def test_int8_candidates_equal_the_oracle_bit_for_bit_with_the_floor_on(corpora, dim, kind):
    """test_int8_candidates_equal_the_oracle_bit_for_bit's comparison at a size where the floor engages."""
    c = corpora(dim)
    t = c.torch
    _assert_forced_floor_engages(t, N, 32)
    s_o, r_o = c.ref_i8(kind)
    for p in PLANT_AT[32]:                  # the corpus's precondition on the quantised operands
        assert set(r_o[p].tolist()) == set(c.plants[32][1].tolist()) and s_o[p, 30] > s_o[p, 31]
    c.f32.set_prefilter("int8")
    try:
        for nq in (1, 16, 17, 32):
            (f, _), _ = c.filters(kind, nq)
            qd = t.from_numpy(c.q[:nq]).cuda().contiguous()

            def cand():
                s, r = c.f32.candidates_device(qd, f)
                return s.cpu().numpy(), r.cpu().numpy()
            s, r = _three_ways(cand)
            assert np.array_equal(r, r_o[:nq]), (c.dim, kind, nq)
            assert np.array_equal(s.view(np.uint32), s_o[:nq].view(np.uint32)), (c.dim, kind, nq)
    finally:
        c.f32.set_prefilter(False)


# ---- e. the batch path
def _device_search(c, ix, qd, k, fd, batch, gs=0, gi=0):
    """search_device_batch (batch) or search_device group by group -> ([nq, k] scores, ids) on the host."""
    t = c.torch
    nq = qd.shape[0]
    groups = (nq + 31) // 32
    s = t.full((groups * (gs or 32 * k),), float("nan"), dtype=t.float32, device="cuda")
    i = t.full((groups * (gi or 32 * k),), -7, dtype=t.int64, device="cuda")
    t.cuda.synchronize()
    if batch:
        ix.search_device_batch(qd.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), d_q_filter_ptr=fd.data_ptr() if fd is not None else 0,
                               out_scores_group_stride=gs, out_ids_group_stride=gi)
    else:
        for g in range(groups):
            b = min(32, nq - 32 * g)
            ix.search_device(qd[32 * g:].data_ptr(), b, k, s[g * 32 * k:].data_ptr(), i[g * 32 * k:].data_ptr(),
                             d_q_filter_ptr=fd[32 * g:].data_ptr() if fd is not None else 0)
    c.eng.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    out_s = np.concatenate([s[g * (gs or 32 * k):][:32 * k] for g in range(groups)])[:nq * k].reshape(nq, k)
    out_i = np.concatenate([i[g * (gi or 32 * k):][:32 * k] for g in range(groups)])[:nq * k].reshape(nq, k)
    assert not np.any(out_i == -7)          # every slot was written
    return out_s, out_i


@pytest.mark.parametrize("dim,mode", PREFILTER_CASES)
def test_prefilter_batch_equals_group_by_group_and_the_flat_scan(corpora, dim, mode):
    """search_device_batch on a mode-1 / mode-2 index: 64 and 128 queries (int8: ONE grouped sample launch for all groups), 70
    (a sample launch per group, a ragged last group of 6).  Bit-identical to the groups sent one by one, to floor mode 0,
    and to the flat scan of the same index (the 45 queries of the proof above, repeated)."""
    c = corpora(dim)
    t = c.torch
    _assert_forced_floor_engages(t, N, 32)
    k = 10
    ix = c.f32
    reps = np.arange(128) % 45
    try:
        for kind in ("none", "plain"):
            assert c.topk_inside_candidates(mode, kind) == 0
            for nq in (64, 128, 70):
                qd = t.from_numpy(c.q[reps[:nq]]).cuda().contiguous()
                fd = t.from_numpy(c.qf[reps[:nq]]).cuda().contiguous() if kind == "plain" else None
                ix.set_prefilter(False)
                flat = _device_search(c, ix, qd, k, fd, batch=True)
                ix.set_prefilter(mode)
                got = _three_ways(lambda: _device_search(c, ix, qd, k, fd, batch=True))
                one = _three_ways(lambda: _device_search(c, ix, qd, k, fd, batch=False))
                assert _same_bits(got, one), (c.dim, mode, kind, nq)
                assert _same_bits(got, flat), (c.dim, mode, kind, nq)
                for p in PLANT_AT[10]:
                    assert set(got[1][p].tolist()) == set(c.plants[10][1].tolist())
        with _Floor("force"):          # the strided-output form, once: the last round's 70 filtered queries
            strided = _device_search(c, ix, qd, k, fd, batch=True, gs=32 * k + 64, gi=32 * k + 32)
        assert _same_bits(strided, got), (c.dim, mode)
    finally:
        ix.set_prefilter(False)


# ---- f. the default rule engages where it says
def test_default_rule_engages_at_eight_samples(gpu, oracle):
    """8 * 64 * grid + 37 synthetic rows at 256 columns: RASS_I8_SAMPLE_FLOOR unset (the floor on by its own rule) against
    = 0, bit for bit — the bf16 corpus at k = 32, the mode-1 and mode-2 candidates and answers; the bf16 corpus also against
    the oracle on the stored rows."""
    from rassengine_amd import ops
    from rassengine_amd.engine import Engine
    t = gpu
    dim = 256
    grid = _grid(t, 1 << 30, 32)
    n = 8 * 64 * grid + 37
    assert _grid(t, n, 32) == grid and grid <= 256 and n >= 8 * 64 * grid
    eng = Engine(0, dim)
    try:
        b16 = eng.open_index("rule-b16", dtype="bf16", capacity_rows=n)
        b16.fill_synthetic(n, seed=31)
        f32 = eng.open_index("rule-f32", capacity_rows=n)
        f32.fill_synthetic(n, seed=31)
        eng.synchronize()
        rng = np.random.default_rng(32)
        q = rng.standard_normal((32, dim)).astype(np.float32)
        q[0] = f32.get_row(n - 1)
        q[1] = f32.get_row(70)
        qd = t.from_numpy(q).cuda().contiguous()

        def on_and_off(call):
            with _Floor(None):
                on = call()
            with _Floor("0"):
                off = call()
            assert _same_bits(on, off)
            return on

        s, i = on_and_off(lambda: b16.search(q, 32))
        stored = b16.get_rows(0, n)
        qb = _bf16_round(ops.normalize_rows(qd[:2]).cpu().numpy())
        rs, ri = oracle.search(stored, qb, 32, kind=oracle.KIND_F64)
        _check_against_bf16_oracle(s[:2], i[:2], rs, ri, oracle.scores(stored, qb), "default rule")
        assert i[0, 0] == n - 1 and i[1, 0] == 70
        flat = f32.search(q, 10)
        for mode in ("bf16", "int8"):
            f32.set_prefilter(mode)

            def cand():
                cs, cr = f32.candidates_device(qd)
                return cs.cpu().numpy(), cr.cpu().numpy()
            cs, cr = on_and_off(cand)
            assert cr[0, 0] == n - 1 and cr[1, 0] == 70
            got = on_and_off(lambda: f32.search(q, 10))
            # the flat scan's exact scores for every row both return (recall is test_gpu_prefilter*.py's subject)
            same = got[1] == flat[1]
            assert same[:2, 0].all() and np.array_equal(got[0][same], flat[0][same])
            f32.set_prefilter(False)
    finally:
        eng.close()
