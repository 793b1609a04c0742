"""What tests/test_gpu_ivf_probe.py holds the IVF's probe plan to, built without a GPU: which lists a query probes, the work
list a launch group of 32 queries turns into, the rows its fine scan touches, and the two worlds the tests run in.

The rules (include/rass_engine.h, ``rass_ivf_search``):

  * nprobe <= 32: the first nprobe lists by (coarse score desc, list id asc)                         ``probed_topn``
  * nprobe  > 32: every list whose coarse score is >= the nprobe-th best, ties included             ``probed_threshold``

Coarse scores are fp64 dot products of the fp32 unit centroids and the fp32 unit query; centroids that are bit copies of one
another get the SAME fp64 score (``ranking`` scores each distinct centroid once), so a tie here is a tie in the engine.

``Wide`` (nlist 1 100: 35 coarse tiles, the last of 12 centroids; two lists per plan thread) and ``Limit`` (nlist 32 768, the
most an IVF takes) build the rows, the assignment and the query pool; ``pick`` takes pool queries whose coarse gap at the
nprobe boundary exceeds COARSE_GAP, whose boundary lists hold rows, and whose restricted answer is free of near-ties.
tests/test_ivf_probe_ref_cpu.py asserts, on these inputs alone, that they can tell a wrong probe set from the right one.
"""
import numpy as np

from nonfinite_ref import TOL_F64, no_near_ties

COARSE_GAP = 1e-4          # 100 x the ~1e-6 the engine's coarse scores differ from numpy's (tests/test_gpu_cfg5.py)
BF16_PICK_TOL = 5e-5       # near-tie margin when CHOOSING queries for a bf16 slab: the query's own bf16 rounding depends on
#                            the last bit of its fp32 normalisation, which the GPU and numpy need not share
PLAN_THREADS = 1024
CU_LDS_BYTES = 160 * 1024
DSHIFT, PMASK, DMASK = 24, 0x00FFFFFF, 0x7F000000


# ------------------------------------------------------------------------------------------------ the rules
def normalize(e):
    """fp32 rows / (norm + 1e-9): what the engine does to rows, centroids and queries."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    return (e / (np.linalg.norm(e, axis=1, keepdims=True) + np.float32(1e-9))).astype(np.float32)


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def ranking(cent, qn):
    """(scores f64 [nq, nlist], order int64 [nq, nlist]): the coarse scores and the stable (score desc, list id asc) order.
    Each DISTINCT centroid is scored once, so bit copies tie exactly."""
    cent = np.ascontiguousarray(cent, dtype=np.float32)
    uniq, inv = np.unique(cent, axis=0, return_inverse=True)
    s = (np.asarray(qn, dtype=np.float64) @ uniq.astype(np.float64).T)[:, np.asarray(inv).reshape(-1)]
    return s, np.argsort(-s, axis=1, kind="stable")


def probed_topn(order, nprobe):
    """nprobe <= 32: the first nprobe lists of one query's order (best first)."""
    return np.asarray(order)[:min(int(nprobe), len(order))]


def probed_threshold(scores, order, nprobe):
    """nprobe > 32: every list whose score is >= the nprobe-th best of one query (ascending list ids)."""
    p = min(int(nprobe), len(order))
    return np.flatnonzero(np.asarray(scores) >= scores[order[p - 1]])


def probed(scores, order, nprobe):
    """The lists one query probes, by the rule its (capped) nprobe selects."""
    p = min(int(nprobe), len(order))
    return probed_topn(order, p) if p <= 32 else probed_threshold(scores, order, p)


def work_list(lists_per_query, list_tile0, list_len, tile_rows):
    """(items, scanned) of one launch group: ``lists_per_query`` holds the probed lists of its <= 32 queries (-1 = none).
    items = [(tile, rows, mask)]: lists ascending, a list's tiles ascending from list_tile0[l], ``rows`` valid rows in the
    tile, bit q of ``mask`` set where query q probes the list (an empty probed list gives no item); scanned = the summed
    lengths of the probed lists."""
    assert len(lists_per_query) <= 32 and tile_rows in (32, 64)
    mask = {}
    for q, ls in enumerate(lists_per_query):
        for l in np.asarray(ls).reshape(-1):
            if 0 <= int(l) < len(list_len):
                mask[int(l)] = mask.get(int(l), 0) | (1 << q)
    items, scanned = [], 0
    for l in sorted(mask):
        n = int(list_len[l])
        scanned += n
        for t in range(-(-n // tile_rows)):
            items.append((int(list_tile0[l]) + t, min(tile_rows, n - tile_rows * t), mask[l]))
    return items, scanned


def batch_coarse_lists(nlist, nprobe):
    """Coarse workgroups per launch group of the batched probe (``wpg``): each leaves a top-nprobe list per query."""
    return max(1, min(8, -(-nlist // 32), 256 // min(nprobe, nlist)))


def plan_lds_bytes(nlist, n_clists, nprobe):
    """Dynamic LDS of the plan kernels: [nlist] masks + [1 024] scan scratch, and for the batched plan (n_clists > 0) the
    scores and ids of 32 queries' n_clists * nprobe candidates.  n_clists = 0: the plain plan."""
    return (nlist + PLAN_THREADS + 2 * 32 * n_clists * nprobe) * 4


def batched_plan_fits(nlist, nprobe):
    p = min(nprobe, nlist)
    return p <= 32 and plan_lds_bytes(nlist, batch_coarse_lists(nlist, p), p) <= CU_LDS_BYTES


# ------------------------------------------------------------------------------------------------ the worlds
def plain_filter(j):
    """The exact-tag filter of query position j: every third query unfiltered."""
    return (None if j % 3 == 0 else int((j % 6) | ((j % 2 + 1) << DSHIFT)), None)


def masked_filter(j):
    """The masked filter of query position j: the low field or the high field of the tag."""
    return (int(j % 6), PMASK) if j % 2 else (int((j % 4 // 2 + 1) << DSHIFT), DMASK)


class ProbeWorld:
    """Rows, caller's assignment, tags, tombstones and a query pool over given centroids; the reference answers."""

    def _finish(self, rng, cent, lens, pre_dead_lists, post_dead_lists, delta, tight_lists, q_raw):
        """``lens``: rows per list in the slab.  Source rows are shuffled; ``pre_dead_lists`` name the lists of rows that are
        tombstoned before the build (they never enter the slab), ``post_dead_lists`` lists of which one row each is deleted
        after it (it keeps its slot); rows of ``tight_lists`` lie close to their centroid."""
        self.cent = cent
        self.nlist, self.dim = cent.shape
        nlist, dim = cent.shape
        self.slab_len = np.asarray(lens, dtype=np.int64)
        labels = np.concatenate([np.repeat(np.arange(nlist), lens), np.asarray(pre_dead_lists, dtype=np.int64)])
        dead = np.concatenate([np.zeros(int(np.sum(lens)), dtype=bool), np.ones(len(pre_dead_lists), dtype=bool)])
        self.covered, self.delta = len(labels), int(delta)
        assert delta == 0 or self.covered % 32 == 0
        perm = rng.permutation(self.covered)
        self.assign = labels[perm].astype(np.int32)
        self.pre_dead = np.flatnonzero(dead[perm])
        self.n = self.covered + self.delta
        home = np.concatenate([self.assign, rng.integers(0, nlist, size=self.delta)])
        sigma = np.where(np.isin(home, list(tight_lists)), 0.2, 1.0).astype(np.float32)[:, None]
        x = cent[home] + sigma * rng.standard_normal((self.n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
        self.xn = normalize(x)
        self.tags_raw = (rng.integers(0, 6, size=self.n) | (rng.integers(1, 3, size=self.n) << DSHIFT)).astype(np.int32)
        live = ~dead[perm]
        assert np.array_equal(np.bincount(self.assign[live], minlength=nlist), self.slab_len)
        self.post_dead = np.array([np.flatnonzero((self.assign == l) & live)[j] for j, l in enumerate(post_dead_lists)],
                                  dtype=np.int64)
        assert len(set(self.post_dead.tolist())) == len(post_dead_lists)
        self.tags = self.tags_raw.copy()
        self.tags[self.pre_dead] = -1
        self.tags[self.post_dead] = -1
        self.q_raw = np.ascontiguousarray(q_raw, dtype=np.float32)
        self.qn = normalize(self.q_raw)
        self.qn_bf16 = self.qn                        # a GPU test puts the GPU's own normalisation here (use_gpu_queries)
        self.scores, self.order = ranking(normalize(cent), self.qn)
        ranked = np.take_along_axis(self.scores, self.order, axis=1)
        self.gap = ranked[:, :-1] - ranked[:, 1:]     # [q, j]: between ranks j and j + 1 (0-based)
        self._x64 = self.xn.astype(np.float64)
        self._xb64 = bf16_round(self.xn[:self.covered]).astype(np.float64)
        self._rows, self._tops = {}, {}

    def use_gpu_queries(self, qn_gpu):
        self.qn_bf16 = np.ascontiguousarray(qn_gpu, dtype=np.float32)
        self._rows = {key: v for key, v in self._rows.items() if key[0] != "bf16"}
        self._tops = {key: v for key, v in self._tops.items() if key[0] != "bf16"}

    # ---- the reference
    def row_scores(self, kind, q):
        """fp64 scores [n] of pool query q: "f32" over the fp32 operands; "bf16" the covered rows over the bf16-rounded
        operands (the delta is an fp32 scan); "bf16pick" the same from numpy's normalisation of the query, whatever
        ``use_gpu_queries`` installed, so that the CHOICE of queries is the same with and without a GPU.  Computed for
        blocks of 64 pool queries at a time."""
        b0 = int(q) // 64 * 64
        key = (kind, b0)
        if key not in self._rows:
            s = self.qn[b0:b0 + 64].astype(np.float64) @ self._x64.T
            if kind != "f32":
                qb = bf16_round((self.qn if kind == "bf16pick" else self.qn_bf16)[b0:b0 + 64]).astype(np.float64)
                s[:, :self.covered] = qb @ self._xb64.T
            self._rows[key] = s
        return self._rows[key][int(q) - b0]

    def lists(self, q, nprobe):
        return probed(self.scores[q], self.order[q], nprobe)

    def member(self, lists, qfilter=None, qmask=None, delta=False, allow=None):
        """The live rows of ``lists`` (+ the delta) that pass the filter and the allow bits."""
        lut = np.zeros(self.nlist, dtype=bool)
        lut[np.asarray(lists, dtype=np.int64)] = True
        ok = self.tags != -1
        ok[:self.covered] &= lut[self.assign]
        if not delta:
            ok[self.covered:] = False
        if qfilter is not None and qfilter >= 0:
            ok &= ((self.tags & qmask) if qmask is not None else self.tags) == qfilter
        if allow is not None:
            ok &= allow
        return np.flatnonzero(ok)

    def top_of(self, kind, q, k, lists, qfilter=None, qmask=None, delta=False, allow=None):
        """(scores f64 [k], ids [k]) best first, (score desc, id asc), padded with (-inf, -1): the brute force of query q over
        the rows of ``lists``."""
        rows = self.member(lists, qfilter, qmask, delta, allow)
        s = self.row_scores(kind, q)[rows]
        o = np.lexsort((rows, -s))[:k]
        rs, ri = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
        rs[:len(o)], ri[:len(o)] = s[o], rows[o]
        return rs, ri

    def top(self, slab, q, k, nprobe, qfilter=None, qmask=None, delta=False):
        kind = slab if slab in ("bf16", "bf16pick") else "f32"          # an int8 slab returns the fp32 IVF's answer
        key = (kind, int(q), k, min(nprobe, self.nlist), qfilter, qmask, delta)
        if key not in self._tops:
            self._tops[key] = self.top_of(kind, q, k, self.lists(q, nprobe), qfilter, qmask, delta)
        return self._tops[key]

    def scanned_of(self, lists_per_query, delta=False):
        """Rows the fine scan of ONE launch group touches: the slab length of the union of its queries' lists (+ the delta)."""
        union = np.unique(np.concatenate([np.asarray(l, dtype=np.int64) for l in lists_per_query]))
        return int(self.slab_len[union].sum()) + (self.delta if delta else 0)

    def scanned_groups(self, qs, nprobe, delta=False):
        return [self.scanned_of([self.lists(q, nprobe) for q in qs[g0:g0 + 32]], delta) for g0 in range(0, len(qs), 32)]

    def scanned(self, qs, nprobe, delta=False):
        return sum(self.scanned_groups(qs, nprobe, delta))

    # ---- the choice of queries
    def qualifies(self, nprobe, boundary_rows=True):
        """bool [pool]: the coarse gap at the nprobe boundary exceeds COARSE_GAP and (``boundary_rows``) the lists at ranks
        nprobe and nprobe + 1 hold rows, so that dropping the one or adding the other changes the rows scanned."""
        p = min(int(nprobe), self.nlist)
        ok = np.ones(len(self.q_raw), dtype=bool)
        if p < self.nlist:
            ok &= self.gap[:, p - 1] > COARSE_GAP
            if boundary_rows:
                ok &= (self.slab_len[self.order[:, p - 1]] > 0) & (self.slab_len[self.order[:, p]] > 0)
        elif boundary_rows:
            ok &= self.slab_len[self.order[:, p - 1]] > 0
        return ok

    def clear(self, q, j, k, nprobe, variants):
        """No near-ties among the k + 1 best of query q at position j under every (slab kind, filter function, delta[,
        allow function]) of ``variants``."""
        for kind, flt, delta, *rest in variants:
            f, m = (None, None) if flt is None else flt(j)
            tol = BF16_PICK_TOL if kind == "bf16pick" else TOL_F64
            if rest and rest[0] is not None:
                rs = self.top_of(kind, q, k + 1, self.lists(q, nprobe), f, m, delta, rest[0](j))[0]
            else:
                rs = self.top(kind, q, k + 1, nprobe, f, m, delta)[0]
            if not no_near_ties(rs[None], tol):
                return False
        return True

    def pick(self, nprobe, count, k, variants, skip=(), boundary_rows=True):
        """The first ``count`` pool queries that qualify at ``nprobe`` and are ``clear`` at the position they take."""
        out = []
        for q in np.flatnonzero(self.qualifies(nprobe, boundary_rows)):
            if int(q) not in skip and self.clear(int(q), len(out), k, nprobe, variants):
                out.append(int(q))
                if len(out) == count:
                    return np.array(out)
        raise AssertionError(f"{len(out)} of {count} queries in the pool (dim {self.dim}, nprobe {nprobe}, k {k})")


def variants_for(slabs, flts=(None,), delta=False):
    """The (slab kind, filter, delta) combinations a set of queries must be clear under."""
    kinds = ["f32"] + (["bf16pick"] if "bf16" in slabs else [])
    return [(kind, flt, delta) for kind in kinds for flt in flts]


# ---- the wide world
WIDE_NLIST = 1100
WIDE_DIMS = (100, 700, 1024)
WIDE_BF16_DIMS = (700, 1024)
WIDE_DELTA = 45
WIDE_POOL = 4096
TIE_PAIRS = ((5, 6), (70, 101), (130, 1090))        # one coarse tile; adjacent tiles; the copy in the ragged last tile
TIE_DIM = 100
TIE_AIMED = 48                                       # pool queries aimed at each pair
# the lists whose lengths are chosen: coarse-tile seams (31 | 32, 1087 | 1088), both lists of plan thread 100 (200, 201), a
# plan-thread chunk whose first list is empty (300, 301), the last list, and the tie pairs (17 and 33 rows each)
WIDE_FIXED = {31: 31, 32: 33, 1087: 64, 1088: 63, 200: 200, 201: 65, 300: 0, 301: 32, 1099: 33,
              5: 17, 6: 33, 70: 17, 101: 33, 130: 33, 1090: 17}
WIDE_PRE_DEAD = (0, 31, 32, 200, 201, 301, 1088, 1099)
WIDE_POST_DEAD = (32, 200, 201, 1087, 6)
DEEP_NPROBES = (33, 64, 100, 500, 1099, 1100, 100000)
DEEP_NQS = (1, 17, 32, 33, 70)
BATCH_NPROBES = (1, 8, 17, 32)
BATCH_NQS = (1, 32, 33, 70, 200)
LISTS_NPROBES = (1, 8, 32)
DELTA_NPROBE = 40
K = 10


def wide_slabs(dim):
    return ("f32", "int8") + (("bf16",) if dim in WIDE_BF16_DIMS else ())


class Wide(ProbeWorld):
    def __init__(self, dim):
        rng = np.random.default_rng(43000 + dim)
        nlist = WIDE_NLIST
        cent = normalize(rng.standard_normal((nlist, dim)))
        self.ties = dim == TIE_DIM
        if self.ties:
            for lo, hi in TIE_PAIRS:
                cent[hi] = cent[lo]
        lens = rng.integers(0, 7, size=nlist)
        for l, n in WIDE_FIXED.items():
            lens[l] = n
        free = [l for l in range(nlist) if l not in WIDE_FIXED and lens[l] < 6]
        short = -(int(lens.sum()) + len(WIDE_PRE_DEAD)) % 32           # the covered rows end on a tile: there is a delta
        lens[free[:short]] += 1
        # the pool: c_a + 0.6 c_b + 0.3 c_c + noise; the first queries have a tie pair's lower list as a, b or c in turn
        a, b, c = (rng.integers(0, nlist, size=WIDE_POOL) for _ in range(3))
        b = np.where(b == a, (a + 1) % nlist, b)
        c = np.where((c == a) | (c == b), (np.maximum(a, b) + 1) % nlist, c)
        c = np.where((c == a) | (c == b), (c + 1) % nlist, c)
        for t, (lo, _hi) in enumerate(TIE_PAIRS):
            j = np.arange(t * TIE_AIMED, (t + 1) * TIE_AIMED)
            a[j[0::3]], b[j[1::3]], c[j[2::3]] = lo, lo, lo
        noise = rng.standard_normal((WIDE_POOL, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
        w_c = np.where(np.arange(WIDE_POOL) < len(TIE_PAIRS) * TIE_AIMED, rng.uniform(0.3, 0.5, size=WIDE_POOL), 0.3)
        q_raw = 2.5 * (cent[a] + 0.6 * cent[b] + w_c[:, None].astype(np.float32) * cent[c] + 0.05 * noise)
        tight = [l for pair in TIE_PAIRS for l in pair]
        self._finish(rng, cent, lens, WIDE_PRE_DEAD, WIDE_POST_DEAD, WIDE_DELTA, tight, q_raw)

    def tie_queries(self, slabs, k=K):
        """[(pair, q, r)]: pool queries whose ranking has the pair at the 1-based ranks r, r + 1 with the gap rule holding
        on both sides of it and a clear restricted answer at nprobe = r; per pair the two lowest and the highest r with
        r + 1 <= 32 (the lower list alone is probed) and the lowest r >= 33 and the lowest r >= 300 (both are)."""
        assert self.ties
        out = []
        rank = np.argsort(self.order, axis=1)                          # rank[q, l]: 0-based rank of list l
        for lo, hi in TIE_PAIRS:
            pos = rank[:, lo]
            assert np.array_equal(rank[:, hi], pos + 1)
            q_all = np.arange(len(pos))
            before = np.where(pos > 0, self.gap[q_all, np.maximum(pos - 1, 0)], np.inf)
            after = np.where(pos + 2 < self.nlist, self.gap[q_all, np.minimum(pos + 1, self.nlist - 2)], np.inf)
            ok = (before > COARSE_GAP) & (after > COARSE_GAP)
            found = {}
            for q in np.flatnonzero(ok):
                r = int(pos[q]) + 1
                if (r + 1 <= 32 or r >= 33) and r not in found and self.clear(int(q), 0, k, r, variants_for(slabs)):
                    found[r] = int(q)
            shallow = sorted(r for r in found if r + 1 <= 32)
            deep = sorted(r for r in found if r >= 33)
            want = shallow[:2] + shallow[-1:] + deep[:1] + [r for r in deep if r >= 300][:1]
            out += [((lo, hi), found[r], r) for r in sorted(set(want))]
        return out


# ---- the limit world
LIMIT_NLIST = 32768
LIMIT_DIM = 100
LIMIT_NEAR = 96
LIMIT_NEAR_FIXED = (0, 31, 32, 1023, 1024, 16383, 16384, 32736, 32767)
LIMIT_FAR_WITH_ROWS = (1, 1025, 20000, 32735, 32766)
LIMIT_POOL = 256
LIMIT_NPROBES = (1, 32, 40)
LIMIT_BATCH_NPROBES = (1, 32)
LIMIT_BATCH_NQ = 70


class Limit(ProbeWorld):
    """96 near centroids 0.7 u + r, every other centroid -0.7 u + r (u a shared unit direction, r random of norm ~0.71);
    a query is a mixture of near centroids, so it scores every near list above every far one."""

    def __init__(self):
        rng = np.random.default_rng(44000)
        nlist, dim = LIMIT_NLIST, LIMIT_DIM
        u = normalize(rng.standard_normal((1, dim)))[0]
        others = np.setdiff1d(np.arange(nlist), LIMIT_NEAR_FIXED + LIMIT_FAR_WITH_ROWS)
        self.near = np.sort(np.concatenate([np.array(LIMIT_NEAR_FIXED),
                                            rng.choice(others, size=LIMIT_NEAR - len(LIMIT_NEAR_FIXED), replace=False)]))
        is_near = np.zeros(nlist, dtype=bool)
        is_near[self.near] = True
        r = normalize(rng.standard_normal((nlist, dim)))
        cent = normalize(np.where(is_near[:, None], 0.7, -0.7).astype(np.float32) * u[None, :] + np.float32(0.714) * r)
        lens = np.zeros(nlist, dtype=np.int64)
        lens[self.near] = rng.integers(1, 61, size=LIMIT_NEAR)
        lens[self.near[:7]] = (31, 32, 33, 63, 64, 65, 200)
        lens[list(LIMIT_FAR_WITH_ROWS)] = 20
        a, b, c = (self.near[rng.integers(0, LIMIT_NEAR, size=LIMIT_POOL)] for _ in range(3))
        noise = rng.standard_normal((LIMIT_POOL, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
        q_raw = 2.5 * (cent[a] + 0.6 * cent[b] + 0.3 * cent[c] + 0.05 * noise)
        self.is_near = is_near
        self._finish(rng, cent, lens, (), (self.near[0], self.near[40]), 0, (), q_raw)


# ------------------------------------------------------------------------------------------------ the query sets
def allow_bits(w, j):
    """bool [n]: the rows the bitmap of query position j allows (half of the live ones, seeded; what a bit on a tombstone does
    is tests/test_gpu_ivf_allow.py's)."""
    return (np.random.default_rng(45000 + 131 * w.dim + j).random(w.n) < 0.5) & (w.tags != -1)


def wide_plan(w):
    """The query sets of the wide world's cases, chosen once: the GPU tests run exactly the queries the CPU test vetted."""
    slabs = wide_slabs(w.dim)
    both = variants_for(slabs, (None, plain_filter))
    plan = {"deep": {p: w.pick(p, max(DEEP_NQS), K, both) for p in DEEP_NPROBES},
            "batch": {p: w.pick(p, max(BATCH_NQS), K, both) for p in BATCH_NPROBES},
            "delta": w.pick(DELTA_NPROBE, 33, K, variants_for(slabs, (masked_filter,), delta=True)),
            "allow": w.pick(DELTA_NPROBE, 33, K, [("f32", None, True, lambda j: allow_bits(w, j))]),
            "ties": [], "tie_groups": {}}
    if w.ties:
        plan["ties"] = w.tie_queries(slabs)
        for _pair, q, r in plan["ties"]:
            fill = w.pick(r, 31, K, variants_for(slabs), skip={q})
            plan["tie_groups"][(q, r)] = np.concatenate([fill[:5], [q], fill[5:]])      # the tie query at position 5
    return plan


def limit_plan(w):
    plain = variants_for(("f32",))
    return {"probe": {p: w.pick(p, LIMIT_BATCH_NQ, K, plain) for p in LIMIT_NPROBES},
            "full": w.pick(LIMIT_NLIST, 33, K, plain, boundary_rows=False)}


def perturbed(w, q, nprobe):
    """{name: lists}: the probe sets of two wrong engines for query q — one that drops the list at rank nprobe, one that
    adds the list at rank nprobe + 1 (where there is one).  (The third, a tie resolved the other way, is built where the
    tie queries are checked.)"""
    p = min(int(nprobe), w.nlist)
    right = w.lists(q, nprobe)
    out = {"drop": np.setdiff1d(right, [w.order[q, p - 1]])}
    if p < w.nlist:
        out["add"] = np.union1d(right, [w.order[q, p]])
    return out


def tells_apart(w, slab_kind, q, k, right, wrong, qfilter=None, qmask=None):
    """A search of query q ALONE over ``wrong`` differs from one over ``right`` in the rows scanned or in the top-k ids."""
    if w.scanned_of([wrong]) != w.scanned_of([right]):
        return True
    return not np.array_equal(w.top_of(slab_kind, q, k, wrong, qfilter, qmask)[1], w.top_of(slab_kind, q, k, right, qfilter, qmask)[1])


def allowed_scanned(w, qs, nprobe, bits):
    """Rows ``search_allowed_delta`` scans for the queries ``qs`` under the per-query bitmaps ``bits`` [len(qs), n] (no bit on
    a tombstone): per launch group, the rows of every 32-row slab tile of a probed list in which a query that probes the list
    has an allowed row (a list's rows lie in the slab in source order), plus the rows of every 32-row delta tile in which a
    query of the group has one."""
    live = np.ones(w.covered, dtype=bool)
    live[w.pre_dead] = False
    total = 0
    for g0 in range(0, len(qs), 32):
        probing = {}
        for j, q in enumerate(qs[g0:g0 + 32]):
            for l in w.lists(q, nprobe):
                probing.setdefault(int(l), []).append(g0 + j)
        for l, js in probing.items():
            rows = np.flatnonzero((w.assign == l) & live)
            for t0 in range(0, len(rows), 32):
                tile = rows[t0:t0 + 32]
                total += len(tile) if bits[js][:, tile].any() else 0
        for t0 in range(w.covered, w.n, 32):
            t1 = min(t0 + 32, w.n)
            total += t1 - t0 if bits[g0:g0 + 32, t0:t1].any() else 0
    return total
