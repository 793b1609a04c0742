"""What tests/test_gpu_kmeans_matrix.py holds the k-means kernels (csrc/kmeans.hip) to, built without a GPU.

The world of one dim.  ``n = (2 * CUs + 37) * 32 - 27`` rows (17 541 on 256 CUs: 548 full 32-row blocks and one of 5, so that
with a grid of ``CUs`` workgroups some walk two row blocks and some three) against a pool of 200 centroids, of which a case
uses the first ``nlist``:

  * centroids 20, 35 and 70 are copies of centroid 3, and 66 of 40.  Within the 32-centroid tiles the kernel ranks, 3 and 20
    share a tile in different lanes, 3 and 35 a lane in different tiles, 3 and 70 neither; 40 sits in an earlier tile and a
    higher lane than 66.  A row that one of them wins ties EXACTLY with its copies, and the lowest list must take it;
  * centroid 5 is all zero (what ``ivf._finite_rows`` can hand the kernel): it scores +0.0 against every row and wins the
    rows whose every other score is negative, which at nlist 7 are about one in 64 of the iid rows.  Behind 199 other
    centroids it wins nothing: the one row it ties for, the all-zero row, goes to list 0;
  * every pool centroid has 30 rows ``c + 0.3 noise`` (cosine 0.96 to c, below 0.6 to any other centroid at the narrowest
    dim), five centroids also an exact copy among the rows, ``-c[0]`` gives nlist 1 a negative best score, one row is all
    zero (every score +0.0: list 0), the rest are iid.  The rows are shuffled, so every kind lands in every part of the slab.

The reference of a case is the oracle's emulation of the scan's summation order (``KIND_F32_MFMA``: 8 slices of 16 * CH
columns, an fmaf chain inside a slice, the slices' partials added in order; symmetric in its operands), computed once per dim
for the whole pool and cut to ``nlist`` columns: ``best`` is its row maximum as fp32 bits, ``assign`` the first column that
attains it.
"""
import numpy as np

DIMS = (101, 200, 384, 498, 640, 703, 896, 1024)          # one per stride class 128 .. 1024; 101, 498, 703: dim % 4 = 1, 2, 3
POOL = 200
NLISTS = (1, 7, 17, 32, 33, 49, 65, 96, 97, 200)          # 1, 1, 1, 1, 2, 2, 3, 3, 4, 7 centroid tiles of 32
RANGE_NLISTS = (33, 97)
DUP_GROUPS = ((3, 20, 35, 70), (40, 66))
ZERO_CENTROID = 5
PER_CENTROID = 30
COPIED = (0, 3, 40, 97, 199)                              # centroids that are also rows: cosine 1
NOISE = 0.3
MIN_TIE_ROWS = 50
SPLIT = 7001                                              # the two add() calls meet inside a 16-row block
N_DEAD = 40


def n_rows(cus):
    return (2 * cus + 37) * 32 - 27


def n_centroid_tiles(nlist):
    return -(-nlist // 32)


def make_world(dim, cus):
    """(raw rows [n, dim] f32, raw centroid pool [200, dim] f32, owner [n]: the pool centroid a row was planted at, -1 for the
    others, special: name -> row) of one dim.  Nothing is normalised here: the index and the centroid packing do that."""
    n = n_rows(cus)
    rng = np.random.default_rng(41000 + dim)
    cent = rng.standard_normal((POOL, dim), dtype=np.float32)
    for grp in DUP_GROUPS:
        for j in grp[1:]:
            cent[j] = cent[grp[0]]
    cent[ZERO_CENTROID] = 0.0
    parts, owner = [], []
    for j in range(POOL):
        parts.append(cent[j] + NOISE * rng.standard_normal((PER_CENTROID, dim), dtype=np.float32))
        owner += [j] * PER_CENTROID
    parts.append(cent[list(COPIED)])
    owner += list(COPIED)
    parts.append(-cent[0:1])
    parts.append(np.zeros((1, dim), dtype=np.float32))
    owner += [-1, -1]
    planted = sum(len(p) for p in parts)
    parts.append(rng.standard_normal((n - planted, dim), dtype=np.float32))
    owner += [-1] * (n - planted)
    x = np.concatenate(parts).astype(np.float32)
    owner = np.array(owner, dtype=np.int64)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    first_copy = POOL * PER_CENTROID
    special = {"copies": inv[first_copy:first_copy + len(COPIED)], "neg0": int(inv[first_copy + len(COPIED)]),
               "zero": int(inv[first_copy + len(COPIED) + 1])}
    assert x.shape == (n, dim) and n % 32 == 5
    return np.ascontiguousarray(x[perm]), cent, owner[perm], special


def dead_rows(cus):
    """40 rows to delete: row 0, the last row of a full block, rows inside the ragged last block, 35 others."""
    n = n_rows(cus)
    rng = np.random.default_rng(42000 + cus)
    fixed = [0, 100 * 32 + 31, n - 5, n - 3, n - 1]
    others = rng.choice(np.setdiff1d(np.arange(n), fixed), size=N_DEAD - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, others])).astype(np.int64)


def emulated(oracle, cent_bits, row_bits):
    """[n, POOL] fp32: the oracle's emulation of the kernel's order for every (row, pool centroid)."""
    s = oracle.scores(cent_bits, row_bits, kind=oracle.KIND_F32_MFMA)
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s)                  # the emulation's values ARE fp32
    return s32


def expect(s32, nlist):
    """(assign int32 [n], best f32 [n]) of the first nlist pool centroids: the maximum and the LOWEST list that attains it."""
    s = s32[:, :nlist]
    return s.argmax(axis=1).astype(np.int32), s.max(axis=1)


def tie_rows(s32, nlist):
    """The rows whose maximum over the first nlist centroids is attained by two or more of them."""
    s = s32[:, :nlist]
    return np.flatnonzero((s == s.max(axis=1, keepdims=True)).sum(axis=1) >= 2)


def group_of(j):
    for grp in DUP_GROUPS:
        if j in grp:
            return grp
    return (j,)


def check_world(s32, owner, special):
    """The conditions the assertions of the matrix rest on, on the reference alone; returns nlist -> number of tie rows."""
    assert not np.isnan(s32).any()
    ties = {}
    for nlist in NLISTS:
        a, best = expect(s32, nlist)
        t = tie_rows(s32, nlist)
        ties[nlist] = len(t)
        if nlist >= 21:
            assert len(t) >= MIN_TIE_ROWS, (nlist, len(t))
        # every duplicate group of which two members are in play wins rows, all of them for its lowest list
        for grp in DUP_GROUPS:
            inside = [j for j in grp if j < nlist]
            if len(inside) >= 2:
                won = np.flatnonzero(np.isin(a, inside))
                assert len(won) >= PER_CENTROID and np.all(a[won] == grp[0]), (nlist, grp, len(won))
                assert np.all(np.isin(won, t))
        # a planted row goes to its own centroid (the lowest of its copies) as soon as that one is in play
        for j in range(nlist):
            if j != ZERO_CENTROID:
                mine = np.flatnonzero(owner == j)
                lowest = group_of(j)[0]
                assert np.all(a[mine] == lowest), (nlist, j)
        assert a[special["zero"]] == 0 and best[special["zero"]].view(np.uint32) == 0        # +0.0, list 0
    a, best = expect(s32, 1)
    assert best[special["neg0"]] < -0.999 and np.all(a == 0)
    a, best = expect(s32, 7)
    zero_wins = np.flatnonzero(a == ZERO_CENTROID)
    assert len(zero_wins) >= 20 and np.all(best[zero_wins].view(np.uint32) == 0), len(zero_wins)
    a, best = expect(s32, POOL)
    copies_of = [j for grp in DUP_GROUPS for j in grp[1:]]
    for j in range(POOL):
        if j == ZERO_CENTROID or j in copies_of:
            assert not np.any(a == j), j                  # a copy never wins: the lower list does; the zero centroid: see above
        else:
            assert np.any(a == j), j
    for r, j in zip(special["copies"], COPIED):
        assert a[r] == group_of(j)[0] and abs(float(best[r]) - 1.0) <= 1e-6
    return ties


def block_ranges(total_blocks):
    """(first_block, block_step, n_blocks) of the four ranges.  n_blocks is the largest the index allows, so the last
    processed block is the last one ``first_block + i * block_step`` reaches: the ragged last block of the index where
    ``(total_blocks - 1 - first_block) % block_step == 0`` (on 256 CUs: 549 blocks, (2, 3) ends on block 548 and (0, 3) on 546)."""
    return [(first, step, (total_blocks - 1 - first) // step + 1) for first, step in ((0, 1), (0, 3), (2, 3), (5, 1))]


def range_rows(first, step, n_blocks):
    """The index row each of the n_blocks * 32 output entries speaks for."""
    e = np.arange(n_blocks * 32, dtype=np.int64)
    return (first + (e // 32) * step) * 32 + e % 32


def caller_assignment(nlist, rows, n, seed):
    """A caller's assignment for the entries ``rows``: random lists, about one entry in eight one of the four values that
    ``rass_kmeans_accumulate`` must skip (-1, nlist, nlist + 5, INT32_MIN); entries of rows past n hold valid lists, which
    must be skipped for their row.  List 1 is left empty (nlist >= 3): whatever a row of list 0 adds behind its last column
    lands there."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nlist, size=len(rows)).astype(np.int32)
    if nlist >= 3:
        a[a == 1] = 0
    bad = np.array([-1, nlist, nlist + 5, np.iinfo(np.int32).min], dtype=np.int64)
    where = np.flatnonzero(rng.random(len(rows)) < 0.125)
    a[where] = bad[np.arange(len(where)) % 4].astype(np.int32)
    assert all(np.any(a[rows < n] == b) for b in bad.astype(np.int32))
    return a


def accumulate_ref(x64, rows, assign, nlist, n):
    """(counts f64 [nlist], sums f64 [nlist, dim], bound f64 [nlist, dim]) of ``rass_kmeans_accumulate`` over the entries
    ``rows`` with the lists ``assign``: entries of rows at or past n and lists outside [0, nlist) are skipped.  The bound
    is the worst case of a list's m fp32 adds in ANY order, m * 2^-24 * sum |x| per column ((m - 1) roundings of relative
    size 2^-24 each on partial sums no larger than sum |x|, second-order terms inside the spare m-th), plus 1e-30."""
    a = assign.astype(np.int64)
    ok = (rows < n) & (a >= 0) & (a < nlist)
    onehot = np.zeros((nlist, int(ok.sum())))
    onehot[a[ok], np.arange(int(ok.sum()))] = 1.0
    xs = x64[rows[ok]]
    counts = onehot.sum(axis=1)
    sums = onehot @ xs
    bound = counts[:, None] * 2.0 ** -24 * (onehot @ np.abs(xs)) + 1e-30
    return counts, sums, bound
