"""The oracle and the inputs of the attention tests (tests/test_gpu_attention*.py, tests/test_attention_ref_cpu.py).  Plain
Python: numpy builds the inputs (seeded, the same on every machine), torch computes the fp64 reference on whatever device
the input lies on.  Nothing here needs a GPU.

Layout everywhere: ``qkv`` bf16 ``[tokens][3 * heads * 64]`` (q | k | v per token, each ``[heads][64]``), sequences packed back
to back, ``lens`` their lengths (0 allowed: an empty sequence owns no rows).

The builders make inputs whose answer is KNOWN, or whose scores sit where the kernels' control flow branches:

* ``uniform``    every probability is exactly 1 / S and V is one-hot: the output counts every key exactly once;
* ``needle``     every query has ONE key 36 nats above all others and V holds small non-zero integers: the output row is a V row,
                 bit for bit, and which V row says which key the kernel read;
* ``staircase``  the tile maximum climbs (or falls) by the same amount from one 32-key tile to the next for EVERY query, just
                 below or just above the 2^8 by which the persistent kernel lets a score exceed its reference maximum;
* ``shifted``    all scores share a large negative offset;
* ``poisoned``   neighbouring sequences hold keys that would take the whole softmax of a clean query if a row leaked.

``handoff_plan`` / ``walk`` lay sequences out so that the persistent kernel's workgroups meet every (chunks of this item,
chunks of the next item) pair, on any CU count, and say which workgroup walks which items."""
import numpy as np
import torch

HEAD = 64
CHUNK = 128                        # rows of the persistent kernel's K / V image replaced per boundary
LOG2E = 1.4426950408889634
NEEDLE_MAX_DOT = 32                # largest dot product of two different codebook rows (of 64 for a row with itself)


# ---------------------------------------------------------------------------------------------------------------------
# oracle

def reference(qkv, lens, heads):
    """fp64 softmax(q k^T / 8) v per sequence and head on the bf16 inputs widened to fp64, with torch on qkv's device.
    Returns (out, mag), both fp64 [tokens][heads * 64]; mag = p @ |v|, what the kernels' rounding of p is relative to."""
    hidden = qkv.shape[1] // 3
    assert hidden == heads * HEAD and int(sum(lens)) == qkv.shape[0]
    out = torch.zeros((qkv.shape[0], hidden), dtype=torch.float64, device=qkv.device)
    mag = torch.zeros_like(out)
    t = 0
    for n in lens:
        if n == 0:
            continue
        blk = qkv[t:t + n].double().view(n, 3, heads, HEAD)
        q, k, v = blk[:, 0].transpose(0, 1), blk[:, 1].transpose(0, 1), blk[:, 2].transpose(0, 1)   # [heads][n][64]
        p = torch.softmax(q @ k.transpose(1, 2) / 8.0, dim=-1)
        out[t:t + n] = (p @ v).transpose(0, 1).reshape(n, hidden)
        mag[t:t + n] = (p @ v.abs()).transpose(0, 1).reshape(n, hidden)
        t += n
    return out, mag


def bound(out, mag, slack=1.0):
    """The kernels round the exponentiated scores to bf16 before the second product (relative 2^-9 per term, so the bound
    follows sum_j p_j |v_j|, not the possibly cancelled result) and the output to bf16:
    |err| <= 2^-8 mag + 2^-8 |out| + 2e-3 per element.  Derived from those two rounding points, not measured."""
    return slack * (2.0 ** -8 * mag + 2.0 ** -8 * out.abs() + 2e-3)


# ---------------------------------------------------------------------------------------------------------------------
# builders

def _pack(parts, heads):
    """parts: per sequence (q, k, v), each float32 [n][heads][64]  ->  bf16 [tokens][3 * heads * 64] (round to nearest even)."""
    rows = [np.concatenate([a.reshape(a.shape[0], heads * HEAD) for a in qkv], axis=1) for qkv in parts]
    flat = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3 * heads * HEAD), np.float32)
    return torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32)).to(torch.bfloat16)


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7fffffff for k in key])


def _randn(rng, n, heads, scale):
    return (rng.standard_normal((n, heads, HEAD)) * scale).astype(np.float32)


def random_qkv(lens, heads, scale=1.0, seed=0):
    parts = []
    for si, n in enumerate(lens):
        rng = _rng(101, seed, si)
        parts.append((_randn(rng, n, heads, scale), _randn(rng, n, heads, scale), _randn(rng, n, heads, scale)))
    return _pack(parts, heads)


def uniform(lens, heads, seed=0):
    """Q = 0, K random, V[j][d] = 1 if j % 64 == d else 0: every score is 0, every probability exactly 1 / S, and
    out[i][d] = #{j < S : j % 64 == d} / S — each key counted once, whatever K holds."""
    parts = []
    for si, n in enumerate(lens):
        rng = _rng(102, seed, si)
        v = np.zeros((n, heads, HEAD), np.float32)
        j = np.arange(n)
        v[j, :, j % HEAD] = 1.0
        parts.append((np.zeros((n, heads, HEAD), np.float32), _randn(rng, n, heads, 1.0), v))
    return _pack(parts, heads)


_CODEBOOK = None


def codebook():
    """512 rows of +-1 [64], seeded, drawn one by one and kept only if their dot product with every row kept so far is
    <= NEEDLE_MAX_DOT (a plain draw of 512 rows peaks at 32-36; the hand-off case uses several hundred codebooks, so the
    bound is built in and not left to the seed).  Every (sequence, head) uses rows of THIS matrix in its own order with its own
    column signs: the cross dots are those of the base, the bits are not."""
    global _CODEBOOK
    if _CODEBOOK is None:
        rng = _rng(103)
        kept = np.zeros((512, HEAD), np.float32)
        n = 0
        while n < 512:
            c = rng.integers(0, 2, size=HEAD).astype(np.float32) * 2.0 - 1.0
            if n == 0 or float((kept[:n] @ c).max()) <= NEEDLE_MAX_DOT:
                kept[n] = c
                n += 1
        _CODEBOOK = kept
    return _CODEBOOK


def reversal(i, n):
    return n - 1 - i


def rotation(i, n):
    return (i + 33) % n


def needle(lens, heads, perm, seed=0):
    """K = 3 C, Q[i] = 3 C[perm(i)], C the (sequence, head)'s +-1 codebook: query i's score on key perm(i) is 72 nats, on any
    other key at most 36.  V holds seeded integers of magnitude 1 .. 32 (exact in bf16; never 0, so that the stray 2^-52 of
    the other keys is absorbed by fp32 rounding and not left standing where V is 0).  Returns (qkv, want) with
    want[i] = V[perm(i)], float32 [tokens][heads * 64]: what every output row must be."""
    base = codebook()
    parts, want = [], []
    for si, n in enumerate(lens):
        assert n <= 512
        q = np.zeros((n, heads, HEAD), np.float32)
        k = np.zeros_like(q)
        v = np.zeros_like(q)
        p = perm(np.arange(n), n) if n else np.zeros((0,), np.int64)
        for h in range(heads):
            rng = _rng(104, seed, si, h)
            c = base[rng.permutation(512)[:n]] * (rng.integers(0, 2, size=HEAD).astype(np.float32) * 2.0 - 1.0)
            k[:, h] = 3.0 * c
            q[:, h] = 3.0 * c[p]
            v[:, h] = rng.integers(1, 33, size=(n, HEAD)) * (rng.integers(0, 2, size=(n, HEAD)) * 2 - 1)
        parts.append((q, k, v))
        want.append(v[p].reshape(n, heads * HEAD))
    want = np.concatenate(want, axis=0) if want else np.zeros((0, heads * HEAD), np.float32)
    return _pack(parts, heads), torch.from_numpy(np.ascontiguousarray(want))


def staircase(lens, heads, step, seed=0):
    """q, k, v random at scale 0.5 / 0.5 / 1, then two columns carry a staircase: Q[:, 0] = Q[:, 1] = 8,
    K[j, 0] = (j // 32) * 5.5 sign(step), K[j, 1] = (j // 32) * (|step| - 5.5) sign(step), so key j's score gains
    (j // 32) * step nats.  step is +-5.5 or +-5.625 nats = 7.93 / 8.12 in the exp2 domain, one on each side of the
    persistent kernel's 2^8 rule.

    Two things make the rise of the tile maximum from one FULL 32-key tile to the next exactly `step` for every query, not
    just on average: (i) the staircase is split over two columns because (j // 32) * 5.625 is no bf16 number from j // 32 = 7
    on (315 / 8 needs 9 bits; rounded, the rise alternates between 5.5 and 5.75 nats) while multiples of 5.5 and of 0.125 up
    to 15 are exact; (ii) the random part of K repeats every 32 keys (K[j, 2:] = K[j % 32, 2:]), so every full tile holds
    the same random scores — drawn per key, their tile maxima would differ by ~0.25 exp2 units, four times the 0.07 between
    7.93 and 8.  V is drawn per key."""
    assert abs(step) in (5.5, 5.625)
    sign = 1.0 if step > 0 else -1.0
    parts = []
    for si, n in enumerate(lens):
        rng = _rng(105, seed, si)
        q, k, v = _randn(rng, n, heads, 0.5), _randn(rng, min(n, 32), heads, 0.5), _randn(rng, n, heads, 1.0)
        j = np.arange(n)
        k = k[j % 32] if n else np.zeros((0, heads, HEAD), np.float32)
        q[:, :, 0:2] = 8.0
        k[:, :, 0] = ((j // 32) * 5.5 * sign).astype(np.float32)[:, None]
        k[:, :, 1] = ((j // 32) * (abs(step) - 5.5) * sign).astype(np.float32)[:, None]
        parts.append((q, k, v))
    return _pack(parts, heads)


def shifted(lens, heads, offset=-60.0, seed=0):
    """Random inputs (scale 1) with Q[:, 1] = 8 and K[:, 1] = offset: every score is shifted by `offset` nats.  At -60 the
    scores stand at -87 in the exp2 domain; at -120 they stand at -173, where exp2 against a maximum of 0 (instead of the
    scores' own) underflows fp32 and the row sum is 0."""
    parts = []
    for si, n in enumerate(lens):
        rng = _rng(106, seed, si)
        q, k, v = _randn(rng, n, heads, 1.0), _randn(rng, n, heads, 1.0), _randn(rng, n, heads, 1.0)
        q[:, :, 1] = 8.0
        k[:, :, 1] = offset
        parts.append((q, k, v))
    return _pack(parts, heads)


def poisoned(lens, heads, seed=0):
    """Sequences alternate clean (even index) and poison (odd).  Clean: Q[:, 0] = 4, K[:, 0] = 0, the rest random.  Poison:
    random Q, K[:, 0] = 100 and V = 100 everywhere.  One poison key row read by a clean query scores 50 nats above the clean
    keys and turns the whole output row into 100; the poison sequences' own rows are exactly 100."""
    parts = []
    for si, n in enumerate(lens):
        rng = _rng(107, seed, si)
        q, k, v = _randn(rng, n, heads, 1.0), _randn(rng, n, heads, 1.0), _randn(rng, n, heads, 1.0)
        if si % 2 == 0:
            q[:, :, 0] = 4.0
            k[:, :, 0] = 0.0
        else:
            k[:, :, 0] = 100.0
            v[:] = 100.0
        parts.append((q, k, v))
    return _pack(parts, heads)


# ---------------------------------------------------------------------------------------------------------------------
# the persistent kernel's walk

def chunks(n):
    return (n + CHUNK - 1) // CHUNK


def handoff_plan(n_cus):
    """(heads, lens): 3 * (n_cus / heads) sequences in three rounds A, B, C; with more items than CUs the grid is n_cus and
    workgroup b walks item b of each round in order (sequence b // heads of the round).  The first 16 sequences of the
    rounds have the chunk counts A_i = i // 4 + 1, B_i = i % 4 + 1, C_i = (i // 4 + i % 4) % 4 + 1: (A, B) and (B, C) both
    run through all 16 pairs.  Lengths sit on chunk edges, differently per round: A = 128 c (full chunks), B = 128 (c - 1) + 1
    (one row in the last chunk: waves without queries, a single key tile at c = 1), C = 128 c - 37 (ragged).  Sequences
    beyond the 16 triples are 200 tokens long."""
    heads = next(h for h in (16, 8, 4, 2, 1) if n_cus % h == 0 and n_cus // h >= 16)
    per_round = n_cus // heads
    a, b, c = [], [], []
    for i in range(per_round):
        if i < 16:
            a.append(CHUNK * (i // 4 + 1))
            b.append(CHUNK * (i % 4) + 1)
            c.append(CHUNK * ((i // 4 + i % 4) % 4 + 1) - 37)
        else:
            a.append(200), b.append(200), c.append(200)
    return heads, a + b + c


def walk(n_cus, heads, lens):
    """Per workgroup of the persistent kernel (grid = min(items, n_cus); workgroup b takes items b, b + grid, ...; item =
    sequence * heads + head): (items, chunk counts of those items)."""
    n_items = len(lens) * heads
    grid = min(n_items, n_cus)
    out = []
    for b in range(grid):
        items = list(range(b, n_items, grid))
        out.append((items, [chunks(lens[it // heads]) for it in items]))
    return out


def transitions(walks, k):
    """The set of (chunks of item k, chunks of item k + 1) over all workgroups' walks."""
    return {(c[k], c[k + 1]) for _, c in walks if len(c) > k + 1}


ALL_PAIRS = {(a, b) for a in range(1, 5) for b in range(1, 5)}


# ---------------------------------------------------------------------------------------------------------------------
# a numpy model of the kernels' rounding points (what `bound` is derived from), for the CPU checks of the inputs

def round_bf16(x):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def rounding_model(qkv, lens, heads, lazy):
    """The kernels' arithmetic with their two bf16 rounding points and nothing else of them: scores in the exp2 domain, a
    reference maximum per query that is exact per 64 keys (lazy = False, the 16x16 kernel) or moves per 32 keys only when
    some query of a 32-query tile exceeds it by more than 8 (lazy = True, the persistent kernel), p rounded to bf16 before
    the second product, the row sum over the UNROUNDED p, the output rounded to bf16.  Returns float32 [tokens][hidden]."""
    x = qkv.float().numpy().astype(np.float64)
    hidden = heads * HEAD
    out = np.zeros((x.shape[0], hidden), np.float32)
    kb = 32 if lazy else 64
    t = 0
    for n in lens:
        blk = x[t:t + n].reshape(n, 3, heads, HEAD)
        for h in range(heads):
            q, k, v = blk[:, 0, h], blk[:, 1, h], blk[:, 2, h]
            s = (q @ k.T) * (LOG2E / 8.0)
            for q0 in range(0, n, 32):
                sq = s[q0:q0 + 32]
                m = np.full(sq.shape[0], -np.inf)
                l = np.zeros(sq.shape[0])
                o = np.zeros((sq.shape[0], HEAD))
                for k0 in range(0, n, kb):
                    mx = sq[:, k0:k0 + kb].max(axis=1)
                    if not lazy or bool((mx > m + 8.0).any()):
                        m_new = np.maximum(m, mx)
                        alpha = np.exp2(m - m_new)
                        l, o, m = l * alpha, o * alpha[:, None], m_new
                    p = np.exp2(sq[:, k0:k0 + kb] - m[:, None]).astype(np.float32)
                    l = l + p.astype(np.float64).sum(axis=1)
                    o = o + round_bf16(p).astype(np.float64) @ v[k0:k0 + kb]
                out[t + q0:t + q0 + sq.shape[0], h * HEAD:(h + 1) * HEAD] = round_bf16((o / l[:, None]).astype(np.float32))
        t += n
    return out
