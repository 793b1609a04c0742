"""The conditions tests/test_gpu_attention_exact.py rests on, checked on tests/attention_ref.py alone (no GPU): the oracle
equals a naive loop; the needle really is a needle and its V rows can be told apart; the staircase really straddles the
persistent kernel's 2^8 rule; the hand-off plan really reaches every (chunks of this item, chunks of the next item) pair as
first and as second transition on every CU count; and a model of the kernels' two bf16 rounding points stays inside the
bound on every builder — so a GPU failure on these inputs is the kernel's, not the inputs'."""
import numpy as np
import pytest
import torch

import attention_ref as A

# every length the GPU file uses for the needle: the single-launch lengths, the padded launch, the fused kernel, the plan
L_SINGLE = [1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 384, 385, 511, 512]
L_PLAN = sorted({n for cus in (256, 304, 64, 32) for n in A.handoff_plan(cus)[1]})
L_NEEDLE = sorted(set(L_SINGLE + [40, 9, 64, 1] + [32, 16, 7, 18, 31, 5] + L_PLAN))
PERMS = [A.reversal, A.rotation]


def _split(qkv, n0, n, heads, h):
    blk = qkv[n0:n0 + n].float().numpy().astype(np.float64).reshape(n, 3, heads, A.HEAD)
    return blk[:, 0, h], blk[:, 1, h], blk[:, 2, h]


def test_reference_equals_a_naive_loop():
    lens, heads = [5, 1, 17], 2
    qkv = A.random_qkv(lens, heads, scale=1.0, seed=3)
    out, mag = A.reference(qkv, lens, heads)
    assert out.dtype == torch.float64 and mag.dtype == torch.float64
    t = 0
    for n in lens:
        for h in range(heads):
            q, k, v = _split(qkv, t, n, heads, h)
            for i in range(n):
                w = np.array([np.exp(sum(q[i, d] * k[j, d] for d in range(64)) / 8.0) for j in range(n)])
                w /= w.sum()
                for d in range(64):
                    o = sum(w[j] * v[j, d] for j in range(n))
                    a = sum(w[j] * abs(v[j, d]) for j in range(n))
                    assert abs(float(out[t + i, 64 * h + d]) - o) <= 1e-12
                    assert abs(float(mag[t + i, 64 * h + d]) - a) <= 1e-12
        t += n


def test_reference_skips_empty_sequences():
    lens, heads = [0, 4, 0, 3], 1
    qkv = A.random_qkv(lens, heads, seed=4)
    out, _ = A.reference(qkv, lens, heads)
    out2, _ = A.reference(qkv, [4, 3], heads)
    assert qkv.shape[0] == 7 and torch.equal(out, out2)


def test_codebook_cross_dots():
    c = A.codebook()
    g = c @ c.T
    assert c.shape == (512, 64) and set(np.unique(c)) == {-1.0, 1.0}
    assert np.all(np.diag(g) == 64) and float((g - 64 * np.eye(512)).max()) <= A.NEEDLE_MAX_DOT


@pytest.mark.parametrize("perm", PERMS, ids=["reversal", "rotation"])
def test_needle_is_a_needle_and_its_value_rows_differ(perm):
    heads = 2
    qkv, want = A.needle(L_NEEDLE, heads, perm)
    assert torch.equal(qkv.float().bfloat16(), qkv) and float(qkv.float().abs().max()) <= 32
    t = 0
    for n in L_NEEDLE:
        for h in range(heads):
            q, k, v = _split(qkv, t, n, heads, h)
            s = q @ k.T / 8.0
            p = np.exp(s - s.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            idx = perm(np.arange(n), n)
            assert np.all(p[np.arange(n), idx] >= 1.0 - 2.0 ** -30), (n, h)
            assert np.array_equal(want[t:t + n, 64 * h:64 * h + 64].numpy(), v[idx].astype(np.float32))
            assert np.all(v != 0) and np.all(v == np.round(v)) and np.abs(v).max() <= 32
            # any two V rows differ by at least 2 in at least 32 components (so none are equal, and one bf16 step — 2^-8
            # relative, at most 1/8 here — cannot turn one into another)
            vi = v.astype(np.int16)
            far = (np.abs(vi[:, None, :] - vi[None, :, :]) >= 2).sum(axis=2) + 64 * np.eye(n, dtype=np.int64)
            assert int(far.min()) >= 32, (n, h, int(far.min()))
        t += n


@pytest.mark.parametrize("step", [5.5, -5.5, 5.625, -5.625])
def test_staircase_straddles_the_2_pow_8_rule(step):
    lens, heads = [512, 385, 129, 64, 33, 1], 2
    qkv = A.staircase(lens, heads, step)
    lo, hi = (7.0, 8.0) if abs(step) == 5.5 else (8.0, 9.0)
    t = 0
    seen = 0
    for n in lens:
        for h in range(heads):
            q, k, _ = _split(qkv, t, n, heads, h)
            s = (q @ k.T) * (A.LOG2E / 8.0)
            full = n // 32
            if full >= 2:
                mx = s[:, :32 * full].reshape(n, full, 32).max(axis=2)        # [query][tile]
                rise = np.diff(mx, axis=1) * np.sign(step)
                assert float(rise.min()) > lo and float(rise.max()) < hi, (n, h, float(rise.min()), float(rise.max()))
                seen += rise.size
        t += n
    assert seen > 0


@pytest.mark.parametrize("n_cus", [256, 304, 64, 32])
def test_handoff_plan_reaches_every_pair_twice(n_cus):
    heads, lens = A.handoff_plan(n_cus)
    assert n_cus % heads == 0 and n_cus // heads >= 16 and len(lens) == 3 * (n_cus // heads)
    walks = A.walk(n_cus, heads, lens)
    assert len(lens) * heads > n_cus and len(walks) == n_cus and all(len(items) == 3 for items, _ in walks)
    assert sorted(it for items, _ in walks for it in items) == list(range(len(lens) * heads))
    assert A.transitions(walks, 0) == A.ALL_PAIRS
    assert A.transitions(walks, 1) == A.ALL_PAIRS
    # rounds A and C swapped: still every pair, and a long item after a short one as the LAST transition
    r = len(lens) // 3
    swapped = lens[2 * r:] + lens[r:2 * r] + lens[:r]
    ws = A.walk(n_cus, heads, swapped)
    assert A.transitions(ws, 0) == A.ALL_PAIRS and A.transitions(ws, 1) == A.ALL_PAIRS
    assert max(lens) <= 512 and min(lens) >= 1 and sum(lens) <= 15000


def test_walk_of_a_small_batch():
    assert A.walk(4, 2, [1, 129, 512]) == [([0, 4], [1, 4]), ([1, 5], [1, 4]), ([2], [2]), ([3], [2])]
    assert A.walk(256, 2, [5, 0]) == [([0], [1]), ([1], [1]), ([2], [0]), ([3], [0])]


def _builders(s):
    three = [s, 64, s]
    yield "uniform", A.uniform([s], 2), [s]
    yield "needle/reversal", A.needle([s], 2, A.reversal)[0], [s]
    yield "needle/rotation", A.needle([s], 2, A.rotation)[0], [s]
    for step in (5.5, -5.5, 5.625, -5.625):
        yield "staircase/%g" % step, A.staircase([s], 2, step), [s]
    yield "shifted/-60", A.shifted([s], 2), [s]
    yield "shifted/-120", A.shifted([s], 2, offset=-120.0), [s]
    yield "poisoned", A.poisoned(three, 2), three
    yield "random", A.random_qkv([s], 2), [s]


@pytest.mark.parametrize("s", [33, 129, 385, 512])
def test_rounding_model_stays_within_the_bound_on_every_builder(s):
    """The bound is derived from the kernels' two bf16 rounding points; a model with exactly those (and either form of the
    reference maximum) must meet it on every input the GPU file uses, or the input, not a kernel, would fail there.  The
    peak ratio is printed: it is a property of the inputs."""
    peak = {}
    for name, qkv, lens in _builders(s):
        ref, mag = A.reference(qkv, lens, 2)
        tol = A.bound(ref, mag).numpy()
        for lazy in (True, False):
            got = A.rounding_model(qkv, lens, 2, lazy)
            assert np.all(np.isfinite(got)), (name, lazy)
            ratio = float((np.abs(got - ref.numpy()) / tol).max())
            peak[name, lazy] = ratio
            assert ratio <= 1.0, (name, lazy, ratio)
    print("S = %d: peak |err| / bound = %.3f (%s)" % (s, max(peak.values()), max(peak, key=peak.get)))


def test_needle_and_uniform_models_meet_their_exact_assertions():
    """What the GPU file asserts on the known-answer inputs holds for the rounding model: needle rows are V rows bit for
    bit, uniform rows are within 2^-8 relative of count / S with no absolute term."""
    lens = [1, 33, 129, 385]
    for perm in PERMS:
        qkv, want = A.needle(lens, 2, perm)
        for lazy in (True, False):
            assert np.array_equal(A.rounding_model(qkv, lens, 2, lazy), want.numpy())
    qkv = A.uniform(lens, 2)
    ref, _ = A.reference(qkv, lens, 2)
    for lazy in (True, False):
        got = A.rounding_model(qkv, lens, 2, lazy)
        assert np.all(np.abs(got - ref.numpy()) <= 2.0 ** -8 * ref.numpy())
