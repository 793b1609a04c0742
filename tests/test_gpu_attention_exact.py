"""The three attention kernels (rass_attention_bf16 as the 32x32-tile persistent kernel `w8`, as the 16x16-tile kernel `w16`
and by its default dispatch; rass_attention_out_bf16, the query-time fusion) on inputs whose answer is KNOWN or whose scores
sit where the control flow branches, against the fp64 oracle of tests/attention_ref.py.  tests/test_attention_ref_cpu.py
proves, without a GPU, that the inputs have the properties relied on here.

* uniform:   every key counted exactly once (relative 2^-8, no absolute term);
* needle:    every output row IS one V row, bit for bit — which one says which key was read;
* staircase: the reference maximum of the persistent kernel moves in every tile / every second tile / never;
* shifted:   all scores far below 0;
* poisoned:  one row leaked across a sequence boundary would take a whole softmax;
* padded launch: the answers do not depend on max_seqlen;
* hand-off:  the persistent kernel's workgroups walk three items each and meet all 16 (chunks of this item, chunks of the
             next) pairs as first and as second transition — asserted from the device's CU count before the launch;
* empty sequences own no rows and disturb nobody (include/rass_engine.h);
* the fused kernel's context rows carry attention_kernel's bits.

Every launch writes into a buffer with three guard rows in front and three behind."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import attention_ref as A

pytestmark = pytest.mark.gpu

L = [1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 384, 385, 511, 512]      # 32 items at 2 heads: one per workgroup
L_POISON = [129, 64, 1, 257, 33, 512, 31, 128]
GUARD = 777.0
PERMS = {"reversal": A.reversal, "rotation": A.rotation}


@contextlib.contextmanager
def _forced(name):
    """RASS_ATTN_VARIANT is read per launch."""
    old = os.environ.get("RASS_ATTN_VARIANT")
    if name:
        os.environ["RASS_ATTN_VARIANT"] = name
    else:
        os.environ.pop("RASS_ATTN_VARIANT", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("RASS_ATTN_VARIANT", None)
        else:
            os.environ["RASS_ATTN_VARIANT"] = old


@pytest.fixture(params=["w8", "w16", ""])
def variant(request):
    with _forced(request.param):
        yield request.param


_CACHE = {}


def _once(key, make):
    """Inputs and references are built once per session and never changed by a test."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _run(torch, qkv, lens, heads, max_seqlen=None):
    """One launch of rass_attention_bf16 -> bf16 [tokens][hidden]; the guard rows around the output must survive."""
    from rassengine_amd import _native as N_
    cu = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    d_cu = torch.from_numpy(cu).cuda()
    hidden = qkv.shape[1] // 3
    total = qkv.shape[0]
    assert total == int(cu[-1])
    buf = torch.full((total + 6, hidden), GUARD, dtype=torch.bfloat16, device="cuda")
    N_.check("rass_attention_bf16", N_.lib().rass_attention_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(d_cu.data_ptr()), len(lens), total,
        int(max_seqlen or max(lens)), hidden, heads, ctypes.c_void_p(buf[3:].data_ptr()),
        ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    assert bool((buf[:3] == GUARD).all()) and bool((buf[total + 3:] == GUARD).all())     # nothing written outside
    return buf[3:total + 3].clone()


def _where(lens, row):
    t = 0
    for si, n in enumerate(lens):
        if row < t + n:
            return "sequence %d (S = %d) query %d" % (si, n, row - t)
        t += n
    return "row %d" % row


def _assert_equal(torch, got, want, lens, what):
    """Bit equality of bf16 rows with known integer values; on a miss, say where and by how much."""
    g = got.float()
    bad = (g != want).any(dim=1)
    if bool(bad.any()):
        rows = torch.nonzero(bad).flatten()
        r = int(rows[0])
        d = (g[r] - want[r]).abs()
        raise AssertionError("%s: %d of %d rows differ; first %s: %d elements, max |diff| %g (want |v| <= 32); rows %s" % (
            what, int(bad.sum()), g.shape[0], _where(lens, r), int((d > 0).sum()), float(d.max()), rows[:8].tolist()))


def _assert_bound(torch, got, ref, mag, lens, what):
    g = got.double()
    assert bool(torch.isfinite(g).all()), what + ": non-finite output"
    err = (g - ref).abs()
    tol = A.bound(ref, mag)
    ratio = float((err / tol).max())
    print("%s: peak |err| / bound = %.3f" % (what, ratio))
    if ratio > 1.0:
        r = int(torch.nonzero((err > tol).any(dim=1)).flatten()[0])
        raise AssertionError("%s: peak |err| / bound = %.3f, %d elements outside; first %s" % (
            what, ratio, int((err > tol).sum()), _where(lens, r)))


def _with_ref(torch, key, make_qkv, lens, heads):
    def make():
        qkv = make_qkv().cuda()
        ref, mag = A.reference(qkv, lens, heads)
        return qkv, ref, mag
    return _once(key, make)


# ---------------------------------------------------------------------------------------------------------------------
# single launches, one item per workgroup

def test_uniform_counts_every_key_once(gpu, variant):
    """Q = 0, V one-hot: out[i][d] = #{j : j % 64 == d} / S.  The count and S are exact in fp32; what remains is the fp32
    rounding of 1 / S and of the product and one bf16 rounding, so the error is relative and there is no absolute term.  A
    lost or doubled key moves an element by at least 1/9 of its value (S = 512: 8 keys per element)."""
    torch = gpu
    qkv, ref, _ = _with_ref(torch, "uniform", lambda: A.uniform(L, 2), L, 2)
    got = _run(torch, qkv, L, 2).double()
    err = (got - ref).abs()
    bad = err > 2.0 ** -8 * ref
    assert not bool(bad.any()), (int(bad.sum()), _where(L, int(torch.nonzero(bad.any(dim=1)).flatten()[0])),
                                 float((err / ref.clamp_min(1e-30)).max()))


@pytest.mark.parametrize("perm", sorted(PERMS))
def test_needle_returns_the_value_row_bit_for_bit(gpu, variant, perm):
    """The needle's probability is exp2(0) = 1, everything else sums to < 2^-38 of it, V is a non-zero integer of magnitude
    <= 32: the output row is V[perm(i)] exactly."""
    torch = gpu
    qkv, want = _once(("needle", perm), lambda: tuple(x.cuda() for x in A.needle(L, 2, PERMS[perm])))
    _assert_equal(torch, _run(torch, qkv, L, 2), want, L, "needle/" + perm)


@pytest.mark.parametrize("step", [5.5, -5.5, 5.625, -5.625])
def test_staircase_around_the_lazy_maximum_threshold(gpu, variant, step):
    """The tile maximum of every query rises (falls) by 7.93 or 8.12 in the exp2 domain per 32-key tile: climbing, the
    persistent kernel's reference maximum moves in every second / in every tile; falling, it stays where tile 0 put it and
    the last tiles' probabilities are 2^-119 and less."""
    torch = gpu
    qkv, ref, mag = _with_ref(torch, ("staircase", step), lambda: A.staircase(L, 2, step), L, 2)
    _assert_bound(torch, _run(torch, qkv, L, 2), ref, mag, L, "staircase/%g" % step)


@pytest.mark.parametrize("offset", [-60.0, -120.0])
def test_scores_with_a_large_common_offset(gpu, variant, offset):
    """Every score shifted by -60 nats (-87 in the exp2 domain) and by -120 (-173).  Against a maximum started at 0 the
    first still fits fp32's exponent range (2^-87 and a relative rounding: the answer would be right); the second underflows
    to a zero row sum.  Both must equal the unshifted softmax."""
    torch = gpu
    qkv, ref, mag = _with_ref(torch, ("shifted", offset), lambda: A.shifted(L, 2, offset), L, 2)
    _assert_bound(torch, _run(torch, qkv, L, 2), ref, mag, L, "shifted/%g" % offset)


def test_poisoned_neighbours(gpu, variant):
    """Clean and poison sequences alternate (3 heads); every output row is checked, the poison sequences' included."""
    torch = gpu
    qkv, ref, mag = _with_ref(torch, "poisoned", lambda: A.poisoned(L_POISON, 3), L_POISON, 3)
    _assert_bound(torch, _run(torch, qkv, L_POISON, 3), ref, mag, L_POISON, "poisoned")


@pytest.mark.parametrize("kind", ["needle", "random"])
def test_answers_do_not_depend_on_max_seqlen(gpu, variant, kind):
    """The launch pads the K / V image to max_seqlen (whole 64-row blocks or 128-row chunks): six classes, bit-identical
    outputs, one of them held to the known answer / the oracle."""
    torch = gpu
    lens, heads = [40, 9, 64, 1], 16
    if kind == "needle":
        qkv, want = _once("padded/needle", lambda: tuple(x.cuda() for x in A.needle(lens, heads, A.reversal, seed=1)))
    else:
        qkv, ref, mag = _with_ref(torch, "padded/random", lambda: A.random_qkv(lens, heads, seed=1), lens, heads)
    outs = [_run(torch, qkv, lens, heads, max_seqlen=m) for m in (64, 65, 128, 129, 300, 512)]
    for m, o in zip((65, 128, 129, 300, 512), outs[1:]):
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), "max_seqlen %d differs from 64 (%s)" % (m, kind)
    if kind == "needle":
        _assert_equal(torch, outs[0], want, lens, "padded/needle")
    else:
        _assert_bound(torch, outs[0], ref, mag, lens, "padded/random")


# ---------------------------------------------------------------------------------------------------------------------
# the persistent kernel's hand-off from item to item

def _plan(torch, order):
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    heads, lens = A.handoff_plan(n_cus)
    if order == "cba":                     # rounds A and C swapped: a long item follows a short one as the LAST transition
        r = len(lens) // 3
        lens = lens[2 * r:] + lens[r:2 * r] + lens[:r]
    return n_cus, heads, lens


def _assert_coverage(n_cus, heads, lens):
    walks = A.walk(n_cus, heads, lens)
    assert len(lens) * heads > n_cus and all(len(items) == 3 for items, _ in walks)
    assert A.transitions(walks, 0) == A.ALL_PAIRS, sorted(A.ALL_PAIRS - A.transitions(walks, 0))
    assert A.transitions(walks, 1) == A.ALL_PAIRS, sorted(A.ALL_PAIRS - A.transitions(walks, 1))


@pytest.mark.parametrize("order", ["abc", "cba"])
def test_handoff_every_chunk_pair_needle(gpu, order):
    """Every workgroup of the persistent kernel walks three items; the 16 x 16 chunk-count pairs all occur as first and as
    second transition.  A chunk of K or V rows that arrives late, is never sent or is sent over rows still in use puts other
    keys or values under some query's needle: the row is then another V row, or none."""
    torch = gpu
    n_cus, heads, lens = _plan(torch, order)
    _assert_coverage(n_cus, heads, lens)
    qkv, want = _once(("handoff/needle", order), lambda: tuple(x.cuda() for x in A.needle(lens, heads, A.reversal, seed=2)))
    with _forced("w8"):                    # the plan's mean length is ~265 tokens: the default dispatch would take w16
        a = _run(torch, qkv, lens, heads)
        b = _run(torch, qkv, lens, heads)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two launches on one input differ"
    _assert_equal(torch, a, want, lens, "hand-off/needle/" + order)


@pytest.mark.parametrize("order", ["abc", "cba"])
def test_handoff_every_chunk_pair_random(gpu, order):
    """The same walk on random data at scale 1 against the oracle, launched twice: the outputs are bit-identical."""
    torch = gpu
    n_cus, heads, lens = _plan(torch, order)
    _assert_coverage(n_cus, heads, lens)

    def make():
        g = torch.Generator(device="cuda")
        g.manual_seed(21 if order == "abc" else 22)
        qkv = torch.randn((sum(lens), 3 * heads * 64), generator=g, device="cuda").bfloat16()
        return (qkv,) + A.reference(qkv, lens, heads)
    qkv, ref, mag = _once(("handoff/random", order), make)
    with _forced("w8"):
        a = _run(torch, qkv, lens, heads)
        b = _run(torch, qkv, lens, heads)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two launches on one input differ"
    _assert_bound(torch, a, ref, mag, lens, "hand-off/random/" + order)


@pytest.mark.parametrize("c", [1, 2])
def test_handoff_all_workgroups_in_step(gpu, c):
    """Every item of a round has the same length (128 c, 128 (c - 1) + 32, 128 c - 37), so all workgroups hand over at the
    same moment and their last chunks (c <= 2: sent only at the end of the item before, the case the kernel's `sync0` state
    stands for) travel together, from memory the launch has not touched: as slow as this arrival gets.  The short middle
    round reads that chunk as early as an item can (at c = 2 key tile 4, all 32 rows of it some query's needle, is fetched
    a step before boundary 1).  A chunk that arrived late would put the item before's rows under those needles.  (What it
    cannot show: on the MI355X the transfer wins that race even without the wait — `sync0 = nc < 2` passes here as it passes
    everywhere else; that wait is justified by the code's ordering, not by a failing output.)"""
    torch = gpu
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    heads, plan = A.handoff_plan(n_cus)
    r = len(plan) // 3
    lens = [128 * c] * r + [128 * (c - 1) + 32] * r + [128 * c - 37] * r
    walks = A.walk(n_cus, heads, lens)
    assert len(walks) == n_cus and all(ch == [c, c, c] for _, ch in walks)
    qkv, want = _once(("handoff/in step", c), lambda: tuple(x.cuda() for x in A.needle(lens, heads, A.reversal, seed=3)))
    torch.empty((1 << 29,), dtype=torch.uint8, device="cuda").zero_()     # 512 MiB: the inputs leave the caches
    with _forced("w8"):
        a = _run(torch, qkv, lens, heads)
    _assert_equal(torch, a, want, lens, "hand-off/in step/%d" % c)


# ---------------------------------------------------------------------------------------------------------------------
# empty sequences: no rows, nobody disturbed

@pytest.mark.parametrize("lens", [[0, 17, 0, 0, 300, 0], [0, 5]], ids=["0-17-0-0-300-0", "0-5"])
def test_empty_sequences_own_no_rows(gpu, variant, lens):
    torch = gpu
    key = tuple(lens)
    qkv, ref, mag = _with_ref(torch, ("empty/random", key), lambda: A.random_qkv(lens, 2, seed=5), lens, 2)
    _assert_bound(torch, _run(torch, qkv, lens, 2), ref, mag, lens, "empty/random")
    nq, want = _once(("empty/needle", key), lambda: tuple(x.cuda() for x in A.needle(lens, 2, A.reversal, seed=5)))
    _assert_equal(torch, _run(torch, nq, lens, 2), want, lens, "empty/needle")


def test_handoff_through_empty_items(gpu):
    """The hand-off plan with every third sequence of round B emptied: a workgroup of the persistent kernel walks
    item -> empty item -> item.  The empty item sends nothing of its own and hands no chunk over; its neighbours' rows are
    what they are without it."""
    torch = gpu
    n_cus, heads, lens = _plan(torch, "abc")
    r = len(lens) // 3
    lens = [0 if (r <= i < 2 * r and (i - r) % 3 == 0) else n for i, n in enumerate(lens)]
    walks = A.walk(n_cus, heads, lens)
    assert {c[1] for _, c in walks} >= {0, 1, 2, 3, 4} and all(len(c) == 3 for _, c in walks)
    assert {(c[0], c[2]) for _, c in walks if c[1] == 0} >= {(1, 1), (1, 4), (4, 4), (4, 3)}    # (before, after) an empty item
    qkv, want = _once("empty/handoff", lambda: tuple(x.cuda() for x in A.needle(lens, heads, A.reversal, seed=6)))
    with _forced("w8"):
        a = _run(torch, qkv, lens, heads)
        b = _run(torch, qkv, lens, heads)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two launches on one input differ"
    _assert_equal(torch, a, want, lens, "hand-off/empty items")


# ---------------------------------------------------------------------------------------------------------------------
# query time: the attention recomputed inside the attention-output projection

def _fused_inputs(kind, lens):
    if kind == "uniform":
        return A.uniform(lens, 16, seed=7), None
    if kind == "needle":
        return A.needle(lens, 16, A.reversal, seed=7)
    return A.poisoned(lens, 16, seed=7), None


@pytest.mark.parametrize("kind", ["uniform", "needle", "poisoned"])
@pytest.mark.parametrize("lens", [[32], [16, 16], [1] * 32, [7, 18, 7], [31, 1], [5, 0, 7]],
                         ids=["32", "16-16", "1x32", "7-18-7", "31-1", "5-0-7"])
def test_fused_context_rows_carry_the_16x16_kernels_bits(gpu, kind, lens):
    """W = the 1024 x 1024 identity, zero bias, zero residual: the projection adds 15 zero partial tiles and two zeros to
    the wave's own context tile, so y IS the context the fused kernel computed — and the header promises that to be
    attention_kernel's, bit for bit.  ctx itself meets the known answer."""
    torch = gpu
    from rassengine_amd import _native as N_
    heads, hidden = 16, 1024
    total = sum(lens)
    qkv, want = _once(("fused", kind, tuple(lens)),
                      lambda: tuple(None if x is None else x.cuda() for x in _fused_inputs(kind, lens)))
    w = _once("fused/identity", lambda: torch.eye(hidden, dtype=torch.bfloat16, device="cuda"))
    bias = torch.zeros((hidden,), dtype=torch.float32, device="cuda")
    res = torch.zeros((total, hidden), dtype=torch.bfloat16, device="cuda")
    with _forced("w16"):
        ctx = _run(torch, qkv, lens, heads)
    cu = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    d_cu = torch.from_numpy(cu).cuda()
    buf = torch.full((total + 6, hidden), GUARD, dtype=torch.bfloat16, device="cuda")
    N_.check("rass_attention_out_bf16", N_.lib().rass_attention_out_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(d_cu.data_ptr()), len(lens), total, hidden, heads,
        ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(res.data_ptr()),
        ctypes.c_void_p(buf[3:].data_ptr()), hidden, ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    assert bool((buf[:3] == GUARD).all()) and bool((buf[total + 3:] == GUARD).all())
    y = buf[3:total + 3]
    # values, not bit patterns: the projection's "+ 0" turns a -0 of the context into +0
    diff = (y.float() != ctx.float())
    assert not bool(diff.any()), (int(diff.sum()), _where(lens, int(torch.nonzero(diff.any(dim=1)).flatten()[0])),
                                  float((y.float() - ctx.float()).abs().max()))
    if kind == "needle":
        _assert_equal(torch, ctx, want, lens, "fused/needle")
    else:
        ref, mag = A.reference(qkv, lens, heads)
        if kind == "uniform":
            assert bool(((ctx.double() - ref).abs() <= 2.0 ** -8 * ref).all())
        else:
            _assert_bound(torch, ctx, ref, mag, lens, "fused/poisoned")
