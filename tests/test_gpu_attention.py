"""K6 on its own (rass_attention_bf16): the encoder's varlen self-attention against a plain PyTorch fp64 reference of the
same op (softmax(q k^T / 8) v per sequence and head, fp64 throughout, on the same bf16 inputs: tests/attention_ref.py).

Tolerance: the kernel rounds the exponentiated scores to bf16 before the second product (relative 2^-9 per term, so
the bound follows sum_j p_j |v_j|, not the possibly cancelled result) and the output to bf16:
|err| <= 2^-8 (sum_j p_j |v_j|) + 2^-8 |ref| + 2e-3 per element.  Both kernels are held to it on every case: the
32x32-tile persistent kernel (RASS_ATTN_VARIANT=w8; the default for batches of mostly-long sequences) and the 16x16-tile
kernel (w16; the default otherwise); the variable is read per launch.

(Round 3's w8f experiment — scale and reference maximum folded into the QK^T MFMA chain: no faster, 3x the error on peaked
scores — is no longer instantiated in the product library: `make EXTRA=-DRASS_ATTN_EXPERIMENTS` builds it,
scripts/probe_attention_accuracy.py measures it.)"""
import ctypes
import os

import numpy as np
import pytest

import attention_ref as A

pytestmark = pytest.mark.gpu

LENS_EDGE = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 320, 448, 511, 512]


def _reference(torch, qkv, lens, heads):
    """fp64 on the device (tests/attention_ref.py): (out, mag = p @ |v|)."""
    return A.reference(qkv, lens, heads)


def _run(torch, qkv, lens, heads, max_seqlen=None):
    from rassengine_amd import _native as N_
    cu = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    d_cu = torch.from_numpy(cu).cuda()
    hidden = qkv.shape[1] // 3
    ctx = torch.full((qkv.shape[0] + 3, hidden), 777.0, dtype=torch.bfloat16, device="cuda")
    N_.check("rass_attention_bf16", N_.lib().rass_attention_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(d_cu.data_ptr()), len(lens), int(cu[-1]),
        int(max_seqlen or max(lens)), hidden, heads, ctypes.c_void_p(ctx.data_ptr()), ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    assert bool((ctx[qkv.shape[0]:] == 777.0).all())          # nothing written past the last token
    return ctx[:qkv.shape[0]].float()


def _check(torch, lens, heads, scale, seed, max_seqlen=None, slack=1.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    total = int(sum(lens))
    qkv = (torch.randn((total, 3 * heads * 64), generator=g, device="cuda") * scale).bfloat16()
    ref, mag = _reference(torch, qkv, lens, heads)
    got = _run(torch, qkv, lens, heads, max_seqlen)
    err = (got - ref).abs()
    tol = slack * (2.0 ** -8 * mag + 2.0 ** -8 * ref.abs() + 2e-3)
    assert bool(torch.isfinite(got).all())
    assert bool((err <= tol).all()), (float((err - tol).max()), int((err > tol).sum()), float((err / tol).max()))


@pytest.fixture(params=["w8", "w16", ""])
def variant(request):
    old = os.environ.get("RASS_ATTN_VARIANT")
    if request.param:
        os.environ["RASS_ATTN_VARIANT"] = request.param
    else:
        os.environ.pop("RASS_ATTN_VARIANT", None)
    yield request.param
    if old is None:
        os.environ.pop("RASS_ATTN_VARIANT", None)
    else:
        os.environ["RASS_ATTN_VARIANT"] = old


def test_attention_every_length_class(gpu, variant):
    """1 .. 512 tokens: below / at / above every 32- and 64-key boundary, sequences packed back to back."""
    _check(gpu, LENS_EDGE, heads=3, scale=1.0, seed=1)


def test_attention_peaked_scores_and_moving_maximum(gpu, variant):
    """|q.k| / 8 up to ~40: the running maximum moves in most key blocks (the rescale path), probabilities span
    2^-100 .. 1."""
    _check(gpu, [512, 77, 300, 64], heads=2, scale=2.5, seed=2)


def test_attention_large_shape_and_padded_launch(gpu, variant):
    """BERT-large heads (16 x 64) and max_seqlen above the longest sequence (the launch pads K / V to it)."""
    _check(gpu, [512, 512, 1, 130, 512], heads=16, scale=1.0, seed=3)
    _check(gpu, [40, 9, 64], heads=16, scale=1.0, seed=4, max_seqlen=512)


def test_attention_more_items_than_workgroups(gpu, variant):
    """40 sequences x 16 heads = 640 (sequence, head) items: the persistent kernel's workgroups (one per CU) walk 2-3
    items each, of different lengths, with the next item's K / V prefetched under the current one."""
    rng = np.random.default_rng(11)
    lens = [512, 1, 257, 300] + [int(x) for x in rng.integers(1, 513, size=36)]
    _check(gpu, lens, heads=16, scale=1.0, seed=6)


def test_attention_variants_agree_closely(gpu):
    """The two kernels implement one algorithm (same bf16 rounding points): outputs within one bf16 ulp of each other
    almost everywhere."""
    torch = gpu
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    lens = [512, 333, 64, 17]
    qkv = torch.randn((sum(lens), 3 * 4 * 64), generator=g, device="cuda").bfloat16()
    old = os.environ.pop("RASS_ATTN_VARIANT", None)
    try:
        os.environ["RASS_ATTN_VARIANT"] = "w8"
        a = _run(torch, qkv, lens, 4)
        os.environ["RASS_ATTN_VARIANT"] = "w16"
        b = _run(torch, qkv, lens, 4)
    finally:
        os.environ.pop("RASS_ATTN_VARIANT", None)
        if old is not None:
            os.environ["RASS_ATTN_VARIANT"] = old
    assert float((a - b).abs().max()) <= 2.0 ** -7 * float(a.abs().max())
    assert float(((a - b).abs() > 2.0 ** -8 * a.abs() + 1e-3).float().mean()) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# Query time: the attention recomputed inside the attention-output projection (rass_attention_out_bf16, one launch)

def _fused_case(torch, lens, seed, scale=1.0):
    from rassengine_amd import _native as N_
    heads, hidden, n = 16, 1024, 1024
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    total = int(sum(lens))
    pad = 128
    qkv = torch.zeros((pad, 3 * hidden), dtype=torch.bfloat16, device="cuda")
    qkv[:total] = (torch.randn((total, 3 * hidden), generator=g, device="cuda") * scale).bfloat16()
    w = (torch.randn((n, hidden), generator=g, device="cuda") * 0.03).bfloat16()
    bias = torch.randn((n,), generator=g, device="cuda") * 0.1
    res = torch.zeros((pad, n), dtype=torch.bfloat16, device="cuda")
    res[:total] = torch.randn((total, n), generator=g, device="cuda").bfloat16()
    cu = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    d_cu = torch.from_numpy(cu).cuda()
    st = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    L = N_.lib()
    # the pair: attention launch + the few-rows GEMM (bias + residual); the scratch selects the query-time GEMM path
    ctx = torch.zeros((pad, hidden), dtype=torch.bfloat16, device="cuda")
    N_.check("rass_attention_bf16", L.rass_attention_bf16(ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(d_cu.data_ptr()),
                                                          len(lens), total, max(lens), hidden, heads,
                                                          ctypes.c_void_p(ctx.data_ptr()), st))
    ws = torch.empty((2 * 256 * n,), dtype=torch.float32, device="cuda")
    y_pair = torch.full((pad, n), 555.0, dtype=torch.bfloat16, device="cuda")
    N_.check("rass_gemm_bf16_ws", L.rass_gemm_bf16_ws(ctypes.c_void_p(ctx.data_ptr()), ctypes.c_void_p(w.data_ptr()),
                                                      ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(res.data_ptr()),
                                                      ctypes.c_void_p(y_pair.data_ptr()), total, pad, n, hidden, 1,
                                                      ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, st))
    y = torch.full((pad, n), 555.0, dtype=torch.bfloat16, device="cuda")
    N_.check("rass_attention_out_bf16", L.rass_attention_out_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(d_cu.data_ptr()), len(lens), total, hidden, heads,
        ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(res.data_ptr()),
        ctypes.c_void_p(y.data_ptr()), n, st))
    torch.cuda.synchronize()
    assert bool((y[total:] == 555.0).all()) and bool((y_pair[total:] == 555.0).all())      # rows past the batch untouched
    # reference of the whole op on the same bf16 inputs (the context in fp64, the projection in fp32)
    ref_ctx, _ = _reference(torch, qkv[:total], lens, heads)
    ref = ref_ctx.bfloat16().float() @ w.float().t() + bias + res[:total].float()
    return y[:total].float(), y_pair[:total].float(), ref


@pytest.mark.parametrize("lens", [[1], [11], [16], [17], [23], [32], [9, 7], [12, 15, 5], [1, 1, 1, 1], [16, 16], [3, 13, 2, 14],
                                  [1] * 32, [5, 0, 7], [0, 16]])
def test_fused_attention_output_projection_equals_the_pair(gpu, lens):
    """One launch == attention + few-rows GEMM: the context rows carry attention_kernel's bits, the projection sums its 16
    head slices in another order than the 4-wave GEMM, so the outputs agree to the last bf16 bit almost everywhere and
    within one ulp elsewhere; both sit within the bf16 bound of the fp32 reference."""
    torch = gpu
    y, y_pair, ref = _fused_case(torch, lens, seed=100 + sum(lens))
    assert bool(torch.isfinite(y).all())
    # one bf16 ulp of the output, or — where bias + residual cancel the product — the fp32 rounding of O(1) partial sums
    ulp = 2.0 ** -7 * torch.maximum(y.abs(), y_pair.abs()) + 4e-6
    assert bool(((y - y_pair).abs() <= ulp).all()), float(((y - y_pair).abs() / ulp).max())
    assert float((y == y_pair).float().mean()) >= 0.97
    tol = 2.0 ** -7 * ref.abs() + 0.03
    assert bool(((y - ref).abs() <= tol).all()), float(((y - ref).abs() - tol).max())


def test_fused_attention_output_projection_peaked_scores(gpu):
    """|q.k| / 8 up to ~40 (probabilities 2^-100 .. 1), ragged sequences."""
    torch = gpu
    y, y_pair, ref = _fused_case(torch, [13, 19], seed=7, scale=2.5)
    ulp = 2.0 ** -7 * torch.maximum(y.abs(), y_pair.abs()) + 4e-6
    assert bool(((y - y_pair).abs() <= ulp).all())


def test_fused_attention_output_projection_as_torch_op(gpu):
    """torch.ops.rass.attention_out_bf16 == the C-ABI call (same launch), and it refuses what the library refuses."""
    torch = gpu
    import rassengine_amd.ops  # noqa: F401  (registers torch.ops.rass.*)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    qkv = torch.randn((13, 3072), generator=g, device="cuda").bfloat16()
    w = (torch.randn((1024, 1024), generator=g, device="cuda") * 0.03).bfloat16()
    bias = torch.randn((1024,), generator=g, device="cuda")
    res = torch.randn((13, 1024), generator=g, device="cuda").bfloat16()
    cu = torch.tensor([0, 13], dtype=torch.int32, device="cuda")
    y = torch.ops.rass.attention_out_bf16(qkv, cu, 16, w, bias, res)
    ctx = torch.ops.rass.attention_bf16(qkv, cu, 13, 16)
    ref = ctx.float() @ w.float().t() + bias + res.float()
    assert y.shape == (13, 1024) and y.dtype == torch.bfloat16
    assert bool(((y.float() - ref).abs() <= 2.0 ** -7 * ref.abs() + 0.03).all())
    with pytest.raises(Exception):
        torch.ops.rass.attention_out_bf16(torch.zeros((40, 3072), dtype=torch.bfloat16, device="cuda"),
                                          torch.tensor([0, 40], dtype=torch.int32, device="cuda"), 16, w, bias,
                                          torch.zeros((40, 1024), dtype=torch.bfloat16, device="cuda"))


def test_fused_attention_output_projection_refuses_outside_its_range(gpu, monkeypatch):
    torch = gpu
    from rassengine_amd import _native as N_
    L = N_.lib()
    z = torch.zeros((64, 3072), dtype=torch.bfloat16, device="cuda")
    cu = torch.tensor([0, 33], dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(z.data_ptr())
    args = lambda total, hidden, heads, n: (p, ctypes.c_void_p(cu.data_ptr()), 1, total, hidden, heads, p, p, p, p, n, None)
    assert L.rass_attention_out_bf16(*args(33, 1024, 16, 1024)) == -5
    assert L.rass_attention_out_bf16(*args(16, 768, 12, 768)) == -5
    assert L.rass_attention_out_bf16(*args(16, 1024, 16, 1000)) == -5
    monkeypatch.setenv("RASS_ATTN_FUSE", "0")
    assert L.rass_attention_out_bf16(*args(16, 1024, 16, 1024)) == -5
