"""The encoder's LayerNorm, embedding and pooling kernels op by op (the C ABI's stand-alone launchers) against fp64
references computed from the same bf16 inputs the kernels read.

Rows.  Besides iid N(0, 1) rows every LayerNorm-bearing case carries the families where LayerNorm arithmetic goes wrong:
a common offset of 8 sigma and of 32 sigma, one outlier column at 100 sigma (BERT's "massive activation"), and rows that
are constant in bf16; gamma is log-uniform in [0.01, 5] with a random sign and beta ~ N(0, 1) in every case.

Tolerances (u = 2^-24, the fp32 unit roundoff; bf16 rounding is relative 2^-8 at most).
* LayerNorm, rounded once to bf16 (embedding + LN, layernorm_kernel, the few-rows query GEMM's x_out):
  fp32 statistics: the mean is a sum of <= 32 values per lane and 6 butterfly steps (<= 38 u relative to the sum of
  |x|), the variance likewise, rsqrt / divide / + eps a few u more, and (x - mean) * rstd * gamma + beta 4 u: the fp32
  value is within 64 u (|gamma| rstd mean|x| + |gamma x^| + |beta|) of the fp64 one, and the bf16 rounding adds
  2^-8 |value|.  Held to  2^-8 (|gamma x^| + |beta|) + 2^-17 (|gamma| rstd mean|x| + |gamma x^| + |beta|) + 1e-6,
  not to 2^-8 |ref| (gamma x^ + beta may cancel).  The 2^-17 term is what fp32 statistics cost at a large offset
  (|mean| / sigma = 32: 2^-12 |gamma|); rows constant in bf16 have an exact fp32 mean (bf16 values, <= 2 048 of them:
  every partial sum is exact), x^ = 0 and must come back as bf16(beta).  The embedding's sum of three bf16 rows in fp32
  adds 2 u of their magnitudes per element (in the same bracket).
* Residual + LayerNorm: the kernels round y = GEMM + bias + residual to bf16 before normalising; the reference rounds
  the fp64 y at the same point and normalises that.  Where the fp32 and fp64 y may round to different neighbours (y64
  within the fp32 GEMM error (K + 3) u (sum |x w| + |b| + |res|) of a rounding midpoint) the bound adds
  |gamma| rstd ulp(y) for that element and |gamma| rstd (1 + |x^_i|) sum_j ulp_j (1 + |x^_j|) / n for the row's others
  (its effect on the statistics).  The GEMM output y itself (where a branch writes it) keeps the GEMM tests' bound
  1.5 2^-8 |ref| + 2e-3.
* The few-rows GEMM with the LayerNorm inside: y = epi(bf16(LN(yin)) W^T + b) against the fp64 epi(LN(yin) W^T + b):
  the GEMM bound plus the LayerNorm bound propagated through W (tol_LN @ |W|^T, times 1.13 = max GELU' for epilogue 2).
* LN fold (encoder_gemm.hip, LnFold).  fold_gamma: W' = bf16(W gamma) bit for bit; colsum and bias' are fp32 sums of
  K / 64 terms per lane and 6 butterfly steps: (K / 64 + 8) u of the sum of magnitudes.  EPI 3: the raw r against fp64
  X W^T + b + LN_prev(res) with LN_prev from the same fp32 (mean, rstd): the GEMM bound + 2^-20 (|gamma| |res| rstd +
  |beta|) for the fp32 rebuild; its per-chunk (sum r, sum r^2) against fp64 sums of the stored bf16 r within 2^-17 of
  the sums of |r| and r^2 (depth <= 16 adds).  ln_stats_finalize: the mean within 2^-16 mean|r| and rstd within 2^-11
  relative of the fp64 statistics of the stored r — the one-pass variance q / n - mean^2 loses log2(mean^2 / var) bits,
  2^-11 holds up to |mean| / sigma = 32.  EPI 4 / 5: against fp64 x^ W'^T + (b + beta W^T) with x^ from fp64
  statistics of the stored r (W' is pinned bit for bit above): the GEMM bound, + K u rstd (|r| @ |W'|^T) for the fp32
  accumulation over the raw (offset) rows, + the statistics' error (2^-11 |x^| @ |W'|^T + rstd 2^-16 mean|r| |colsum|)
  when (mean, rstd) come from the kernels.  Rows that are constant, or offset beyond 32 sigma, are outside the fold's
  contract (the one-pass variance cancels) and are not tested here; the unfused kernels serve them.
* Pooling: the mean is a sequential fp32 sum: (n + 2) u mean|x|; normalised: + 64 u |ref| and the mean's error relative
  to the norm.

Every case also checks that nothing is written past the last row (sentinel fill).  Large cases reference a subset of the
rows (every 7th and the last 64)."""
import ctypes

import numpy as np
import pytest

from tests.helpers import _residual_branch, _splitk_slices  # noqa: F401  (the routing mirror)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-12
SENT = 777.0
HIDDENS = [128, 384, 768, 1000, 1024, 1536, 2048]


# ---------------------------------------------------------------------------------------------------------- plumbing
def _lib():
    from rassengine_amd import _native as N_
    return N_


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st(torch):
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _call(name, *args):
    N_ = _lib()
    N_.check(name, getattr(N_.lib(), name)(*args))


def _gen(torch, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _ref_rows(m):
    """every 7th row and the last 64 (all rows of small cases)"""
    if m <= 512:
        return np.arange(m)
    return np.unique(np.concatenate([np.arange(0, m, 7), np.arange(max(0, m - 64), m)]))


def _gamma_beta(torch, g, n):
    u = torch.rand((n,), generator=g, device="cuda", dtype=torch.float32)
    sign = torch.where(torch.rand((n,), generator=g, device="cuda") < 0.2, -1.0, 1.0)
    gamma = (0.01 * 500.0 ** u * sign).float()
    beta = torch.randn((n,), generator=g, device="cuda")
    return gamma, beta


def _family_rows(torch, g, m, n, families=5, const=None):
    """fp32 [m][n]: row i is of family i % families — 0 iid, 1 offset 8, 2 offset 32, 3 outlier column at 100,
    4 constant (`const` [m] values; default +-4 / +-8)"""
    x = torch.randn((m, n), generator=g, device="cuda")
    fam = torch.arange(m, device="cuda") % families
    x[fam == 1] += 8.0
    x[fam == 2] += 32.0
    x[fam == 3, (n // 3 + 5) % n] = 100.0
    if families > 4:
        c = torch.tensor([4.0, -4.0, 8.0, -8.0], device="cuda")[torch.arange(m, device="cuda") % 4] if const is None else const
        rows = fam == 4
        x[rows] = c[rows, None].expand(-1, n)
    return x


def _ln64(torch, x64, gamma, beta, eps=EPS, xmag=None):
    """fp64 LayerNorm of [r][n] and the bound of a kernel that rounds its output once to bf16"""
    g = gamma.double()
    b = beta.double()
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x64 - mean) * rstd
    ref = xh * g + b
    mag = x64.abs() if xmag is None else xmag
    # rows constant in bf16 (var = 0) have an exact fp32 mean: no statistics term there
    stat = torch.where(var > 0, g.abs() * rstd * mag.mean(-1, keepdim=True), torch.zeros_like(ref))
    tol = 2.0 ** -8 * ((g * xh).abs() + b.abs()) + 2.0 ** -17 * (stat + (g * xh).abs() + b.abs()) + 1e-6
    if xmag is not None:   # the input itself summed in fp32 (embedding: 2 u of the three rows' magnitudes)
        tol = tol + torch.where(var > 0, 4 * U * g.abs() * rstd * xmag, torch.zeros_like(ref))
    return ref, tol, mean, rstd, xh


def _assert_within(name, got, ref, tol, ratios=None):
    err = (got.double() - ref).abs()
    bad = err > tol
    worst = float((err / tol).max())
    if ratios is not None:
        ratios.append(worst)
    assert not bool(bad.any()), "%s: %d elements over the bound, worst err/bound %.3f at %s" % (
        name, int(bad.sum()), worst, tuple(int(i) for i in np.unravel_index(int((err / tol).argmax()), tuple(err.shape))))
    return worst


def _ulp_bf16(y):
    import torch
    _, e = torch.frexp(y)
    return torch.ldexp(torch.ones_like(y), (e - 8).to(torch.int32))


# ------------------------------------------------------------------------------------------------- a. embedding + LN
def _embed_case(torch, hidden, lens, vocab, max_pos, seed, ids_override=None):
    g = _gen(torch, seed)
    te = (torch.round(torch.randn((hidden,), generator=g, device="cuda") * 8).clamp(-16, 16) / 16).bfloat16()
    fam_n = 5
    word32 = _family_rows(torch, g, vocab, hidden, fam_n)
    word32[torch.arange(vocab, device="cuda") % fam_n == 4] -= te.float()   # constant rows: word + type0 = c exactly
    word = word32.bfloat16()
    pos = (torch.randn((max_pos, hidden), generator=g, device="cuda") * 0.5).bfloat16()
    pos[0::2] = 0                                                           # (constant rows at even positions)
    gamma, beta = _gamma_beta(torch, g, hidden)
    cu = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    total = int(cu[-1])
    if ids_override is None:
        ids = torch.randint(0, vocab, (total,), generator=g, device="cuda", dtype=torch.int32)
        ids[0] = 0
        ids[-1] = vocab - 1
        ids[total // 2] = vocab - 1
    else:
        ids = ids_override
    d_cu = torch.from_numpy(cu).cuda()
    out = torch.full((total + 5, hidden), SENT, dtype=torch.bfloat16, device="cuda")
    _call("rass_embed_layernorm_bf16", _vp(ids), _vp(d_cu), len(lens), total, _vp(word), _vp(pos), _vp(te), _vp(gamma),
          _vp(beta), ctypes.c_float(EPS), hidden, vocab, max_pos, _vp(out), _st(torch))
    torch.cuda.synchronize()
    assert bool((out[total:] == SENT).all())
    # reference: the documented clamps, positions restart in every sequence
    idc = ids.long().clone()
    idc[(idc < 0) | (idc >= vocab)] = 0
    p = torch.from_numpy(np.concatenate([np.arange(n) for n in lens] or [np.zeros(0)]).astype(np.int64)).cuda()
    p = p.clamp(max=max_pos - 1)
    w, pe, t = word[idc].double(), pos[p].double(), te.double()[None, :]
    x64 = w + t + pe
    ref, tol, _, _, _ = _ln64(torch, x64, gamma, beta, xmag=w.abs() + t.abs() + pe.abs())
    got = out[:total]
    return got, ref, tol, beta, idc, p


@pytest.mark.parametrize("hidden", HIDDENS)
def test_embedding_layernorm(gpu, hidden):
    torch = gpu
    lens = [1, 2, 0, 511, 512]                      # an empty sequence in the middle of cu
    got, ref, tol, beta, idc, p = _embed_case(torch, hidden, lens, 1000, 512, seed=hidden)
    w = _assert_within("embed+LN hidden %d" % hidden, got, ref, tol)
    # constant rows (word + type0 = c exactly, an all-zero position row) come back as beta
    const = ((idc % 5) == 4) & ((p % 2) == 0)
    assert int(const.sum()) > 0
    assert torch.equal(got[const], beta.bfloat16()[None, :].expand(int(const.sum()), -1))
    print("embed+LN hidden %d: worst err/bound %.3f" % (hidden, w))


def test_embedding_layernorm_clamps(gpu):
    """ids < 0 or >= vocab read row 0; positions >= max_pos read row max_pos - 1"""
    torch = gpu
    lens = [40, 300]
    vocab, max_pos = 500, 256
    g = _gen(torch, 99)
    ids = torch.randint(0, vocab, (sum(lens),), generator=g, device="cuda", dtype=torch.int32)
    ids[3], ids[4], ids[5], ids[50] = -1, vocab, 1 << 30, -(1 << 30)
    got, ref, tol, *_ = _embed_case(torch, 1024, lens, vocab, max_pos, seed=7, ids_override=ids)
    _assert_within("embed clamps", got, ref, tol)
    # the same row read through a clamp and directly: identical bits
    ids2 = ids.clone()
    ids2[3], ids2[4], ids2[5], ids2[50] = 0, 0, 0, 0
    got2, *_ = _embed_case(torch, 1024, lens, vocab, max_pos, seed=7, ids_override=ids2)
    assert torch.equal(got, got2)


# ------------------------------------------------------------------------------------------------- b. layernorm_kernel
def _layernorm(torch, x, gamma, beta, rows, hidden, pad=3):
    out = torch.full((rows + pad, hidden), SENT, dtype=torch.bfloat16, device="cuda")
    _call("rass_layernorm_bf16", _vp(x), _vp(gamma), _vp(beta), ctypes.c_float(EPS), rows, hidden, _vp(out), _st(torch))
    torch.cuda.synchronize()
    assert bool((out[rows:] == SENT).all())
    return out[:rows]


@pytest.mark.parametrize("rows", [1, 37, 4095, 4096, 8192 + 13])
@pytest.mark.parametrize("hidden", HIDDENS)
def test_layernorm_kernel(gpu, hidden, rows, monkeypatch):
    torch = gpu
    g = _gen(torch, hidden * 31 + rows)
    x = _family_rows(torch, g, rows, hidden).bfloat16()
    gamma, beta = _gamma_beta(torch, g, hidden)
    monkeypatch.delenv("RASS_LN_NT", raising=False)
    got = _layernorm(torch, x, gamma, beta, rows, hidden)
    sel = torch.from_numpy(_ref_rows(rows)).cuda()
    ref, tol, _, _, _ = _ln64(torch, x[sel].double(), gamma, beta)
    w = _assert_within("layernorm %d x %d" % (rows, hidden), got[sel], ref, tol)
    const = sel[(sel % 5) == 4]
    if len(const):
        assert torch.equal(got[const], beta.bfloat16()[None, :].expand(len(const), -1))
    if rows >= 4096:   # every RASS_LN_NT value (nontemporal loads / stores): the same bits
        for mode in "0123":
            monkeypatch.setenv("RASS_LN_NT", mode)
            assert torch.equal(_layernorm(torch, x, gamma, beta, rows, hidden), got), mode
    print("layernorm %d x %d: worst err/bound %.3f" % (rows, hidden, w))


# --------------------------------------------------------------------------------------------- c. residual + LayerNorm
_RES_CASES = [  # (m, n, k, ws?, forced RASS_GEMM_SPLITK_S)
    (1, 1024, 4096, True, None), (16, 1024, 4096, True, None), (17, 1024, 4096, True, None), (64, 1024, 4096, True, None),
    (1, 1024, 1024, True, None), (16, 1024, 1024, True, None),
    (65, 1024, 1024, True, None), (65, 1024, 1024, True, 2), (100, 1024, 4096, True, None), (200, 1024, 4096, True, None),
    (300, 1024, 4096, True, None),
    (1, 768, 4096, True, None), (17, 768, 4096, True, None), (64, 768, 4096, True, None), (65, 768, 1024, True, None),
    (300, 768, 4096, True, None),
    (150, 1024, 1024, True, None), (300, 768, 1024, True, None),
    (17, 1024, 4096, False, None), (300, 768, 1024, False, None), (64, 1024, 1024, False, None),
]
_WS_FLOATS = 16 * 384 * 1024


def _res_id(c):
    m, n, k, ws, s = c
    return "m%d-n%d-k%d-%s" % (m, n, k, _residual_branch(m, (m + 255) // 256 * 256, n, k, _WS_FLOATS * 4 if ws else 0, s))


def test_residual_cases_cover_every_branch():
    names = {_res_id(c).split("-")[-1] for c in _RES_CASES}
    for b in ("fewrows4+ln_exact", "fewrows+pair", "splitk2+ln_exact", "splitk4+ln_exact", "splitk8+ln_exact",
              "splitk16+ln", "splitk4+ln", "splitk8+ln", "pair"):
        assert b in names, (b, sorted(names))


def _run_res(torch, X, W, bias, R0, gamma, beta, m, m_pad, n, k, ws):
    out = R0.clone()                                     # residual aliased to out, as the encoder calls it
    y = torch.full((m_pad, n), SENT, dtype=torch.bfloat16, device="cuda")
    _call("rass_gemm_bf16_residual_layernorm", _vp(X), _vp(W), _vp(bias), _vp(out), _vp(y), _vp(gamma), _vp(beta),
          ctypes.c_float(EPS), _vp(out), m, m_pad, n, k, _vp(ws), ws.numel() * 4 if ws is not None else 0, _st(torch))
    torch.cuda.synchronize()
    return out, y


@pytest.mark.parametrize("case", _RES_CASES, ids=_res_id)
def test_gemm_residual_layernorm(gpu, case, monkeypatch):
    torch = gpu
    m, n, k, use_ws, forced = case
    m_pad = (m + 255) // 256 * 256
    branch = _res_id(case).split("-")[-1]
    for v in ("RASS_LN_EXACT", "RASS_GEMM_SPLITK_S", "RASS_GEMM_FEWROWS"):
        monkeypatch.delenv(v, raising=False)
    if forced:
        monkeypatch.setenv("RASS_GEMM_SPLITK_S", str(forced))
    g = _gen(torch, m * 7 + n + k)
    fam = torch.arange(m, device="cuda") % 5
    X = torch.zeros((m_pad, k), dtype=torch.bfloat16, device="cuda")
    X[:m] = torch.randn((m, k), generator=g, device="cuda").bfloat16()
    X[:m][fam == 4] = 0                                  # constant rows: the LayerNorm input is bias + residual
    W = (torch.randn((n, k), generator=g, device="cuda") / k ** 0.5).bfloat16()
    bias = torch.round(torch.randn((n,), generator=g, device="cuda") * 8).clamp(-16, 16) / 16   # multiples of 1/16
    res32 = _family_rows(torch, g, m, n)
    res32[fam == 4] -= bias                              # b + res = +-4 / +-8 exactly (bf16-representable)
    R0 = torch.full((m_pad, n), SENT, dtype=torch.bfloat16, device="cuda")
    R0[:m] = res32.bfloat16()
    gamma, beta = _gamma_beta(torch, g, n)
    ws = torch.empty((_WS_FLOATS,), dtype=torch.float32, device="cuda") if use_ws else None

    out, y = _run_res(torch, X, W, bias, R0, gamma, beta, m, m_pad, n, k, ws)
    assert bool((out[m:] == SENT).all()) and bool((y[m:] == SENT).all())   # nothing past m
    got = out[:m]

    # fp64 reference, y rounded to bf16 where the kernels round it
    x64, w64, r64 = X[:m].double(), W.double(), R0[:m].double()
    y64 = x64 @ w64.T + bias.double() + r64
    y_bf = y64.float().bfloat16().double()
    e_y = (k + 3) * U * (x64.abs() @ w64.abs().T + bias.double().abs() + r64.abs())
    ulp = _ulp_bf16(y_bf.float()).double()
    flip = (y64 - y_bf).abs() >= ulp / 2 - e_y
    ref, tol, _, rstd, xh = _ln64(torch, y_bf, gamma, beta)
    ga = gamma.double().abs()
    row = (flip * ulp * (1 + xh.abs())).sum(-1, keepdim=True) / n
    tol = tol + flip * ga * rstd * ulp + ga * rstd * (1 + xh.abs()) * row
    w = _assert_within("residual+LN %s" % branch, got, ref, tol)
    const = torch.nonzero(fam == 4).flatten()
    if len(const):
        assert torch.equal(got[const], beta.bfloat16()[None, :].expand(len(const), -1))

    if branch.endswith("pair"):                           # y written: the GEMM, then rass_layernorm_bf16 of it
        _assert_within("residual+LN y", y[:m], y64, 1.5 * 2.0 ** -8 * y64.abs() + 2e-3)
        assert torch.equal(got, _layernorm(torch, y[:m].contiguous(), gamma, beta, m, n))
    else:                                                 # one reduce + residual + LayerNorm launch: y is not written
        assert bool((y == SENT).all())
    if branch.startswith("splitk"):
        # "the same bits" as the split-K GEMM with epilogue 1 and layernorm_kernel after it (encoder_kernels.h)
        monkeypatch.setenv("RASS_GEMM_FEWROWS", "0")
        y2 = torch.full((m_pad, n), SENT, dtype=torch.bfloat16, device="cuda")
        _call("rass_gemm_bf16_ws", _vp(X), _vp(W), _vp(bias), _vp(R0), _vp(y2), m, m_pad, n, k, 1, _vp(ws), ws.numel() * 4,
              _st(torch))
        torch.cuda.synchronize()
        monkeypatch.delenv("RASS_GEMM_FEWROWS")
        assert torch.equal(got, _layernorm(torch, y2[:m].contiguous(), gamma, beta, m, n))
    if branch.endswith("_exact"):                         # RASS_LN_EXACT=0: the general kernel, the same bits
        monkeypatch.setenv("RASS_LN_EXACT", "0")
        out0, _ = _run_res(torch, X, W, bias, R0, gamma, beta, m, m_pad, n, k, ws)
        assert torch.equal(out0, out)
    print("residual+LN m %d n %d k %d [%s]: worst err/bound %.3f" % (m, n, k, branch, w))


# ------------------------------------------------------------------------------ d. LayerNorm inside the query GEMM
@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("n", [1024, 3072, 4096])
@pytest.mark.parametrize("m", [1, 12, 16, 17, 32])
def test_gemm_ln_input(gpu, m, n, epi, monkeypatch):
    torch = gpu
    g = _gen(torch, m * 3 + n + epi)
    yin = _family_rows(torch, g, m, 1024).bfloat16()
    gamma, beta = _gamma_beta(torch, g, 1024)
    W = (torch.randn((n, 1024), generator=g, device="cuda") / 32).bfloat16()
    bias = torch.randn((n,), generator=g, device="cuda") * 0.1
    ln_bits = _layernorm(torch, yin, gamma, beta, m, 1024)
    lnr, tol_ln, _, _, _ = _ln64(torch, yin.double(), gamma, beta)
    pre = lnr @ W.double().T + bias.double()
    ref = torch.nn.functional.gelu(pre) if epi == 2 else pre
    tol = 1.5 * 2.0 ** -8 * ref.abs() + 2e-3 + (1.13 if epi == 2 else 1.0) * (tol_ln @ W.double().abs().T)
    worst = []
    for waves in ("16", "4"):
        if waves == "4":
            monkeypatch.setenv("RASS_GEMM_LNIN_WAVES", "4")
        else:
            monkeypatch.delenv("RASS_GEMM_LNIN_WAVES", raising=False)
        x_out = torch.full((m + 2, 1024), SENT, dtype=torch.bfloat16, device="cuda")
        y = torch.full((m + 2, n), SENT, dtype=torch.bfloat16, device="cuda")
        _call("rass_gemm_bf16_ln_input", _vp(yin), _vp(gamma), _vp(beta), ctypes.c_float(EPS), _vp(x_out), _vp(W), _vp(bias),
              _vp(y), m, n, 1024, epi, _st(torch))
        torch.cuda.synchronize()
        assert bool((x_out[m:] == SENT).all()) and bool((y[m:] == SENT).all())
        assert torch.equal(x_out[:m], ln_bits), waves     # "the bits launch_layernorm would write"
        _assert_within("ln-input GEMM waves %s" % waves, y[:m], ref, tol, worst)
    print("ln-input GEMM m %d n %d epi %d: worst err/bound %.3f" % (m, n, epi, max(worst)))


def test_gemm_ln_input_refuses_other_shapes(gpu):
    torch = gpu
    N_ = _lib()
    buf = torch.zeros((64 * 4096,), dtype=torch.bfloat16, device="cuda")
    f = torch.zeros((4096,), dtype=torch.float32, device="cuda")
    for (m, n, k) in [(0, 1024, 1024), (33, 1024, 1024), (16, 1000, 1024), (16, 512, 1024), (16, 1024, 768)]:
        rc = N_.lib().rass_gemm_bf16_ln_input(_vp(buf), _vp(f), _vp(f), ctypes.c_float(EPS), _vp(buf), _vp(buf), _vp(f),
                                              _vp(buf), m, n, k, 0, _st(torch))
        assert rc == -5, (m, n, k, rc)   # RASS_ERR_UNSUPPORTED
    rc = N_.lib().rass_gemm_bf16_ln_input(_vp(buf), _vp(f), _vp(f), ctypes.c_float(EPS), _vp(buf), _vp(buf), _vp(f), _vp(buf),
                                          16, 1024, 1024, 1, _st(torch))
    assert rc == -1                      # RASS_ERR_INVALID: epilogue 1
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------- e. LN fold chain
def _fold_gamma(torch, W, gamma, beta, bias):
    n, k = W.shape
    W2 = torch.empty_like(W)
    cs = torch.empty((n,), dtype=torch.float32, device="cuda")
    b2 = torch.empty((n,), dtype=torch.float32, device="cuda")
    _call("rass_fold_gamma_bf16", _vp(W), _vp(gamma), _vp(beta), _vp(bias), n, k, _vp(W2), _vp(cs), _vp(b2), _st(torch))
    torch.cuda.synchronize()
    # W' = bf16(W gamma) bit for bit; colsum / bias' against fp64 from the same bf16 values
    assert torch.equal(W2, (W.float() * gamma[None, :]).bfloat16())
    c = k // 64 + 8
    _assert_within("fold colsum", cs, W2.double().sum(1), c * U * W2.double().abs().sum(1) + 1e-30)
    wb = W.double() * beta.double()[None, :]
    _assert_within("fold bias'", b2, bias.double() + wb.sum(1), c * U * (bias.double().abs() + wb.abs().sum(1)) + 1e-30)
    return W2, cs, b2


def _fold_gemm(torch, X, W, bias, res, m, m_pad, n, k, epi, mr, gamma=None, beta=None, colsum=None):
    Y = torch.full((m_pad, n), SENT, dtype=torch.bfloat16, device="cuda")
    stats = torch.full((m_pad, n // 128, 2), SENT, dtype=torch.float32, device="cuda") if epi == 3 else None
    _call("rass_gemm_bf16_fold", _vp(X), _vp(W), _vp(bias), _vp(res), _vp(Y), m, m_pad, n, k, epi, _vp(mr), _vp(gamma),
          _vp(beta), _vp(stats), _vp(colsum), _st(torch))
    torch.cuda.synchronize()
    assert bool((Y[m:] == SENT).all())
    if stats is not None:
        assert bool((stats[m:] == SENT).all())
    return Y, stats


def _finalize(torch, stats, m, n):
    mr = torch.full(((m + 255) // 256 * 256 + 4, 2), SENT, dtype=torch.float32, device="cuda")
    _call("rass_ln_stats_finalize", _vp(stats), m, n, ctypes.c_float(EPS), _vp(mr), _st(torch))
    torch.cuda.synchronize()
    assert bool((mr[m:] == SENT).all())
    return mr


def _check_epi3(torch, X, W, bias, res, mr, gamma, beta, Y, stats, sel, n):
    x64, w64 = X[sel].double(), W.double()
    mu, rs = mr[sel, 0:1].double(), mr[sel, 1:2].double()
    r64 = res[sel].double()
    g64, b64 = gamma.double()[None, :], beta.double()[None, :]
    lnp = (r64 - mu) * rs * g64 + b64
    ref = x64 @ w64.T + bias.double() + lnp
    tol = 1.5 * 2.0 ** -8 * ref.abs() + 2e-3 + 2.0 ** -20 * (g64.abs() * r64.abs() * rs + b64.abs())
    w = _assert_within("EPI 3 r", Y[sel], ref, tol)
    yq = Y[sel].double().view(len(sel), n // 128, 128)
    _assert_within("EPI 3 sum r", stats[sel, :, 0], yq.sum(-1), 2.0 ** -17 * yq.abs().sum(-1) + 1e-30)
    _assert_within("EPI 3 sum r^2", stats[sel, :, 1], (yq * yq).sum(-1), 2.0 ** -17 * (yq * yq).sum(-1) + 1e-30)
    return w


def _check_finalize(torch, mr, Y, sel):
    r = Y[sel].double()
    mean = r.mean(-1)
    rstd = 1.0 / torch.sqrt(((r - mean[:, None]) ** 2).mean(-1) + EPS)
    _assert_within("finalize mean", mr[sel, 0], mean, 2.0 ** -16 * r.abs().mean(-1) + 1e-30)
    return _assert_within("finalize rstd", mr[sel, 1], rstd, 2.0 ** -11 * rstd)


def _check_epi45(torch, Yr, W2, b2_64, cs, mr, sel, epi, out, k, exact_stats):
    """out = epi(LN(r) W^T + b) via the fold, against fp64 x^ W'^T + bias' from fp64 statistics of the stored r"""
    r = Yr[sel].double()
    mean = r.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((r - mean) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (r - mean) * rstd
    w2 = W2.double()
    pre = xh @ w2.T + b2_64
    ref = torch.nn.functional.gelu(pre) if epi == 5 else pre
    extra = k * U * rstd * (r.abs() @ w2.abs().T)
    if not exact_stats:
        extra = extra + 2.0 ** -11 * (xh.abs() @ w2.abs().T) + rstd * 2.0 ** -16 * r.abs().mean(-1, keepdim=True) * cs.double().abs()
    tol = 1.5 * 2.0 ** -8 * ref.abs() + 2e-3 + (1.13 if epi == 5 else 1.0) * extra
    return _assert_within("EPI %d" % epi, out[sel], ref, tol), ref, tol


@pytest.mark.parametrize("m", [12288 + 37, 32768 + 101])
def test_ln_fold_chain(gpu, m):
    """One layer of the folded forward at H = 1024, I = 4096: attn-out (EPI 3, layer 0's identity LayerNorm) -> stats ->
    QKV (EPI 4) and FFN-up (EPI 5) on the raw rows -> FFN-down (EPI 3 with the real gamma / beta) -> stats; each stage
    against fp64 from its actual inputs, then FFN-up again from fp64 statistics (the stage alone), and the unfused pair
    (rass_layernorm_bf16, then rass_gemm_bf16) against the fold."""
    torch = gpu
    H, I = 1024, 4096
    m_pad = (m + 255) // 256 * 256
    g = _gen(torch, m)
    sel = torch.from_numpy(_ref_rows(m)).cuda()
    ctx = torch.zeros((m_pad, H), dtype=torch.bfloat16, device="cuda")
    ctx[:m] = torch.randn((m, H), generator=g, device="cuda").bfloat16()
    x0 = torch.full((m_pad, H), SENT, dtype=torch.bfloat16, device="cuda")
    x0[:m] = _family_rows(torch, g, m, H, families=4).bfloat16()   # iid / 8 sigma / 32 sigma / outlier
    Wo = (torch.randn((H, H), generator=g, device="cuda") / 32 * 0.25).bfloat16()
    bo = torch.randn((H,), generator=g, device="cuda") * 0.1
    ones = torch.ones((H,), dtype=torch.float32, device="cuda")
    zeros = torch.zeros((H,), dtype=torch.float32, device="cuda")
    mr_id = torch.zeros((m_pad, 2), dtype=torch.float32, device="cuda")
    mr_id[:, 1] = 1.0
    ratios = {}

    # attn-out, layer 0: LN_prev is the identity
    r1, st1 = _fold_gemm(torch, ctx, Wo, bo, x0, m, m_pad, H, H, 3, mr_id, ones, zeros)
    ratios["epi3 identity"] = _check_epi3(torch, ctx, Wo, bo, x0, mr_id, ones, zeros, r1, st1, sel, H)
    mr1 = _finalize(torch, st1, m, H)
    ratios["finalize"] = _check_finalize(torch, mr1, r1, sel)

    g1, b1 = _gamma_beta(torch, g, H)
    Wqkv = (torch.randn((3 * H, H), generator=g, device="cuda") / 32).bfloat16()
    bqkv = torch.randn((3 * H,), generator=g, device="cuda") * 0.1
    Wup = (torch.randn((I, H), generator=g, device="cuda") / 32).bfloat16()
    bup = torch.randn((I,), generator=g, device="cuda") * 0.1
    Wq2, csq, bq2 = _fold_gamma(torch, Wqkv, g1, b1, bqkv)
    Wu2, csu, bu2 = _fold_gamma(torch, Wup, g1, b1, bup)
    b2q64 = bqkv.double() + Wqkv.double() @ b1.double()
    b2u64 = bup.double() + Wup.double() @ b1.double()

    qkv, _ = _fold_gemm(torch, r1, Wq2, bq2, None, m, m_pad, 3 * H, H, 4, mr1, colsum=csq)
    ratios["epi4"] = _check_epi45(torch, r1, Wq2, b2q64, csq, mr1, sel, 4, qkv, H, False)[0]
    h, _ = _fold_gemm(torch, r1, Wu2, bu2, None, m, m_pad, I, H, 5, mr1, colsum=csu)
    ratios["epi5"], ref_f, tol_f = _check_epi45(torch, r1, Wu2, b2u64, csu, mr1, sel, 5, h, H, False)

    # the stage alone: (mean, rstd) from fp64
    r = r1[:m].double()
    mean = r.mean(-1)
    mr64 = torch.zeros((m_pad, 2), dtype=torch.float32, device="cuda")
    mr64[:m, 0] = mean.float()
    mr64[:m, 1] = (1.0 / torch.sqrt(((r - mean[:, None]) ** 2).mean(-1) + EPS)).float()
    h64, _ = _fold_gemm(torch, r1, Wu2, bu2, None, m, m_pad, I, H, 5, mr64, colsum=csu)
    ratios["epi5 exact stats"] = _check_epi45(torch, r1, Wu2, b2u64, csu, mr64, sel, 5, h64, H, True)[0]

    # the unfused pair on the same raw rows
    ln1 = _layernorm(torch, r1[:m].contiguous(), g1, b1, m, H)
    x_pad = torch.zeros((m_pad, H), dtype=torch.bfloat16, device="cuda")
    x_pad[:m] = ln1
    hp = torch.full((m_pad, I), SENT, dtype=torch.bfloat16, device="cuda")
    _call("rass_gemm_bf16", _vp(x_pad), _vp(Wup), _vp(bup), None, _vp(hp), m, m_pad, I, H, 2, _st(torch))
    torch.cuda.synchronize()
    lnr, tol_ln, _, _, _ = _ln64(torch, r1[sel].double(), g1, b1)
    pre_p = lnr @ Wup.double().T + bup.double()
    ref_p = torch.nn.functional.gelu(pre_p)
    tol_p = 1.5 * 2.0 ** -8 * ref_p.abs() + 2e-3 + 1.13 * (tol_ln @ Wup.double().abs().T)
    ratios["pair"] = _assert_within("unfused pair", hp[sel], ref_p, tol_p)
    ratios["fold vs pair"] = _assert_within("fold vs unfused pair", h[sel], hp[sel].double(),
                                            tol_f + tol_p + (ref_f - ref_p).abs())

    # FFN-down with the real LayerNorm rebuilt from (mr1, g1, b1) -> r2 and its statistics
    Wd = (torch.randn((H, I), generator=g, device="cuda") / 64 * 0.25).bfloat16()
    bd = torch.randn((H,), generator=g, device="cuda") * 0.1
    h[m:] = 0
    r2, st2 = _fold_gemm(torch, h, Wd, bd, r1, m, m_pad, H, I, 3, mr1, g1, b1)
    ratios["epi3 real"] = _check_epi3(torch, h, Wd, bd, r1, mr1, g1, b1, r2, st2, sel, H)
    mr2 = _finalize(torch, st2, m, H)
    ratios["finalize 2"] = _check_finalize(torch, mr2, r2, sel)
    print("LN fold m %d: worst err/bound %s" % (m, {k: round(v, 3) for k, v in ratios.items()}))


def test_ln_stats_finalize_alone(gpu):
    """(sum, sum of squares) per 128-column chunk computed in fp64 from bf16 rows and rounded to fp32 -> (mean, rstd): the
    one-pass variance within 2^-11 of fp64 up to |mean| / sigma = 32 (iid, 8 sigma, 32 sigma and outlier rows)"""
    torch = gpu
    m, n = 4099, 1024
    g = _gen(torch, 5)
    xb = _family_rows(torch, g, m, n, families=4).bfloat16().double()
    ch = xb.view(m, n // 128, 128)
    stats = torch.stack([ch.sum(-1), (ch * ch).sum(-1)], -1).float().contiguous()
    mr = _finalize(torch, stats, m, n)
    mean = xb.mean(-1)
    rstd = 1.0 / torch.sqrt(((xb - mean[:, None]) ** 2).mean(-1) + EPS)
    _assert_within("finalize mean", mr[:m, 0], mean, 2.0 ** -16 * xb.abs().mean(-1) + 1e-30)
    w = _assert_within("finalize rstd", mr[:m, 1], rstd, 2.0 ** -11 * rstd)
    print("finalize alone: worst err/bound %.3f" % w)


def test_fold_refuses_other_shapes(gpu):
    torch = gpu
    N_ = _lib()
    buf = torch.zeros((16,), dtype=torch.bfloat16, device="cuda")
    f = torch.zeros((16,), dtype=torch.float32, device="cuda")
    for (m, m_pad, n, k) in [(1000, 1024, 1024, 1024), (12288, 12288, 1000, 1024), (12288, 12288, 1024, 64),
                             (2048, 2048, 1024, 1024)]:   # (the last: 32 tiles of 256^2, < 192)
        rc = N_.lib().rass_gemm_bf16_fold(_vp(buf), _vp(buf), _vp(f), None, _vp(buf), m, m_pad, n, k, 4, _vp(f), None, None,
                                          None, _vp(f), _st(torch))
        assert rc == -5, (m, m_pad, n, k, rc)


# ----------------------------------------------------------------------------------------------------------- f. pooling
def _pool(torch, x, cu, nseq, hidden, mean, norm):
    d_cu = torch.from_numpy(cu).cuda()
    out = torch.full((nseq + 3, hidden), SENT, dtype=torch.float32, device="cuda")
    _call("rass_pool_bf16", _vp(x), _vp(d_cu), nseq, hidden, int(mean), int(norm), _vp(out), _st(torch))
    torch.cuda.synchronize()
    assert bool((out[nseq:] == SENT).all())
    return out[:nseq]


@pytest.mark.parametrize("hidden", [128, 384, 1000, 2048])
@pytest.mark.parametrize("nseq", [1, 40000])
def test_pool(gpu, hidden, nseq):
    torch = gpu
    rng = np.random.default_rng(hidden + nseq)
    if nseq == 1:
        lens = np.array([512])
    else:
        lens = rng.choice([0, 1, 7, 8, 9, 512], size=nseq, p=[0.1, 0.25, 0.2, 0.2, 0.248, 0.002])
        lens[:6] = [0, 1, 7, 8, 9, 512]
        lens[-1] = 0
        if hidden > 1000:
            lens = lens[:8000]
            nseq = len(lens)
    cu = np.zeros(nseq + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    total = int(cu[-1])
    g = _gen(torch, hidden)
    x = (torch.randn((total, hidden), generator=g, device="cuda") + 0.3).bfloat16()
    x64 = x.double()
    seg = torch.from_numpy(np.repeat(np.arange(nseq), lens)).cuda()
    sums = torch.zeros((nseq, hidden), dtype=torch.float64, device="cuda").index_add_(0, seg, x64)
    abs_sums = torch.zeros((nseq, hidden), dtype=torch.float64, device="cuda").index_add_(0, seg, x64.abs())
    n = torch.from_numpy(lens.astype(np.float64)).cuda()[:, None]
    first = torch.zeros((nseq, hidden), dtype=torch.float64, device="cuda")
    nz = torch.from_numpy(np.nonzero(lens)[0]).cuda()
    first[nz] = x64[torch.from_numpy(cu[:-1].astype(np.int64)).cuda()[nz]]
    empty = torch.from_numpy(lens == 0).cuda()
    for mode_mean in (0, 1):
        if mode_mean:
            e = torch.where(n > 0, sums / n.clamp(min=1), torch.zeros_like(sums))
            te = (n + 2) * U * abs_sums / n.clamp(min=1) + 1e-30
        else:
            e, te = first, torch.full_like(first, 1e-30)
        for norm in (0, 1):
            got = _pool(torch, x, cu, nseq, hidden, mode_mean, norm)
            assert bool(torch.isfinite(got).all())
            assert bool((got[empty] == 0).all())                        # empty sequences: zeros, not NaN
            if norm:
                d = e.norm(dim=-1, keepdim=True) + 1e-9
                ref = e / d
                tol = 64 * U * ref.abs() + (te + ref.abs() * te.norm(dim=-1, keepdim=True)) / d + 1e-30
            else:
                ref, tol = e, te
            w = _assert_within("pool mean=%d norm=%d" % (mode_mean, norm), got, ref, tol)
            print("pool hidden %d nseq %d mean %d norm %d: worst err/bound %.3f" % (hidden, nseq, mode_mean, norm, w))
