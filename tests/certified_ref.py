"""numpy restatement of the certified int8 search (prefilter mode 3, DESIGN.md §3 "certified int8 search"), built on
``oracle.quantize_i8``: the hi + lo query quantisation, the candidate score a(y), the 128-deep candidate lists with tau, the
row / query terms of the certificate's bound B_q and the certificate itself.  Every fp32 step is one IEEE operation, as on the
device, so candidate scores and lists are reproduced bit for bit."""
import numpy as np

from oracle.oracle import quantize_i8

F32 = np.float32
C = 128          # candidates per query
U = 2.0 ** -24   # fp32 unit roundoff


def query_hilo(qn):
    """q ~ s_hi q_hi + s_lo q_lo; q_lo quantises the fp32 residual q - s_hi * q_hi (one multiply, one subtract)."""
    qn = np.ascontiguousarray(qn, dtype=F32)
    qh, s_hi = quantize_i8(qn)
    r = (qn - (s_hi[:, None] * qh.astype(F32)).astype(F32)).astype(F32)
    ql, s_lo = quantize_i8(r)
    return qh, s_hi, ql, s_lo


def scores(xn, qn):
    """a(y) = s_y * (s_hi * (float)dot(y8, q_hi) + s_lo * (float)dot(y8, q_lo)), [nq, n] float32."""
    xq, sx = quantize_i8(xn)
    qh, s_hi, ql, s_lo = query_hilo(qn)
    X = xq.astype(np.float64)
    dh = (qh.astype(np.float64) @ X.T).astype(F32)   # exact integers, one rounding to fp32
    dl = (ql.astype(np.float64) @ X.T).astype(F32)
    t = ((s_hi[:, None] * dh).astype(F32) + (s_lo[:, None] * dl).astype(F32)).astype(F32)
    return (sx[None, :] * t).astype(F32)


def eligible(n, nq, tags=None, qfilter=None, qmask=None):
    ok = np.ones((nq, n), dtype=bool)
    if tags is not None:
        tags = np.asarray(tags)
        ok &= (tags != -1)[None, :]
        if qfilter is not None:
            m = np.full(nq, -1, dtype=np.int64) if qmask is None else np.asarray(qmask, dtype=np.int64)
            f = np.asarray(qfilter, dtype=np.int64)
            ok &= (f[:, None] < 0) | ((tags[None, :].astype(np.int64) & m[:, None]) == f[:, None])
    return ok


def candidates(xn, qn, tags=None, qfilter=None):
    """The 128 best eligible rows per query under (a desc, row asc) and tau: the 129th score when more than 128 rows are
    eligible, else -inf (a corpus of <= 16 384 rows: no sample floor on the device).  (scores [nq,128], rows [nq,128], tau)."""
    a = scores(xn, qn)
    nq, n = a.shape
    ok = eligible(n, nq, tags, qfilter)
    cs = np.full((nq, C), -np.inf, dtype=F32)
    cr = np.full((nq, C), -1, dtype=np.int64)
    tau = np.full(nq, -np.inf, dtype=F32)
    for q in range(nq):
        rows = np.nonzero(ok[q])[0]
        order = rows[np.lexsort((rows, -a[q, rows].astype(np.float64)))]
        top = order[:C]
        cs[q, :len(top)] = a[q, top]
        cr[q, :len(top)] = top
        if len(order) > C:
            tau[q] = a[q, order[C]]
    return cs, cr, tau


def row_terms(xn):
    """Per row: rho = |y - s_y y8|, nu = |s_y y8|, |y| (fp64)."""
    xn = np.asarray(xn, dtype=F32)
    xq, sx = quantize_i8(xn)
    yh = sx.astype(np.float64)[:, None] * xq.astype(np.float64)
    rho = np.sqrt(((xn.astype(np.float64) - yh) ** 2).sum(1))
    return rho, np.sqrt((yh ** 2).sum(1)), np.sqrt((xn.astype(np.float64) ** 2).sum(1))


def query_terms(qn):
    """Per query: |q|, rho_q = |q - s_hi q_hi - s_lo q_lo|, |s_hi q_hi| + |s_lo q_lo| (fp64)."""
    qh, s_hi, ql, s_lo = query_hilo(qn)
    q = np.asarray(qn, dtype=np.float64)
    ph = s_hi.astype(np.float64)[:, None] * qh
    pl = s_lo.astype(np.float64)[:, None] * ql
    return (np.sqrt((q ** 2).sum(1)), np.sqrt(((q - ph - pl) ** 2).sum(1)),
            np.sqrt((ph ** 2).sum(1)) + np.sqrt((pl ** 2).sum(1)))


def bound(R, V, Y, qnorm, rho_q, qa, D):
    """B_q = R |q| + V rho_q + gamma_D Y |q| + gamma_4 V (|s_hi q_hi| + |s_lo q_lo|)."""
    gD = D * U / (1 - D * U)
    g4 = 4 * U / (1 - 4 * U)
    return R * qnorm + V * rho_q + gD * Y * qnorm + g4 * V * qa
