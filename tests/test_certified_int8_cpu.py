"""CPU checks of the certified int8 search (prefilter mode 3): the certificate's bound is sound against fp64 for random and
adversarial rows (unnormalised and zero rows included), and the configuration accepts the mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import certified_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_bound(x, q):
    """|fl32 score - a(y)| <= B_q for every (row, query): the fp32 flat score in two different summation orders and the exact
    fp64 score, against the candidate score the int8 scan computes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    a = CR.scores(x, q).astype(np.float64)
    rho, nu, yn = CR.row_terms(x)
    qnorm, rq, qa = CR.query_terms(q)
    B = CR.bound(rho.max(), nu.max(), yn.max(), qnorm, rq, qa, x.shape[1])[:, None]
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    blas32 = (q @ x.T).astype(np.float64)
    seq32 = np.zeros((q.shape[0], x.shape[0]), dtype=np.float32)
    for c in range(x.shape[1]):                      # a left-to-right fp32 sum of fp32 products: another order
        seq32 = (seq32 + (q[:, c:c + 1] * x[None, :, c]).astype(np.float32)).astype(np.float32)
    for f in (exact, blas32, seq32.astype(np.float64)):
        assert np.all(np.abs(f - a) <= B), float((np.abs(f - a) - B).max())
    return B


@pytest.mark.parametrize("dim", [64, 384, 1024, 2048])
def test_bound_is_sound_on_random_rows(dim):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((300, dim)).astype(np.float32)
    x[:100] /= np.linalg.norm(x[:100], axis=1, keepdims=True)   # normalised rows, and rows that were not
    x[5] = 0.0                                                   # a zero row
    x[6] *= 1e-3
    q = rng.standard_normal((7, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    _check_bound(x, q)


def test_bound_is_sound_on_adversarial_rows():
    rng = np.random.default_rng(1)
    dim = 1024
    q = rng.standard_normal((4, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x = np.concatenate([
        q[0] + 1e-5 * rng.standard_normal((50, dim)).astype(np.float32),   # near-duplicates of a query
        rng.standard_normal((50, dim)).astype(np.float32) * np.float32(1e3),
        np.eye(dim, dtype=np.float32)[:20],                                 # one-hot rows: residual 0
        np.zeros((3, dim), dtype=np.float32),
    ])
    x[60, 7] = 1e7                                                          # an outlier component
    x[61, :] = np.float32(0.5) + np.arange(dim, dtype=np.float32) / np.float32(dim * 254)   # values between int8 steps
    B = _check_bound(x, q)
    assert np.all(B > 0)


def test_hi_lo_query_residual_is_small():
    rng = np.random.default_rng(2)
    q = rng.standard_normal((16, 1024)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qnorm, rq, _ = CR.query_terms(q)
    assert np.all(rq < 1e-4) and np.all(np.abs(qnorm - 1) < 1e-5)


def test_config_accepts_int8_exact():
    code = "from rassengine_amd import config; print(config.RASS_PREFILTER)"
    env = dict(os.environ, RASS_PREFILTER="int8_exact")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "int8_exact"
    env["RASS_PREFILTER"] = "int9"
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert bad.returncode != 0 and "int8_exact" in bad.stderr


def test_python_surface_knows_mode_3():
    from rassengine_amd.engine import FlatIndex
    assert FlatIndex.PREFILTER_MODES["int8_exact"] == 3
    assert hasattr(FlatIndex, "certify_stats") and hasattr(FlatIndex, "candidates_exact_device")
    hdr = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    assert "#define RASS_PREFILTER_INT8_EXACT 3" in hdr
