"""The encoder GEMM's routing rule against its Python mirror (CPU: loads librass_hip.so, touches no device).

rass_gemm_bf16_route answers, without a GPU, which kernel an entry point gives a shape (csrc/gemm_route.cpp).  The mirror
in tests/helpers.py states the same rule independently; the GPU tests predict their branch from it.  Here the two are
compared over the encoder's shapes with every RASS_GEMM_* switch at its default and at each of its A/B values, and the
boundaries DESIGN.md §4 documents are checked literally.  The library loads on a host without a GPU (the query needs no
device), so nothing here is skipped for want of one."""
import ctypes
import itertools

import pytest

from tests.helpers import _fold_branch, _gemm_branch, _ln_input_branch, _residual_branch

ROWS = [1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 300, 1024, 1025, 1536, 2048, 8192, 131072]
# (n, k) of QKV, attention-out, FFN-up, FFN-down of the hidden 1 024 / 4 096 and the 768 / 3 072 models
GEMMS = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (2304, 768), (768, 768), (3072, 768), (768, 3072)]
WS_BYTES = 16 * 384 * 1024 * 4     # the scratch the GPU tests lend
ENTRY_GEMM, ENTRY_RESIDUAL, ENTRY_LN_INPUT, ENTRY_FOLD = 0, 1, 2, 3

# (environment, the mirror's switches): the default and each A/B value of every switch.  RASS_GEMM_GRID, RASS_P5_POLICY
# and RASS_ENCODER_LN_FOLD change launch parameters or the encoder's choice of entry point, not a kernel kind: their
# labels must equal the default's.
SETTINGS = [
    ({}, {}),
    ({"RASS_GEMM_FEWROWS": "0"}, {"fewrows": False}),
    ({"RASS_GEMM_FEWROWS_MAX": "128"}, {"fewrows_max": 128}),
    ({"RASS_GEMM_FEWROWS_MAX": "64"}, {"fewrows_max": 64}),
    ({"RASS_GEMM_FEWROWS_MAX": "1"}, {"fewrows_max": 16}),        # clamped to 16 .. 128
    ({"RASS_GEMM_FEWROWS_MAX": "500"}, {"fewrows_max": 128}),
    ({"RASS_GEMM_FEWROWS_RES": "32"}, {"fewrows_res": 32}),
    ({"RASS_GEMM_MID": "0"}, {"mid": 0}),
    ({"RASS_GEMM_MID": "2"}, {"mid": 2}),
    ({"RASS_GEMM_VARIANT": "p4"}, {"variant": "p4"}),
    ({"RASS_GEMM_VARIANT": "p5"}, {"variant": "p5"}),
    ({"RASS_GEMM_SPLITK_S": "2"}, {"splitk_s": 2}),
    ({"RASS_GEMM_SPLITK_S": "4"}, {"splitk_s": 4}),
    ({"RASS_GEMM_SPLITK_S": "8"}, {"splitk_s": 8}),
    ({"RASS_GEMM_SPLITK_S": "16"}, {"splitk_s": 16}),
    ({"RASS_GEMM_MID_BM": "64"}, {"mid_bm": 64}),
    ({"RASS_GEMM_MID_BM": "128"}, {"mid_bm": 128}),
    ({"RASS_GEMM_LNIN_WAVES": "4"}, {"lnin_waves": 4}),
    ({"RASS_GEMM_GRID": "64"}, {}),
    ({"RASS_P5_POLICY": "0"}, {}),
    ({"RASS_ENCODER_LN_FOLD": "0"}, {}),
]
SWITCHES = ["RASS_GEMM_FEWROWS", "RASS_GEMM_FEWROWS_MAX", "RASS_GEMM_FEWROWS_RES", "RASS_GEMM_MID", "RASS_GEMM_VARIANT",
            "RASS_GEMM_SPLITK_S", "RASS_GEMM_MID_BM", "RASS_GEMM_LNIN_WAVES", "RASS_GEMM_GRID", "RASS_P5_POLICY",
            "RASS_ENCODER_LN_FOLD"]


@pytest.fixture(scope="module")
def route():
    from rassengine_amd import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(32)

    def ask(entry, m, m_pad, n, k, epi, ws_bytes):
        _native.check("rass_gemm_bf16_route", lib.rass_gemm_bf16_route(entry, m, m_pad, n, k, epi, ws_bytes, buf, len(buf)))
        return buf.value.decode()
    return ask


def _pad(m):
    return (m + 255) // 256 * 256


def _set(monkeypatch, env):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join("%s=%s" % kv for kv in s[0].items()) or "default")
def test_route_equals_mirror(route, setting, monkeypatch):
    env, sw = setting
    _set(monkeypatch, env)
    n_checked, kinds = 0, set()
    for m, (n, k), ws in itertools.product(ROWS, GEMMS, (0, WS_BYTES)):
        mp = _pad(m)
        for epi in (0, 1, 2):
            want = _gemm_branch(m, mp, n, k, epi, ws, sw)
            got = route(ENTRY_GEMM, m, mp, n, k, epi, ws)
            assert got == want, ("gemm_ws", env, m, n, k, epi, ws, got, want)
            kinds.add(got)
            n_checked += 1
        want = _residual_branch(m, mp, n, k, ws, sw=sw).replace("_exact", "")   # (_exact: which LayerNorm kernel follows)
        got = route(ENTRY_RESIDUAL, m, mp, n, k, 1, ws)
        assert got == want, ("residual_layernorm", env, m, n, k, ws, got, want)
        kinds.add(got)
        for epi in (0, 2):
            assert route(ENTRY_LN_INPUT, m, mp, n, k, epi, 0) == _ln_input_branch(m, n, k, sw), ("ln_input", env, m, n, k, epi)
        for epi in (3, 4, 5):
            want = _fold_branch(m, mp, n, k, epi, sw)
            got = route(ENTRY_FOLD, m, mp, n, k, epi, 0)
            assert got == want, ("fold", env, m, n, k, epi, got, want)
            kinds.add(got)
        n_checked += 6
    if not env:   # the default rule reaches every kind of kernel on this grid
        for kind in ("fewrows4", "fewrows16", "splitk4", "splitk8", "mid64", "mid128", "tile128", "p4", "p5", "fewrows4+ln",
                     "fewrows+pair", "splitk8+ln", "pair", "unsupported"):
            assert kind in kinds, (kind, sorted(kinds))
    print("%d routes equal the mirror (%s)" % (n_checked, env or "default"))


def test_design_boundaries(route, monkeypatch):
    """DESIGN.md §4, literally."""
    _set(monkeypatch, {})
    ws = WS_BYTES
    # 96 -> 97 rows: few-rows to mid (K = 1 024; the QKV projection and FFN-up)
    for n in (3072, 4096):
        assert route(ENTRY_GEMM, 96, 256, n, 1024, 0, ws) == "fewrows4"
        assert route(ENTRY_GEMM, 97, 256, n, 1024, 0, ws).startswith("mid")
    # 1 024 -> 1 025 rows: mid ends
    for n, k in ((1024, 1024), (3072, 1024)):
        assert route(ENTRY_GEMM, 1024, 1024, n, k, 0, 0).startswith("mid")
        assert not route(ENTRY_GEMM, 1025, 1280, n, k, 0, 0).startswith("mid")
    assert route(ENTRY_GEMM, 1536, 1536, 1024, 1024, 0, 0) == "tile128"
    # 192 tiles of 256 x 256: persistent begins (N = 1 024: 4 tiles per 256 rows)
    assert route(ENTRY_GEMM, 47 * 256, 47 * 256, 1024, 1024, 0, 0) == "tile128"
    assert route(ENTRY_GEMM, 48 * 256, 48 * 256, 1024, 1024, 0, 0) == "p4"
    assert route(ENTRY_FOLD, 47 * 256, 47 * 256, 1024, 1024, 3, 0) == "unsupported"
    assert route(ENTRY_FOLD, 48 * 256, 48 * 256, 1024, 1024, 3, 0) == "p4"
    # EPI 5 (the folded GELU epilogue) stays on p5; RASS_GEMM_VARIANT=p4 asks for p4 everywhere
    assert route(ENTRY_FOLD, 131072, 131072, 4096, 1024, 4, 0) == "p4"
    assert route(ENTRY_FOLD, 131072, 131072, 4096, 1024, 5, 0) == "p5"
    monkeypatch.setenv("RASS_GEMM_VARIANT", "p4")
    assert route(ENTRY_FOLD, 131072, 131072, 4096, 1024, 5, 0) == "p4"
    monkeypatch.delenv("RASS_GEMM_VARIANT")
    # residual few-rows applies up to 64 rows
    assert route(ENTRY_RESIDUAL, 64, 256, 1024, 4096, 1, ws) == "fewrows4+ln"
    assert route(ENTRY_RESIDUAL, 65, 256, 1024, 4096, 1, ws) == "splitk16+ln"
    assert route(ENTRY_RESIDUAL, 64, 256, 1024, 1024, 1, ws) == "fewrows+pair"
    assert route(ENTRY_RESIDUAL, 65, 256, 1024, 1024, 1, ws) == "splitk4+ln"


def test_route_refuses_bad_arguments(route):
    from rassengine_amd import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(32)
    assert lib.rass_gemm_bf16_route(7, 1, 128, 1024, 1024, 0, 0, buf, len(buf)) != 0
    assert lib.rass_gemm_bf16_route(0, 1, 128, 1024, 1024, 0, 0, None, 0) != 0
    assert route(ENTRY_GEMM, 12, 128, 1000, 1024, 0, 0) == "unsupported"      # n % 128
    assert route(ENTRY_GEMM, 12, 128, 1024, 1024, 4, 0) == "unsupported"      # gemm_ws takes epilogue 0 / 1 / 2
    short = ctypes.create_string_buffer(4)                                     # a short buffer is cut, NUL-terminated
    assert lib.rass_gemm_bf16_route(0, 1536, 1536, 1024, 1024, 0, 0, short, len(short)) == 0 and short.value == b"til"
