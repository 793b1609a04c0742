"""The host-side layers of the IVF probe within a row bitmap, without a GPU: the byte rule ``IvfPolicy.allow_route`` against its
numpy restatement, the ``allow_probe`` switch and ``RASS_IVF_ALLOW``, the routing of ``IvfBackedIndex.search_allowed`` over a
stand-in IVF, the numpy restatements themselves, and the new entry points' presence in the header and the binding table."""
import importlib
import os
import re

import numpy as np
import pytest

from rassengine_amd import _native, config
from rassengine_amd.engine import FlatIndex, pack_allow
from rassengine_amd.ivf import IvfBackedIndex, IvfPolicy
from tests.ivf_allow_ref import member_bits, route, slab_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("rass_ivf_search_allowed_delta", "rass_ivf_search_allowed_delta_device", "rass_ivf_probe_lists",
                    "rass_index_allow_count")


# ---------------------------------------------------------------------------------------------- the byte rule
def test_allow_route_equals_the_byte_rule_on_a_grid():
    rng = np.random.default_rng(3)
    p = IvfPolicy(nlist=64, nprobe=4, allow_probe=True)
    seen = set()
    for covered, nlist in ((0, 16), (20_000, 64), (12_500_000, 4096), (6_016, 16)):
        for nprobe in (1, 2, 8, 64):
            for nq in (1, 17, 32, 40, 70):
                for scale in (0, 1, 30, 3_000, 400_000):
                    for shared in (False, True):
                        counts = rng.integers(0, scale + 1, size=1 if shared else nq)
                        got = p.allow_route(counts, nq, shared, nprobe, covered, nlist)
                        assert got == route(counts, nq, shared, nprobe, covered, nlist), (covered, nlist, nprobe, nq, scale, shared)
                        seen.add(got)
    assert seen == {"ivf", "flat"}


def test_allow_route_boundary_groups_and_factor():
    p = IvfPolicy()
    # probe rows = 8 * 32_000 / 64 = 4_000 = 32 * 125: equality goes to flat, one more allowed row to the IVF
    assert p.allow_route([125], 5, True, 8, 32_000, 64) == "flat"
    assert p.allow_route([126], 5, True, 8, 32_000, 64) == "ivf"
    # per-query counts add up over a launch group of 32; the call's LARGEST group decides
    assert p.allow_route([4] * 31 + [1], 32, False, 8, 32_000, 64) == "flat"      # C = 125
    assert p.allow_route([4] * 31 + [2], 32, False, 8, 32_000, 64) == "ivf"       # C = 126
    assert p.allow_route([0] * 32 + [126], 33, False, 8, 32_000, 64) == "ivf"     # the second group alone
    assert p.allow_route([3] * 32 + [3] * 8, 40, False, 8, 32_000, 64) == "flat"  # 96 and 24: neither group reaches it
    # a shared bitmap counts once however many queries share it
    assert p.allow_route([125], 32, True, 8, 32_000, 64) == "flat"
    # covered = 0: the probe streams nothing — any non-empty bitmap goes to the IVF form (whose delta scan is the flat scan),
    # an empty one stays flat
    assert p.allow_route([1], 1, True, 8, 0, 64) == "ivf"
    assert p.allow_route([0], 1, True, 8, 0, 64) == "flat"
    assert p.allow_route([], 0, False, 8, 32_000, 64) == "flat"
    # the factor scales the probe's side
    assert IvfPolicy(allow_exact_factor=2.0).allow_route([250], 1, True, 8, 32_000, 64) == "flat"
    assert IvfPolicy(allow_exact_factor=2.0).allow_route([251], 1, True, 8, 32_000, 64) == "ivf"
    assert IvfPolicy(allow_exact_factor=0.5).allow_route([63], 1, True, 8, 32_000, 64) == "ivf"


def test_allow_probe_is_off_by_default_and_follows_the_environment(monkeypatch):
    assert IvfPolicy().allow_probe is False and IvfPolicy().allow_exact_factor == 1.0
    assert IvfPolicy.manual().allow_probe is False
    try:
        for value, want in ((None, False), ("0", False), ("1", True), (" 1 ", True), ("yes", False), ("", False)):
            if value is None:
                monkeypatch.delenv("RASS_IVF_ALLOW", raising=False)
            else:
                monkeypatch.setenv("RASS_IVF_ALLOW", value)
            importlib.reload(config)
            assert config.RASS_IVF_ALLOW is want, value
            assert IvfPolicy.from_config().allow_probe is want
    finally:
        monkeypatch.undo()
        importlib.reload(config)


# ---------------------------------------------------------------------------------------------- the routing of search_allowed
class FakeIvf:
    def __init__(self, dtype="f32", covered=32_000, nlist=64):
        self.dtype, self.covered_rows, self.nlist = dtype, covered, nlist
        self.calls = []

    def search_allowed_delta(self, flat, queries, k, nprobe, allow, q_filter=None, q_filter_mask=None):
        self.calls.append((k, nprobe, tuple(allow.shape), q_filter, q_filter_mask))
        return "ivf-scores", "ivf-ids", 7


class BackedStandIn(IvfBackedIndex):
    """``IvfBackedIndex.search_allowed`` over a stand-in IVF: no engine, no handle; ``rows`` and the bitmap counts are given."""
    rows = 32_000
    counts = np.array([20_000])

    def __init__(self, policy, ivf):
        self.policy, self.ivf, self.ivf_allowed = policy, ivf, 0

    def allow_count(self, allow):
        return self.counts


@pytest.fixture()
def flat_calls(monkeypatch):
    calls = []

    def fake(self, queries, k, allow, q_filter=None, q_filter_mask=None):
        calls.append((k, tuple(np.shape(allow)), q_filter, q_filter_mask))
        return "flat-scores", "flat-ids"
    monkeypatch.setattr(FlatIndex, "search_allowed", fake)
    return calls


def test_search_allowed_routes_by_switch_exact_k_dtype_and_bytes(flat_calls):
    q = np.zeros((3, 8), dtype=np.float32)
    allow = np.zeros(1000, dtype=np.uint32)
    on = IvfPolicy(nlist=64, nprobe=8, allow_probe=True)
    # the IVF serves a broad bitmap when everything holds, with the policy's nprobe or the call's
    idx = BackedStandIn(on, FakeIvf())
    assert idx.search_allowed(q, 10, allow) == ("ivf-scores", "ivf-ids") and idx.ivf_allowed == 1 and not flat_calls
    f, m = np.arange(3, dtype=np.int32), np.full(3, 0xFFFFFF, dtype=np.int32)
    idx.search_allowed(q, 32, allow, f, m, nprobe=3)
    assert idx.ivf.calls == [(10, 8, (1000,), None, None), (32, 3, (1000,), f, m)]
    # ... and the flat method takes every other case, with the caller's arguments
    for kwargs, k, ivf, policy in (
            (dict(exact=True), 10, FakeIvf(), on),
            ({}, 33, FakeIvf(), on),
            ({}, 10, FakeIvf(dtype="bf16"), on),
            ({}, 10, FakeIvf(dtype="int8"), on),
            ({}, 10, None, on),
            ({}, 10, FakeIvf(), IvfPolicy(nlist=64, nprobe=8))):           # the switch is off by default
        del flat_calls[:]
        idx = BackedStandIn(policy, ivf)
        assert idx.search_allowed(q, k, allow, f, m, **kwargs) == ("flat-scores", "flat-ids"), (kwargs, k)
        assert flat_calls == [(k, (1000,), f, m)] and idx.ivf_allowed == 0 and (ivf is None or not ivf.calls)
    # a selective bitmap: the byte rule keeps it flat (8 * 32 000 / 64 = 4 000 rows probed against 32 * 125)
    del flat_calls[:]
    idx = BackedStandIn(on, FakeIvf())
    idx.counts = np.array([125])
    assert idx.search_allowed(q, 10, allow)[0] == "flat-scores" and not idx.ivf.calls
    idx.counts = np.array([126])
    assert idx.search_allowed(q, 10, allow)[0] == "ivf-scores"
    # a bitmap shorter than the index needs now goes to the flat method, which extends it
    del flat_calls[:]
    assert idx.search_allowed(q, 10, np.zeros(999, dtype=np.uint32))[0] == "flat-scores" and flat_calls[0][1] == (999,)


# ---------------------------------------------------------------------------------------------- the restatements
def test_slab_words_and_member_bits():
    # a slab of two lists: list 0 = source rows 5, 1, 40 (one tile, 3 rows), list 1 = 33 rows (two tiles: 32 + 1)
    ids = np.full(96, -1, dtype=np.int64)
    ids[:3] = [1, 5, 40]
    ids[32:65] = [r for r in range(2, 45) if r not in (5, 40)][:33]
    bits = np.zeros(44, dtype=bool)          # the bitmap ends before source row 44
    bits[[5, 40, 2, 35]] = True
    w = slab_words(ids, bits, [0, 1, 2], [3, 32, 1])
    assert w[0] == 0b110                      # rows 5 and 40 sit at positions 1 and 2
    assert w[1] == 1                          # source row 2 is the first of list 1; 35 is its 33rd row: the next tile
    assert int(ids[64]) == 35 and w[2] == 1
    assert slab_words(ids, bits, [2], [0])[0] == 0                          # no valid row: nothing
    assert slab_words(ids, np.ones(3, dtype=bool), [0], [3])[0] == 0b001    # rows 5 and 40 lie past a 3-row bitmap
    assign = np.array([0, 1, 1, 0, 2, 2, 1, 0], dtype=np.int32)
    assert member_bits(assign, [1, -1], 6, 10).tolist() == [False, True, True, False, False, False, True, True, True, True]
    assert member_bits(assign, [0, 2], 8, 8).tolist() == [True, False, False, True, True, True, False, True]
    assert pack_allow(member_bits(assign, [1], 6, 10)).tolist() == [0b1111000110]


# ---------------------------------------------------------------------------------------------- the ABI
def test_new_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(rass_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in _native.SIGNATURES, name
    # the two searches take the bitmap triple of rass_index_search_allowed and end in the scanned-rows pointer
    host = _native.SIGNATURES["rass_ivf_search_allowed_delta"][1]
    dev = _native.SIGNATURES["rass_ivf_search_allowed_delta_device"][1]
    assert len(host) == len(dev) == 14 and host[-1] is _native.c_i64_p
