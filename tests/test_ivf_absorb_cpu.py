"""The device-planned IVF build and the absorb above the kernel, without a GPU: the ABI surface and the policy that decides
between retraining and absorbing (``IvfPolicy.action`` / ``IvfBackedIndex.maybe_rebuild``) on a fake IVF that counts the
``train_centroids`` / ``build`` / ``absorb`` calls."""
import ctypes
import os
import re
import subprocess
import threading
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rass_ivf_plan_workspace_bytes", "rass_ivf_plan_lists", "rass_ivf_build_device", "rass_ivf_absorb",
               "rass_ivf_lists_device")


# ------------------------------------------------------------------------------------------------ the ABI surface
def test_header_library_and_binding_carry_the_new_entry_points():
    from rassengine_amd import _native as N
    header = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(rass_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    exported = set(re.findall(r" T (rass_[a-z0-9_]+)", subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], check=True,
                                                                      capture_output=True, text=True).stdout))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in N.SIGNATURES, name
        assert callable(getattr(N.lib(), name))


def test_plan_workspace_is_positive_and_monotone():
    from rassengine_amd import _native as N
    L = N.lib()
    sizes = [L.rass_ivf_plan_workspace_bytes(n, 4096) for n in (0, 1, 31, 4096, 4097, 100_000, 3_000_000, 12_500_000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= 12_500_000 * 6                       # the first pass's keys and rows
    by_lists = [L.rass_ivf_plan_workspace_bytes(100_000, nl) for nl in (1, 7, 256, 257, 4096, 32768)]
    assert all(s > 0 for s in by_lists) and by_lists == sorted(by_lists)
    for n, nl in ((-1, 16), (10, 0), (10, 32769)):           # out of range: no size to give
        assert L.rass_ivf_plan_workspace_bytes(n, nl) == 0


def test_null_handles_are_refused_with_a_message():
    from rassengine_amd import _native as N
    L = N.lib()
    out = ctypes.c_void_p(1)
    assert L.rass_ivf_absorb(None, None, -1, ctypes.byref(out)) == -1 and b"NULL" in L.rass_last_error()   # RASS_ERR_INVALID
    assert L.rass_ivf_absorb(None, None, -1, None) == -1
    assert L.rass_ivf_build_device(None, None, 16, None, 0, -1, ctypes.byref(out)) == -1 and b"NULL" in L.rass_last_error()
    assert L.rass_ivf_lists_device(None, None, 0, None) == -1 and b"NULL" in L.rass_last_error()
    assert L.rass_ivf_plan_lists(None, None, 10, 16, 32, None, None, None, None, 64, None, None, None, 0, None) == -1
    assert b"NULL" in L.rass_last_error()
    # shapes are checked before any pointer is used
    assert L.rass_ivf_plan_lists(None, None, 10, 0, 32, None, None, None, None, 64, None, None, None, 0, None) == -1
    assert b"nlist" in L.rass_last_error()
    assert L.rass_ivf_plan_lists(None, None, 10, 16, 48, None, None, None, None, 64, None, None, None, 0, None) == -1
    assert b"tile_rows" in L.rass_last_error()


def test_config_default_is_never():
    from rassengine_amd import config
    from rassengine_amd.ivf import IvfPolicy
    assert config.RASS_IVF_ABSORB_FRACTION == 0
    assert IvfPolicy().absorb_fraction == 0 and IvfPolicy.manual().absorb_fraction == 0
    assert IvfPolicy.from_config().absorb_fraction == 0


# ------------------------------------------------------------------------------------------------ the policy
class FakeIvf:
    def __init__(self, covered):
        self.covered_rows = covered
        self.closed = False

    def absorb(self, flat, n_rows=-1):
        assert not self.closed and n_rows % 32 == 0 and self.covered_rows < n_rows <= flat.rows
        flat.log.append(("absorb", flat.rows, n_rows))
        return FakeIvf(n_rows)

    def close(self):
        self.closed = True


@pytest.fixture
def backed(monkeypatch):
    """``make(policy)`` -> an ``IvfBackedIndex`` whose flat index is a row counter and whose IVFs are ``FakeIvf``s; every
    train / build / absorb lands in its ``log``."""
    from rassengine_amd import ivf as M

    class CountingIndex(M.IvfBackedIndex):
        def __init__(self, policy):
            self.policy, self.ivf, self.builds, self.trained_rows = policy, None, 0, 0
            self._ivf_lock = threading.RLock()
            self.n, self.log = 0, []

        rows = property(lambda self: self.n)

        def add(self, n):
            self.n += n
            self.maybe_rebuild()
            return self.builds, self.covered

    def train(index, nlist, *a, **kw):
        index.log.append(("train", index.rows))
        return "centroids"

    def build(index, nlist=0, centroids=None, dtype="f32", assign=None, n_rows=-1, **kw):
        assert centroids == "centroids" and n_rows % 32 == 0
        index.log.append(("build", index.rows, n_rows))
        return FakeIvf(n_rows)

    monkeypatch.setattr(M, "train_centroids", train)
    monkeypatch.setattr(M, "assign_rows", lambda index, centroids: np.zeros(index.rows, dtype=np.int32))
    monkeypatch.setattr(M.IvfIndex, "build", staticmethod(build))
    return CountingIndex


def _todays_rule(adds, nlist, min_rows, fraction):
    """The parent commit's ``maybe_rebuild``, restated: train + build over rows // 32 * 32 when the index has no IVF yet or
    its delta exceeds ``fraction`` of the covered rows."""
    rows = covered = builds = 0
    log, seen = [], []
    for n in adds:
        rows += n
        if nlist > 0 and rows >= max(min_rows, nlist) and (covered <= 0 or rows - covered > fraction * covered):
            covered, builds = rows // 32 * 32, builds + 1
            log += [("train", rows), ("build", rows, covered)]
        seen.append((builds, covered))
    return log, seen


def test_without_absorb_fraction_the_call_sequence_is_todays(backed):
    from rassengine_amd.ivf import IvfPolicy
    adds = [400] * 8
    idx = backed(IvfPolicy(nlist=16, min_rows=1500, rebuild_fraction=0.5))
    seen = [idx.add(n) for n in adds]
    # the numbers tests/test_gpu_ivf_delta.py pins for the same script: built at 1 600 rows, rebuilt once the delta > 800
    assert [b for b, _ in seen] == [0, 0, 0, 1, 1, 1, 2, 2] and seen[3][1] == 1600 and seen[6][1] == 2784
    assert idx.log == [("train", 1600), ("build", 1600, 1600), ("train", 2800), ("build", 2800, 2784)]
    for adds, nlist, min_rows, fraction in (([64] * 60, 16, 1000, 0.25), ([700, 1, 1, 3000, 5, 64, 64, 2000], 64, 512, 0.1),
                                            ([100] * 30, 0, 0, 0.25)):
        idx = backed(IvfPolicy(nlist=nlist, min_rows=min_rows, rebuild_fraction=fraction, absorb_fraction=0))
        seen = [idx.add(n) for n in adds]
        want_log, want_seen = _todays_rule(adds, nlist, min_rows, fraction)
        assert idx.log == want_log and seen == want_seen
        assert not any(e[0] == "absorb" for e in idx.log)


def test_absorbs_at_the_five_percent_crossings_without_training(backed):
    from rassengine_amd.ivf import IvfPolicy
    idx = backed(IvfPolicy(nlist=16, min_rows=1024, rebuild_fraction=0.25, absorb_fraction=0.05))
    for _ in range(16):
        idx.add(64)                                            # 1 024 rows: the first build
    assert idx.log == [("train", 1024), ("build", 1024, 1024)] and idx.trained_rows == 1024
    first = idx.ivf
    del idx.log[:]
    seen = [idx.add(64) for _ in range(4)]                     # 1 088 .. 1 280: each 64-row upload is > 5 % of the covered rows
    assert idx.log == [("absorb", r, r) for r in (1088, 1152, 1216, 1280)]
    assert seen == [(2, 1088), (3, 1152), (4, 1216), (5, 1280)] and idx.trained_rows == 1024
    assert first.closed and not idx.ivf.closed                 # swapped through the build's swap: the old one is freed
    # below the crossing nothing happens
    big = backed(IvfPolicy(nlist=16, min_rows=4096, rebuild_fraction=0.25, absorb_fraction=0.05))
    assert big.add(4096) == (1, 4096)
    del big.log[:]
    assert big.add(128) == (1, 4096) and big.log == []         # 3.1 % of the covered rows
    assert big.add(129) == (2, 4352) and big.log == [("absorb", 4353, 4352)]    # 6.3 %: absorbed up to the scan tile
    # fewer than 32 new rows cannot be absorbed, whatever the fraction says
    tiny = backed(IvfPolicy(nlist=16, min_rows=64, rebuild_fraction=10.0, absorb_fraction=0.05))
    assert tiny.add(64) == (1, 64) and tiny.add(8) == (1, 64) and tiny.absorb_delta() is None
    assert tiny.add(24) == (2, 96) and tiny.log[-1] == ("absorb", 96, 96)


def test_retrains_once_the_rows_exceed_the_trained_rows_by_the_rebuild_fraction(backed):
    from rassengine_amd.ivf import IvfPolicy
    idx = backed(IvfPolicy(nlist=16, min_rows=1024, rebuild_fraction=0.25, absorb_fraction=0.05))
    idx.add(1024)
    idx.add(256)                                               # 1 280 = 1.25 x 1 024 exactly: not yet stale
    assert idx.log[2:] == [("absorb", 1280, 1280)] and idx.trained_rows == 1024
    idx.add(1)                                                 # 1 281 > 1.25 x 1 024: the centroids are retrained
    assert idx.log[3:] == [("train", 1281), ("build", 1281, 1280)] and idx.trained_rows == 1280
    # from here the clock runs from 1 280 trained rows: absorbs up to 1 600, the next training past it
    del idx.log[:]
    for _ in range(6):
        idx.add(64)                                            # 1 345 .. 1 665
    assert idx.log == [("absorb", 1345, 1344), ("absorb", 1473, 1472), ("train", 1601), ("build", 1601, 1600)]
    assert idx.trained_rows == 1600
    # dropping the IVF (a compaction does) forgets the training: the next build trains
    idx.drop_ivf()
    assert idx.trained_rows == 0 and idx.ivf is None
    del idx.log[:]
    idx.add(1)
    assert [e[0] for e in idx.log] == ["train", "build"]


def test_a_loaded_ivf_takes_its_covered_rows_as_trained_rows(monkeypatch, tmp_path):
    from rassengine_amd import ivf as M
    path = str(tmp_path / "u.rass")
    open(path + ".ivf", "wb").close()
    lib = types.SimpleNamespace(rass_index_rows=lambda h: 2000)
    engine = types.SimpleNamespace(_L=lib, load_index=lambda name, p: types.SimpleNamespace(engine=engine, name=name, _h=7))
    monkeypatch.setattr(M.IvfIndex, "load", staticmethod(lambda eng, f: FakeIvf(1920)))
    idx = M.IvfBackedIndex.load(engine, "u", path, M.IvfPolicy(nlist=16, min_rows=64, absorb_fraction=0.05))
    assert idx.covered == 1920 and idx.trained_rows == 1920
    assert idx.policy.action(2000, idx.covered, idx.trained_rows) is None          # 80 rows: 4.2 % of 1 920
    assert idx.policy.action(2048, idx.covered, idx.trained_rows) == "absorb"
    assert idx.policy.action(2401, idx.covered, idx.trained_rows) == "train"       # > 1.25 x 1 920
    assert idx.policy.action(2401, 2368, idx.trained_rows) == "train"              # ... however much was absorbed meanwhile
    # an IVF that does not fit the index is not adopted, and nothing counts as trained
    monkeypatch.setattr(M.IvfIndex, "load", staticmethod(lambda eng, f: FakeIvf(4000)))
    idx = M.IvfBackedIndex.load(engine, "u", path, M.IvfPolicy(nlist=16, min_rows=64, absorb_fraction=0.05))
    assert idx.ivf is None and idx.trained_rows == 0


# ------------------------------------------------------------------------------------------------ training over rows that are not finite
def test_a_centroid_that_is_not_finite_is_replaced_not_kept():
    """``_finite_rows`` (include/rass_engine.h, "Scores that are not finite"): a new centroid holding a NaN or an Inf — a
    seed or a re-seed drawn from such an index row — gives way to the same row of the old set where that one is finite, to a
    zero row otherwise; finite rows pass through bit for bit, and a set without such a row is returned as it is."""
    import torch
    from rassengine_amd.ivf import _finite_rows
    g = torch.Generator().manual_seed(1)
    new = torch.randn((6, 8), generator=g)
    old = torch.randn((6, 8), generator=g)
    assert _finite_rows(new, old) is new and _finite_rows(new, None) is new
    bad = new.clone()
    bad[1, 3] = float("nan")
    bad[2, 0] = float("inf")
    bad[4] = float("nan")
    bad[5, 7] = float("-inf")
    prev = old.clone()
    prev[2, 5] = float("nan")                                  # the old row 2 is no better: zeros
    out = _finite_rows(bad, prev)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[0], new[0]) and torch.equal(out[3], new[3])
    assert torch.equal(out[1], old[1]) and torch.equal(out[4], old[4]) and torch.equal(out[5], old[5])
    assert torch.equal(out[2], torch.zeros(8))
    seeds = _finite_rows(bad, None)                            # the seeds have no older set
    assert bool(torch.isfinite(seeds).all()) and torch.equal(seeds[0], new[0])
    for r in (1, 2, 4, 5):
        assert torch.equal(seeds[r], torch.zeros(8))
