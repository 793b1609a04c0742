"""The host-side layers of the diversified (MMR) search, without a GPU: the numpy reference of the selection rule
(``tests/mmr_ref.py``) against hand-worked cases, the argument validation of ``FlatIndex.search_mmr`` / ``rows_gram`` (which
refuse before any native call is made), ``HipIndexer.semantic_search_diverse`` over a stand-in index that answers
``search_mmr`` through the reference, and the new entry points' presence in the header, the binding table and the built
library."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from rassengine_amd import _native, config, indexer
from rassengine_amd.docstore import REGISTRY, TAG_PATIENT_MASK, IndexState
from rassengine_amd.engine import FlatIndex
from tests import mmr_ref as R

DIM = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("rass_index_rows_gram", "rass_index_rows_gram_device", "rass_index_search_mmr", "rass_index_search_mmr_device")
NEG_INF = np.float32(-np.inf)


# ---------------------------------------------------------------------------------------------- the reference, by hand
def test_lambda_one_is_the_identity():
    rng = np.random.default_rng(1)
    s = np.sort(rng.random(20).astype(np.float32))[::-1]
    G = rng.random((20, 20)).astype(np.float32)
    assert R.select_f32(s, G, 1.0, 7).tolist() == list(range(7))
    assert R.select_f32(s, G, 1.0, 20).tolist() == list(range(20))


def test_all_tie_gives_rank_order():
    s = np.full(6, 0.5, dtype=np.float32)
    G = np.full((6, 6), 0.25, dtype=np.float32)
    for lam in (0.0, 0.3, 0.5, 1.0):
        assert R.select_f32(s, G, lam, 6).tolist() == [0, 1, 2, 3, 4, 5]


def test_hand_worked_duplicates_are_passed_over():
    # ranks 0 and 1 are the same vector (G = 1), rank 2 is different: at lambda = 0.5 the objective of rank 1 after picking 0
    # is 0.5 * 0.9 - 0.5 * 1.0 = -0.05, of rank 2 it is 0.5 * 0.8 - 0.5 * 0.1 = 0.35
    s = np.array([0.9, 0.9, 0.8], dtype=np.float32)
    G = np.array([[1.0, 1.0, 0.1], [1.0, 1.0, 0.1], [0.1, 0.1, 1.0]], dtype=np.float32)
    assert R.select_f32(s, G, 0.5, 3).tolist() == [0, 2, 1]
    assert R.select_f32(s, G, 1.0, 3).tolist() == [0, 1, 2]
    assert R.select_f32(s, G, 0.5, 2).tolist() == [0, 2]


def test_negative_similarity_is_not_clipped():
    # after picking 0: rank 1 has G = 0 (objective 0.5 * 0.5 - 0 = 0.25), rank 2 has G = -0.8 (0.5 * 0.3 + 0.4 = 0.55).
    # Clipped at zero rank 2 would score 0.15 and lose.
    s = np.array([0.9, 0.5, 0.3], dtype=np.float32)
    G = np.array([[1.0, 0.0, -0.8], [0.0, 1.0, 0.0], [-0.8, 0.0, 1.0]], dtype=np.float32)
    assert R.select_f32(s, G, 0.5, 2).tolist() == [0, 2]
    # the penalty is the MAXIMUM over the picked: after 0 and 2, rank 1 has max(0, 0) = 0
    assert R.select_f32(s, G, 0.5, 3).tolist() == [0, 2, 1]


def test_short_candidate_lists_pad():
    s = np.array([0.9, 0.5, -np.inf, -np.inf], dtype=np.float32)
    G = np.zeros((4, 4), dtype=np.float32)
    assert R.select_f32(s, G, 0.5, 4).tolist() == [0, 1]           # c = 2 < k: two picks
    assert R.select_f32(np.full(4, -np.inf, dtype=np.float32), G, 0.5, 4).tolist() == []


def test_the_objective_is_rounded_step_by_step():
    # near-ties one ulp apart: the second pick follows the objectives as three separately rounded fp32 operations, restated
    # here by hand (equal objectives go to the lower rank)
    lam = np.float32(0.3)
    s = np.array([0.7000001, 0.7, 0.6999999], dtype=np.float32)
    G = np.zeros((3, 3), dtype=np.float32)
    G[0, 1] = G[1, 0] = np.float32(1e-8)
    got = R.select_f32(s, G, lam, 3)
    m = np.float32(np.float32(1.0) - lam)
    o1 = np.float32(np.float32(lam * s[1]) - np.float32(m * G[0, 1]))
    o2 = np.float32(np.float32(lam * s[2]) - np.float32(m * G[0, 2]))
    assert got[0] == 0 and got[1] == (1 if o1 >= o2 else 2)


def test_f64_rule_agrees_on_a_well_separated_case():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((12, 8))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rows[:3].sum(axis=0)
    q /= np.linalg.norm(q)
    order = np.argsort(-(rows @ q))
    rows = rows[order]
    want = R.mmr_f64(q, rows, 0.5, 6)
    got = R.select_f32((rows @ q).astype(np.float32), R.gram_f64(rows).astype(np.float32), 0.5, 6)
    assert got.tolist() == want.tolist() and len(set(got.tolist())) == 6


# ---------------------------------------------------------------------------------------------- FlatIndex validation
class RefusingLib:
    def rass_index_dim(self, h):
        return DIM

    def rass_index_search_mmr(self, *a):
        raise AssertionError("the native entry point was reached")

    def rass_index_rows_gram(self, *a):
        raise AssertionError("the native entry point was reached")


def test_flat_index_search_mmr_validates_before_the_native_call():
    idx = FlatIndex(types.SimpleNamespace(_L=RefusingLib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, k=5, fetch_k=20, lambda_mult=0.5)
    bad = [dict(queries=np.zeros(DIM)), dict(queries=np.zeros((3, DIM + 1))), dict(k=0), dict(k=-1), dict(k=21), dict(fetch_k=129),
           dict(fetch_k=0), dict(k=129, fetch_k=None), dict(lambda_mult=float("nan")), dict(lambda_mult=-0.01), dict(lambda_mult=1.5),
           dict(lambda_mult=np.array([0.5, 0.5])), dict(lambda_mult=np.array([0.5, np.nan, 0.5])), dict(lambda_mult="half"),
           dict(lambda_mult=np.zeros((3, 1))), dict(q_filter=np.zeros(2, dtype=np.int32)), dict(q_filter_mask=np.zeros(3, dtype=np.int32)),
           dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(4, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_mmr(**dict(good, **kw))
    for kw in (dict(), dict(k=1, fetch_k=1), dict(k=128, fetch_k=128), dict(fetch_k=None), dict(k=100, fetch_k=None), dict(lambda_mult=0),
               dict(lambda_mult=1), dict(lambda_mult=np.array([0.0, 0.5, 1.0])),
               dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(3, dtype=np.int32))):
        with pytest.raises(AssertionError, match="native entry point"):
            idx.search_mmr(**dict(good, **kw))
    s, i, r = idx.search_mmr(np.zeros((0, DIM), dtype=np.float32), 5)                                     # no query, no call
    assert s.shape == (0, 5) and i.shape == (0, 5) and r.shape == (0, 5) and r.dtype == np.int32


def test_default_fetch_k():
    assert FlatIndex._check_mmr(3, None) == (3, 16)
    assert FlatIndex._check_mmr(10, None) == (10, 40)
    assert FlatIndex._check_mmr(32, None) == (32, 128)
    assert FlatIndex._check_mmr(100, None) == (100, 128)


def test_flat_index_rows_gram_validates_before_the_native_call():
    idx = FlatIndex(types.SimpleNamespace(_L=RefusingLib()), "v", None)
    for rows in (np.zeros((2, 129), dtype=np.int64), np.zeros((2, 0), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64)):
        with pytest.raises(ValueError):
            idx.rows_gram(rows)
    for rows in (np.zeros(5, dtype=np.int64), np.zeros((3, 128), dtype=np.int64), [[1, 2], [3, 4]]):
        with pytest.raises(AssertionError, match="native entry point"):
            idx.rows_gram(rows)
    assert idx.rows_gram(np.zeros((0, 4), dtype=np.int64)).shape == (0, 4, 4)


# ---------------------------------------------------------------------------------------------- the stand-in index
class StandInIndex:
    """``FlatIndex``'s write path, ``search`` and ``search_mmr`` in numpy; the selection is ``mmr_ref.select_f32``."""

    def __init__(self):
        self.x = np.zeros((0, DIM), dtype=np.float32)
        self.tags = np.zeros(0, dtype=np.int32)
        self.layout_epoch = 0
        self.calls = []
        self.compact_during_next = 0     # that many coming searches see the index compacted under them

    rows = property(lambda self: self.x.shape[0])

    def add(self, vecs, tags=None, normalize=True):
        v = np.asarray(vecs, dtype=np.float32)
        v = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
        first = self.rows
        self.x = np.concatenate([self.x, v.astype(np.float32)])
        self.tags = np.concatenate([self.tags, np.asarray(tags, dtype=np.int32)])
        return first

    def delete(self, row):
        self.tags[row] = -1

    def search(self, queries, k, q_filter=None, q_filter_mask=None):
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        out_s = np.full((q.shape[0], k), -np.inf, dtype=np.float32)
        out_i = np.full((q.shape[0], k), -1, dtype=np.int64)
        for j in range(q.shape[0]):
            s = (self.x @ q[j]).astype(np.float32)
            ok = self.tags != -1
            if q_filter is not None and q_filter[j] >= 0:
                ok &= ((self.tags & q_filter_mask[j]) if q_filter_mask is not None else self.tags) == q_filter[j]
            rows = np.flatnonzero(ok)
            rows = rows[np.lexsort((rows, -s[rows]))][:k]
            out_s[j, :len(rows)], out_i[j, :len(rows)] = s[rows], rows
        return out_s, out_i

    def search_mmr(self, queries, k, fetch_k=None, lambda_mult=0.5, q_filter=None, q_filter_mask=None):
        k, fetch_k = FlatIndex._check_mmr(k, fetch_k)
        self.calls.append(dict(k=k, fetch_k=fetch_k, lam=lambda_mult, q_filter=q_filter, q_filter_mask=q_filter_mask))
        if self.compact_during_next > 0:
            self.compact_during_next -= 1
            self.layout_epoch += 1
        cs, ci = self.search(queries, fetch_k, q_filter, q_filter_mask)
        nq = cs.shape[0]
        out_s = np.full((nq, k), -np.inf, dtype=np.float32)
        out_i = np.full((nq, k), -1, dtype=np.int64)
        out_r = np.full((nq, k), -1, dtype=np.int32)
        for j in range(nq):
            rows = np.where(ci[j] >= 0, ci[j], 0)
            G = (self.x[rows] @ self.x[rows].T).astype(np.float32)
            p = R.select_f32(cs[j], G, lambda_mult, k)
            out_s[j, :len(p)], out_i[j, :len(p)], out_r[j, :len(p)] = cs[j, p], ci[j, p], p
        return out_s, out_i, out_r


def _fill(name, idx):
    """20 distinct directions, each indexed twice (chunks n and n + 100 carry the same vector), of four patients by n % 4;
    the cosine to the query e0 falls with n."""
    REGISTRY.put(IndexState(name, idx))
    cos = np.linspace(0.95, 0.10, 20)
    emb = np.zeros((40, DIM), dtype=np.float32)
    docs = []
    for n in range(20):
        for copy in range(2):
            r = 2 * n + copy
            emb[r, 0] = cos[n]
            emb[r, 1 + n % (DIM - 1)] = np.sqrt(1.0 - cos[n] ** 2) * (1.0 if n < DIM - 1 else -1.0)
            docs.append({"doc_id": f"d{n}-{copy}", "patientId": f"p{n % 4}", "doc_type": "note", "n": n + 100 * copy, "text": f"t{n}"})
    indexer.add_documents(name, docs, emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    return q, cos


@pytest.fixture
def world():
    name = "mmr-cpu"
    idx = StandInIndex()
    q, cos = _fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, cos
    REGISTRY.drop(name)


def ns(hits):
    return [d["n"] for d, _ in hits]


def test_diverse_skips_the_duplicates_plain_search_returns(world):
    hip, idx, q, cos = world
    assert ns(hip.semantic_search(q, k=4)) == [0, 100, 1, 101]
    hits = hip.semantic_search_diverse(q, k=4, lambda_mult=0.5)
    assert len({d["text"] for d, _ in hits}) == 4 and ns(hits)[0] == 0
    assert idx.calls[-1]["k"] == 4 and idx.calls[-1]["fetch_k"] == 16 and idx.calls[-1]["q_filter"] is None
    # lambda = 1 is semantic_search
    assert ns(hip.semantic_search_diverse(q, k=4, lambda_mult=1.0)) == [0, 100, 1, 101]
    assert hip.semantic_search_diverse(q, k=5, fetch_k=7)[0][0]["n"] == 0 and idx.calls[-1]["fetch_k"] == 7


def test_diverse_filters_as_semantic_search(world):
    hip, idx, q, cos = world
    hits = hip.semantic_search_diverse(q, k=3, patient_id="p1")
    assert all(d["patientId"] == "p1" for d, _ in hits) and len({d["text"] for d, _ in hits}) == 3
    call = idx.calls[-1]
    assert int(call["q_filter_mask"][0]) == TAG_PATIENT_MASK and call["q_filter"].shape == (1,)
    hits = hip.semantic_search_diverse(q, k=3, filter_clause={"term": {"patientId": "p2"}})
    assert all(d["patientId"] == "p2" for d, _ in hits) and len(hits) == 3
    # only 10 chunks of p3: k = 16 returns all ten of them, picked once each
    hits = hip.semantic_search_diverse(q, k=16, patient_id="p3")
    assert sorted(ns(hits)) == sorted([n + c for n in range(3, 20, 4) for c in (0, 100)])


@pytest.mark.parametrize("mode", ["opensearch", "cosine"])
def test_scores_are_in_the_units_semantic_search_returns(world, monkeypatch, mode):
    hip, idx, q, cos = world
    monkeypatch.setattr(config, "RASS_SCORE_MODE", mode)
    plain = {d["n"]: s for d, s in hip.semantic_search(q, k=40)}
    hits = hip.semantic_search_diverse(q, k=6)
    assert len(hits) == 6
    for d, score in hits:
        assert isinstance(score, float) and score == pytest.approx(plain[d["n"]], abs=1e-6)
        assert score == pytest.approx(indexer._score_out(float(np.float32(cos[d["n"] % 100]))), abs=1e-5)


def test_empty_cases(world):
    hip, idx, q, cos = world
    n_calls = len(idx.calls)
    assert hip.semantic_search_diverse(np.zeros(0)) == []
    assert hip.semantic_search_diverse(None) == []
    assert hip.semantic_search_diverse(q, patient_id="nobody") == []
    assert hip.semantic_search_diverse(q, patient_id="p1", filter_clause={"term": {"patientId": "p2"}}) == []
    assert indexer.HipIndexer(None, "no-such-index").semantic_search_diverse(q) == []
    assert len(idx.calls) == n_calls                                                  # none of them searched
    with pytest.raises(ValueError):
        hip.semantic_search_diverse(q, k=5, fetch_k=4)                                # errors raise
    with pytest.raises(ValueError):
        hip.semantic_search_diverse(q, k=5, fetch_k=200)


def test_layout_epoch_retry(world):
    hip, idx, q, cos = world
    idx.compact_during_next = 2                     # two searches see a compaction land under them, the third is clean
    n0 = len(idx.calls)
    assert len(hip.semantic_search_diverse(q, k=3)) == 3
    assert len(idx.calls) - n0 == 3
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_search_diverse(q, k=3)
    assert len(idx.calls) - n0 == 3 + indexer.LAYOUT_ATTEMPTS


def test_an_index_without_the_method_says_so():
    class PlainIndex(StandInIndex):
        search_mmr = property()          # hasattr() is False

    name = "mmr-cpu-plain"
    q, _ = _fill(name, PlainIndex())
    try:
        with pytest.raises(NotImplementedError, match="diversified"):
            indexer.HipIndexer(None, name).semantic_search_diverse(q, k=3)
        assert len(indexer.HipIndexer(None, name).semantic_search(q, k=3)) == 3      # the plain search is untouched
    finally:
        REGISTRY.drop(name)


# ---------------------------------------------------------------------------------------------- header / table / library
def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    assert re.search(r"#define\s+RASS_MAX_MMR_FETCH\s+128\b", header) and _native.RASS_MAX_MMR_FETCH == 128
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in _native.SIGNATURES, f"{name} is not in the binding table"
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), f"{name}: header and binding table disagree"
    assert os.path.exists(_native.LIB_PATH), "librass_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [name for name in NEW_ENTRY_POINTS if name not in exported]
    assert not missing, f"not exported by the built library: {missing}"
