"""The host-side layers of the score-threshold search, without a GPU: ``HipIndexer.semantic_search_above`` over a stand-in
index that answers ``search_range`` in numpy, and the argument validation of ``FlatIndex.search_range`` (which refuses
before any native call is made)."""
import types

import numpy as np
import pytest

from rassengine_amd import config, indexer
from rassengine_amd.docstore import REGISTRY, IndexState
from rassengine_amd.engine import FlatIndex

DIM = 16


class StandInIndex:
    """``FlatIndex``'s write path and ``search_range`` in numpy: exact cosine, (score desc, id asc), exact totals."""

    def __init__(self):
        self.x = np.zeros((0, DIM), dtype=np.float32)
        self.tags = np.zeros(0, dtype=np.int32)
        self.layout_epoch = 0
        self.calls = []
        self.compact_during_next = 0     # that many coming searches see the index compacted under them

    rows = property(lambda self: self.x.shape[0])
    count = property(lambda self: int(np.count_nonzero(self.tags != -1)))

    def add(self, vecs, tags=None, normalize=True):
        v = np.asarray(vecs, dtype=np.float32)
        v = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
        first = self.rows
        self.x = np.concatenate([self.x, v.astype(np.float32)])
        self.tags = np.concatenate([self.tags, np.asarray(tags, dtype=np.int32)])
        return first

    def delete(self, row):
        self.tags[row] = -1

    def search_range(self, queries, min_score, max_hits=256, q_filter=None, q_filter_mask=None):
        self.calls.append(dict(min_score=np.array(min_score), max_hits=max_hits, q_filter=q_filter, q_filter_mask=q_filter_mask))
        if self.compact_during_next > 0:
            self.compact_during_next -= 1
            self.layout_epoch += 1
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        nq = q.shape[0]
        out_s = np.full((nq, max_hits), -np.inf, dtype=np.float32)
        out_i = np.full((nq, max_hits), -1, dtype=np.int64)
        total = np.zeros(nq, dtype=np.int64)
        for j in range(nq):
            s = (self.x @ q[j]).astype(np.float32)
            ok = (self.tags != -1) & (s >= np.float32(min_score[j]))
            if q_filter is not None and q_filter[j] >= 0:
                ok &= ((self.tags & q_filter_mask[j]) if q_filter_mask is not None else self.tags) == q_filter[j]
            rows = np.flatnonzero(ok)
            rows = rows[np.lexsort((rows, -s[rows]))]
            total[j] = len(rows)
            m = min(len(rows), max_hits)
            out_s[j, :m], out_i[j, :m] = s[rows[:m]], rows[:m]
        return out_s, out_i, total


@pytest.fixture
def world():
    """An index of 40 chunks of two patients whose cosine to the query e0 is known by construction."""
    name = "range-cpu"
    idx = StandInIndex()
    REGISTRY.put(IndexState(name, idx))
    cos = np.linspace(0.99, 0.02, 40)
    emb = np.zeros((40, DIM), dtype=np.float32)
    emb[:, 0] = cos
    emb[:, 1] = np.sqrt(1.0 - cos ** 2)
    docs = [{"doc_id": f"d{i}", "patientId": "alice" if i % 2 == 0 else "bob", "doc_type": "unstructured", "n": i} for i in range(40)]
    indexer.add_documents(name, docs, emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    yield indexer.HipIndexer(None, name), idx, q, cos
    REGISTRY.drop(name)


@pytest.mark.parametrize("mode", ["opensearch", "cosine"])
def test_score_units_round_trip(mode):
    for cos in (-1.0, -0.25, 0.0, 0.3, 0.8, 0.999, 1.0):
        score = indexer._score_out(cos, mode)
        assert indexer._cos_of_score(score, mode) == pytest.approx(cos, abs=1e-12)
        assert indexer._score_out(indexer._cos_of_score(score, mode), mode) == pytest.approx(score, abs=1e-12)
    assert np.isnan(indexer._cos_of_score(float("nan"), mode))
    assert indexer._cos_of_score(float("-inf"), mode) == float("-inf")
    assert indexer._cos_of_score(0.0, "opensearch") == float("-inf")      # below every OpenSearch score
    assert indexer._cos_of_score(2.0, "opensearch") > 1.0                  # above every one: nothing matches


def test_min_score_is_in_the_units_semantic_search_returns(world, monkeypatch):
    hip, idx, q, cos = world
    for mode in ("opensearch", "cosine"):
        monkeypatch.setattr(config, "RASS_SCORE_MODE", mode)
        bound = indexer._score_out(0.8)
        hits, total = hip.semantic_search_above(q, bound)
        want = [i for i in range(40) if np.float32(cos[i]) >= 0.8 + 1e-6]
        assert total == len(hits) and [d["n"] for d, _ in hits][: len(want)] == want and len(hits) - len(want) <= 1
        assert all(s >= bound - 1e-6 for _, s in hits)
        assert [s for _, s in hits] == sorted((s for _, s in hits), reverse=True)
        # one conversion, to a cosine, handed to the index as float32
        assert idx.calls[-1]["min_score"].dtype == np.float32
        assert float(idx.calls[-1]["min_score"][0]) == pytest.approx(0.8, abs=1e-6)
    with pytest.raises(ValueError):
        hip.semantic_search_above(q, float("nan"))


def test_filters_are_prepared_as_in_knn(world):
    hip, idx, q, cos = world
    hits, total = hip.semantic_search_above(q, indexer._score_out(0.5), patient_id="bob")
    assert total == len(hits) > 0 and all(d["patientId"] == "bob" for d, _ in hits)
    call = idx.calls[-1]
    assert call["q_filter"].dtype == np.int32 and call["q_filter_mask"].dtype == np.int32
    hits2, total2 = hip.semantic_search_above(q, indexer._score_out(0.5), filter_clause={"term": {"patientId": "bob"}})
    assert (hits2, total2) == (hits, total)
    n_calls = len(idx.calls)
    assert hip.semantic_search_above(q, 0.0, patient_id="nobody") == ([], 0)                 # never indexed
    assert hip.semantic_search_above(q, 0.0, patient_id="bob", filter_clause={"term": {"patientId": "alice"}}) == ([], 0)
    assert hip.semantic_search_above(np.zeros(0), 0.0) == ([], 0)
    assert indexer.HipIndexer(None, "no-such-index").semantic_search_above(q, 0.0) == ([], 0)
    assert len(idx.calls) == n_calls                                                          # none of them searched
    # no filter: the index is called without one
    hip.semantic_search_above(q, 0.0)
    assert idx.calls[-1]["q_filter"] is None and idx.calls[-1]["q_filter_mask"] is None


def test_total_passes_through_beyond_the_limit(world):
    hip, idx, q, cos = world
    hits, total = hip.semantic_search_above(q, float("-inf"), limit=5)
    assert total == 40 and [d["n"] for d, _ in hits] == [0, 1, 2, 3, 4]
    assert idx.calls[-1]["max_hits"] == 5
    hits, total = hip.semantic_search_above(q, float("-inf"), limit=5, patient_id="alice")
    assert total == 20 and [d["n"] for d, _ in hits] == [0, 2, 4, 6, 8]
    # a superseded chunk is tombstoned: neither listed nor counted
    indexer.add_documents(hip.index_name, [{"doc_id": "d0", "patientId": "alice", "doc_type": "unstructured", "n": 100}],
                          np.eye(1, DIM, 1, dtype=np.float32))
    hits, total = hip.semantic_search_above(q, float("-inf"), limit=3)
    assert total == 40 and [d["n"] for d, _ in hits] == [1, 2, 3]


def test_layout_epoch_retry(world):
    hip, idx, q, cos = world
    idx.compact_during_next = 2                     # two searches see a compaction land under them, the third is clean
    before = len(idx.calls)
    hits, total = hip.semantic_search_above(q, float("-inf"), limit=4)
    assert len(idx.calls) - before == 3 and total == 40 and len(hits) == 4
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_search_above(q, float("-inf"), limit=4)
    assert len(idx.calls) - before == 3 + indexer.LAYOUT_ATTEMPTS


def test_flat_index_search_range_validates_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def rass_index_search_range(self, *a):
            raise AssertionError("the native entry point was reached with bad arguments")

    idx = FlatIndex(types.SimpleNamespace(_L=Lib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    bad = [
        dict(queries=np.zeros(DIM), min_score=0.5),                                  # queries must be [nq, dim]
        dict(queries=np.zeros((3, DIM + 1)), min_score=0.5),
        dict(queries=q, min_score=np.zeros(2)),                                      # one threshold per query
        dict(queries=q, min_score=np.zeros((3, 1))),
        dict(queries=q, min_score=np.array(["a", "b", "c"])),                        # not numbers
        dict(queries=q, min_score=np.zeros(3, dtype=np.complex64)),
        dict(queries=q, min_score=[0.1, float("nan"), 0.2]),
        dict(queries=q, min_score=0.5, max_hits=0),
        dict(queries=q, min_score=0.5, max_hits=4097),
        dict(queries=q, min_score=0.5, q_filter=np.zeros(2, dtype=np.int32)),
        dict(queries=q, min_score=0.5, q_filter_mask=np.zeros(3, dtype=np.int32)),   # a mask needs a filter
        dict(queries=q, min_score=0.5, q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(4, dtype=np.int32)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_range(**kw)
    # good arguments do reach it: a scalar threshold, float64 thresholds, integer thresholds, both bounds of max_hits
    for kw in (dict(min_score=0.5), dict(min_score=np.zeros(3, dtype=np.float64)), dict(min_score=np.zeros(3, dtype=np.int64)),
               dict(min_score=-np.inf, max_hits=1), dict(min_score=0.5, max_hits=4096)):
        with pytest.raises(AssertionError, match="native entry point"):
            idx.search_range(q, **kw)
