"""The host-side layers of the semantic terms aggregation, without a GPU: ``HipIndexer.semantic_aggregate`` over a stand-in
index that answers ``search_counts`` in numpy, and the argument validation of ``FlatIndex.search_counts`` (which refuses
before any native call is made)."""
import types

import numpy as np
import pytest

from rassengine_amd import config, indexer
from rassengine_amd.docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_PATIENT_MASK, IndexState
from rassengine_amd.engine import FlatIndex

DIM = 16
EMPTY = {"buckets": [], "sum_other_doc_count": 0, "cardinality": 0, "total": 0}


class PlainIndex:
    """``FlatIndex``'s write path in numpy and nothing else: an index object WITHOUT ``search_counts``."""

    def __init__(self):
        self.x = np.zeros((0, DIM), dtype=np.float32)
        self.tags = np.zeros(0, dtype=np.int32)
        self.layout_epoch = 0

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


class StandInIndex(PlainIndex):
    """... plus ``search_counts`` in numpy: exact cosine, the hits counted per group, the buckets under (count desc, group
    asc), each with its best row under (score desc, row asc), exact figures."""

    def __init__(self):
        super().__init__()
        self.calls = []
        self.compact_during_next = 0     # that many coming searches see the index compacted under them
        self.after_search = None         # called at the end of a search: a concurrent ingest

    def search_counts(self, queries, min_score, size, group_mask, n_groups, q_filter=None, q_filter_mask=None):
        self.calls.append(dict(min_score=np.array(min_score), size=size, group_mask=group_mask, n_groups=n_groups,
                               q_filter=q_filter, q_filter_mask=q_filter_mask))
        if self.compact_during_next > 0:
            self.compact_during_next -= 1
            self.layout_epoch += 1
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        nq = q.shape[0]
        thr = np.broadcast_to(np.asarray(min_score, dtype=np.float32), (nq,))
        shift = (group_mask & -group_mask).bit_length() - 1
        keys = (self.tags.astype(np.int64) & group_mask) >> shift
        out_g = np.full((nq, size), -1, dtype=np.int32)
        out_c = np.zeros((nq, size), dtype=np.int64)
        out_s = np.full((nq, size), -np.inf, dtype=np.float32)
        out_i = np.full((nq, size), -1, dtype=np.int64)
        n_buckets = np.zeros(nq, dtype=np.int64)
        total = np.zeros(nq, dtype=np.int64)
        for j in range(nq):
            s = (self.x @ q[j]).astype(np.float32)
            ok = (self.tags != -1) & (s >= thr[j])
            if q_filter is not None and q_filter[j] >= 0:
                ok &= ((self.tags & q_filter_mask[j]) if q_filter_mask is not None else self.tags) == q_filter[j]
            assert not np.any(ok & (keys >= n_groups)), "a hit's group key is >= n_groups"
            rows = np.flatnonzero(ok)
            total[j] = len(rows)
            buckets = sorted(set(keys[rows].tolist()), key=lambda g: (-int(np.count_nonzero(keys[rows] == g)), g))
            n_buckets[j] = len(buckets)
            for at, g in enumerate(buckets[:size]):
                mine = rows[keys[rows] == g]
                best = mine[np.lexsort((mine, -s[mine]))][0]
                out_g[j, at], out_c[j, at], out_s[j, at], out_i[j, at] = g, len(mine), s[best], best
        if self.after_search is not None:
            self.after_search()
        return out_g, out_c, out_s, out_i, n_buckets, total


def _fill(name, idx):
    """40 chunks whose cosine to the query e0 is known by construction and falls with n.  alice: n % 4 == 0 (10 chunks), bob:
    the odd n (20), carol: n % 4 == 2 (10).  Every fourth chunk, n % 4 == 3, is a 'note' (bob's), the rest 'unstructured'."""
    REGISTRY.put(IndexState(name, idx))
    cos = np.linspace(0.99, 0.02, 40)
    emb = np.zeros((40, DIM), dtype=np.float32)
    emb[:, 0] = cos
    emb[:, 1] = np.sqrt(1.0 - cos ** 2)
    who = {0: "alice", 1: "bob", 2: "carol", 3: "bob"}
    docs = [{"doc_id": f"d{i}", "patientId": who[i % 4], "doc_type": "note" if i % 4 == 3 else "unstructured", "n": i}
            for i in range(40)]
    indexer.add_documents(name, docs, emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    return q, cos


def _score(cos_value):
    """A min_score, in semantic_search's units, just below the score of a chunk with this cosine."""
    return indexer._score_out(float(np.float32(cos_value))) - 1e-4


@pytest.fixture
def world():
    name = "agg-cpu"
    idx = StandInIndex()
    q, cos = _fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, cos
    REGISTRY.drop(name)


def _shape(agg):
    return [(b["key"], b["doc_count"], b["top_hit"][0]["n"]) for b in agg["buckets"]]


def test_buckets_by_patient(world):
    hip, idx, q, cos = world
    agg = hip.semantic_aggregate(q, min_score=0.0)                      # at or below 0: every chunk
    assert _shape(agg) == [("bob", 20, 1), ("alice", 10, 0), ("carol", 10, 2)]      # a tie in doc_count: first-indexed first
    assert agg["sum_other_doc_count"] == 0 and agg["cardinality"] == 3 and agg["total"] == 40
    assert set(agg) == {"buckets", "sum_other_doc_count", "cardinality", "total"}
    call = idx.calls[-1]
    assert call["group_mask"] == TAG_PATIENT_MASK and call["n_groups"] == 4 and call["size"] == 5   # codes 1..3 and 0 = none
    assert call["q_filter"] is None and call["q_filter_mask"] is None and np.isneginf(call["min_score"][0])
    for b in agg["buckets"]:
        assert isinstance(b["doc_count"], int) and isinstance(b["top_hit"][1], float) and b["top_hit"][0]["patientId"] == b["key"]
    # the chunks n <= 9 only: alice 0 4 8, bob 1 3 5 7 9, carol 2 6
    agg = hip.semantic_aggregate(q, min_score=_score(cos[9]))
    assert _shape(agg) == [("bob", 5, 1), ("alice", 3, 0), ("carol", 2, 2)] and agg["total"] == 10 and agg["cardinality"] == 3
    # size below the number of buckets: the rest is summed, the cardinality and the total still say all
    agg = hip.semantic_aggregate(q, min_score=_score(cos[9]), size=1)
    assert _shape(agg) == [("bob", 5, 1)]
    assert agg["sum_other_doc_count"] == 5 and agg["cardinality"] == 3 and agg["total"] == 10
    # above every chunk: the empty aggregation, from a search that found nothing
    n_calls = len(idx.calls)
    assert hip.semantic_aggregate(q, min_score=_score(1.0) + 0.01) == EMPTY and len(idx.calls) == n_calls + 1


def test_code_zero_becomes_none(world):
    hip, idx, q, cos = world
    indexer.add_documents(hip.index_name, [{"doc_id": "anon", "doc_type": "unstructured", "n": 200}],
                          np.eye(1, DIM, 0, dtype=np.float32))
    agg = hip.semantic_aggregate(q, min_score=_score(cos[1]))
    assert _shape(agg) == [(None, 1, 200), ("alice", 1, 0), ("bob", 1, 1)] and agg["cardinality"] == 3 and agg["total"] == 3
    # a superseded chunk is tombstoned: alice's count drops and her bucket goes
    indexer.add_documents(hip.index_name, [{"doc_id": "d0", "patientId": "alice", "doc_type": "unstructured", "n": 100}],
                          np.eye(1, DIM, 1, dtype=np.float32))
    agg = hip.semantic_aggregate(q, min_score=_score(cos[1]))
    assert _shape(agg) == [(None, 1, 200), ("bob", 1, 1)] and agg["cardinality"] == 2 and agg["total"] == 2


def test_buckets_by_doc_type(world):
    hip, idx, q, cos = world
    agg = hip.semantic_aggregate(q, min_score=0.0, by="doc_type")
    assert _shape(agg) == [("unstructured", 30, 0), ("note", 10, 3)] and agg["cardinality"] == 2 and agg["total"] == 40
    call = idx.calls[-1]
    assert call["group_mask"] == TAG_DOCTYPE_MASK and call["n_groups"] == 3
    for bad in ("patient", "", None, "doc_id", "conditionCodeText"):
        with pytest.raises(ValueError, match="by must be"):
            hip.semantic_aggregate(q, min_score=0.0, by=bad)


def test_filters_are_prepared_as_in_knn(world):
    hip, idx, q, cos = world
    agg = hip.semantic_aggregate(q, min_score=0.0, by="doc_type", patient_id="bob")
    assert _shape(agg) == [("unstructured", 10, 1), ("note", 10, 3)] and agg["total"] == 20    # a tie: first-indexed first
    call = idx.calls[-1]
    assert call["q_filter"].dtype == np.int32 and call["q_filter_mask"].dtype == np.int32
    assert int(call["q_filter_mask"][0]) == TAG_PATIENT_MASK
    assert hip.semantic_aggregate(q, min_score=0.0, by="doc_type", filter_clause={"term": {"patientId": "bob"}}) == agg
    agg = hip.semantic_aggregate(q, min_score=0.0, filter_clause={"term": {"doc_type": "note"}})
    assert _shape(agg) == [("bob", 10, 3)] and agg["cardinality"] == 1
    n_calls = len(idx.calls)
    assert hip.semantic_aggregate(q, 0.0, patient_id="nobody") == EMPTY                       # never indexed
    assert hip.semantic_aggregate(q, 0.0, patient_id="bob", filter_clause={"term": {"patientId": "alice"}}) == EMPTY
    assert hip.semantic_aggregate(np.zeros(0), 0.0) == EMPTY
    assert hip.semantic_aggregate(None, 0.0) == EMPTY
    assert indexer.HipIndexer(None, "no-such-index").semantic_aggregate(q, 0.0) == EMPTY
    assert len(idx.calls) == n_calls                                                          # none of them searched


@pytest.mark.parametrize("mode", ["opensearch", "cosine"])
def test_min_score_and_scores_are_in_the_units_semantic_search_returns(world, monkeypatch, mode):
    hip, idx, q, cos = world
    monkeypatch.setattr(config, "RASS_SCORE_MODE", mode)
    bound = indexer._score_out(0.5)
    agg = hip.semantic_aggregate(q, min_score=bound)
    assert float(idx.calls[-1]["min_score"][0]) == pytest.approx(0.5, abs=1e-6)               # converted once, to a cosine
    assert idx.calls[-1]["min_score"].dtype == np.float32 and idx.calls[-1]["min_score"].shape == (1,)
    assert agg["total"] == int(np.count_nonzero(cos.astype(np.float32) >= 0.5 + 1e-6)) and agg["cardinality"] == 3
    for b, c in zip(agg["buckets"], (cos[1], cos[0], cos[2])):
        assert b["top_hit"][1] == pytest.approx(indexer._score_out(float(np.float32(c))), abs=1e-6)
    with pytest.raises(ValueError, match="NaN"):
        hip.semantic_aggregate(q, min_score=float("nan"))


def test_n_groups_is_read_per_attempt(world):
    hip, idx, q, cos = world

    def ingest():        # a new patient arrives while the first attempt, which a compaction voids, is under way
        idx.after_search = None
        indexer.add_documents(hip.index_name, [{"doc_id": "new", "patientId": "dave", "doc_type": "unstructured", "n": 300}],
                              np.eye(1, DIM, 0, dtype=np.float32))

    idx.compact_during_next = 1
    idx.after_search = ingest
    agg = hip.semantic_aggregate(q, min_score=_score(cos[0]))
    assert [c["n_groups"] for c in idx.calls[-2:]] == [4, 5]            # the second attempt saw dave's code
    assert _shape(agg) == [("alice", 1, 0), ("dave", 1, 300)]


def test_layout_epoch_retry(world):
    hip, idx, q, cos = world
    idx.compact_during_next = 2                     # two searches see a compaction land under them, the third is clean
    before = len(idx.calls)
    agg = hip.semantic_aggregate(q, min_score=0.0, size=4)
    assert len(idx.calls) - before == 3 and agg["total"] == 40 and len(agg["buckets"]) == 3
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_aggregate(q, min_score=0.0, size=4)
    assert len(idx.calls) - before == 3 + indexer.LAYOUT_ATTEMPTS


def test_an_index_without_the_method_says_so():
    name = "agg-cpu-plain"
    q, _ = _fill(name, PlainIndex())
    try:
        with pytest.raises(NotImplementedError, match="PlainIndex has no aggregation"):
            indexer.HipIndexer(None, name).semantic_aggregate(q, 0.0)
        assert indexer.HipIndexer(None, name).semantic_aggregate(np.zeros(0), 0.0) == EMPTY
    finally:
        REGISTRY.drop(name)


def test_aggregate_search_is_still_the_delegated_original():
    class Original:
        def __init__(self, client, index_name):
            self.index_name = index_name

        def aggregate_search(self, query, filter_clause=None, patient_id=None):
            return {"from": "the text engine", "index": self.index_name}

    cls = indexer.make_indexer_class(Original)
    assert "aggregate_search" not in vars(indexer.HipIndexer) and "aggregate_search" not in vars(cls)
    assert "semantic_aggregate" in vars(indexer.HipIndexer)
    assert cls(None, "x").aggregate_search("How many patients have hypertension?") == {"from": "the text engine", "index": "x"}
    with pytest.raises(AttributeError, match="aggregate_search"):
        indexer.HipIndexer(None, "x").aggregate_search        # no original kept: the text builders are not re-implemented


def test_flat_index_search_counts_validates_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def rass_index_aggregate(self, *a):
            raise AssertionError("the native entry point was reached with bad arguments")

        def rass_index_aggregate_device(self, *a):
            raise AssertionError("the native entry point was reached with bad arguments")

    idx = FlatIndex(types.SimpleNamespace(_L=Lib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, min_score=0.5, size=5, group_mask=TAG_PATIENT_MASK, n_groups=10)
    bad = [
        dict(queries=np.zeros(DIM)),                                                  # queries must be [nq, dim]
        dict(queries=np.zeros((3, DIM + 1))),
        dict(min_score=float("nan")), dict(min_score=np.array([0.1, np.nan, 0.3])), dict(min_score=np.zeros(2)),
        dict(min_score=np.zeros((3, 1))), dict(min_score="0.5"), dict(min_score=None),
        dict(size=0), dict(size=4097), dict(size=-3),
        dict(group_mask=0), dict(group_mask=-1), dict(group_mask=0x80000000), dict(group_mask=1 << 32),
        dict(n_groups=0), dict(n_groups=-1), dict(n_groups=(1 << 20) + 1),
        dict(q_filter=np.zeros(2, dtype=np.int32)),
        dict(q_filter_mask=np.zeros(3, dtype=np.int32)),                              # a mask needs a filter
        dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(4, dtype=np.int32)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_counts(**dict(good, **kw))
    for kw in (dict(size=0), dict(size=4097), dict(group_mask=0), dict(group_mask=0x80000000), dict(n_groups=0),
               dict(n_groups=(1 << 20) + 1)):
        a = dict(dict(size=5, group_mask=TAG_PATIENT_MASK, n_groups=10), **kw)
        with pytest.raises(ValueError):
            idx.search_counts_device(0, 3, 0, a["size"], a["group_mask"], a["n_groups"], 0, 0, 0, 0, 0, 0, 0)
    # good arguments do reach it: both bounds of size, of n_groups and of the mask, the doc_type mask, -inf, a threshold per
    # query, a filter with its mask
    for kw in (dict(), dict(size=1), dict(size=4096), dict(n_groups=1), dict(n_groups=1 << 20), dict(group_mask=1),
               dict(group_mask=0x7FFFFFFF), dict(group_mask=TAG_DOCTYPE_MASK), dict(min_score=-np.inf), dict(min_score=2),
               dict(min_score=np.array([0.1, 0.2, 0.3])),
               dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(3, dtype=np.int32))):
        with pytest.raises(AssertionError, match="native entry point"):
            idx.search_counts(**dict(good, **kw))
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_counts_device(0, 3, 0, 5, TAG_PATIENT_MASK, 10, 0, 0, 0, 0, 0, 0, 0)
