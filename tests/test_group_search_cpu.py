"""The host-side layers of the grouped (collapsed) search, without a GPU: ``HipIndexer.semantic_search_collapsed`` over a
stand-in index that answers ``search_grouped`` in numpy, and the argument validation of ``FlatIndex.search_grouped`` (which
refuses before any native call is made)."""
import types

import numpy as np
import pytest

from rassengine_amd import config, indexer
from rassengine_amd.docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_PATIENT_MASK, IndexState
from rassengine_amd.engine import FlatIndex

DIM = 16


class PlainIndex:
    """``FlatIndex``'s write path in numpy and nothing else: an index object WITHOUT ``search_grouped``."""

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
    """... plus ``search_grouped`` in numpy: exact cosine, the best row per group under (score desc, row asc), the groups
    in that order, exact totals."""

    def __init__(self):
        super().__init__()
        self.calls = []
        self.compact_during_next = 0     # that many coming searches see the index compacted under them

    def search_grouped(self, queries, k, group_mask, n_groups, q_filter=None, q_filter_mask=None):
        self.calls.append(dict(k=k, group_mask=group_mask, n_groups=n_groups, q_filter=q_filter, q_filter_mask=q_filter_mask))
        if self.compact_during_next > 0:
            self.compact_during_next -= 1
            self.layout_epoch += 1
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        nq = q.shape[0]
        shift = (group_mask & -group_mask).bit_length() - 1
        keys = (self.tags.astype(np.int64) & group_mask) >> shift
        out_s = np.full((nq, k), -np.inf, dtype=np.float32)
        out_i = np.full((nq, k), -1, dtype=np.int64)
        out_g = np.full((nq, k), -1, dtype=np.int32)
        total = np.zeros(nq, dtype=np.int64)
        for j in range(nq):
            s = (self.x @ q[j]).astype(np.float32)
            ok = self.tags != -1
            if q_filter is not None and q_filter[j] >= 0:
                ok &= ((self.tags & q_filter_mask[j]) if q_filter_mask is not None else self.tags) == q_filter[j]
            assert not np.any(ok & (keys >= n_groups)), "a matching row's group key is >= n_groups"
            rows = np.flatnonzero(ok)
            rows = rows[np.lexsort((rows, -s[rows]))]
            _, first = np.unique(keys[rows], return_index=True)
            reps = rows[np.sort(first)]
            total[j] = len(reps)
            m = min(len(reps), k)
            out_s[j, :m], out_i[j, :m], out_g[j, :m] = s[reps[:m]], reps[:m], keys[reps[:m]]
        return out_s, out_i, out_g, total


def _fill(name, idx):
    """40 chunks of two patients (alice: even n, bob: odd n; every fourth chunk a 'note') whose cosine to the query e0 is
    known by construction and falls with n."""
    REGISTRY.put(IndexState(name, idx))
    cos = np.linspace(0.99, 0.02, 40)
    emb = np.zeros((40, DIM), dtype=np.float32)
    emb[:, 0] = cos
    emb[:, 1] = np.sqrt(1.0 - cos ** 2)
    docs = [{"doc_id": f"d{i}", "patientId": "alice" if i % 2 == 0 else "bob",
             "doc_type": "note" if i % 4 == 3 else "unstructured", "n": i} for i in range(40)]
    indexer.add_documents(name, docs, emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    return q, cos


@pytest.fixture
def world():
    name = "group-cpu"
    idx = StandInIndex()
    q, cos = _fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, cos
    REGISTRY.drop(name)


def test_two_patients_give_two_hits_each_the_patients_best_chunk(world):
    hip, idx, q, cos = world
    hits, total = hip.semantic_search_collapsed(q, k=5)
    assert total == 2 and [(d["patientId"], d["n"]) for d, _ in hits] == [("alice", 0), ("bob", 1)]
    call = idx.calls[-1]
    assert call["group_mask"] == TAG_PATIENT_MASK and call["n_groups"] == 3 and call["k"] == 5     # codes 1, 2 and 0 = none
    assert call["q_filter"] is None and call["q_filter_mask"] is None
    # k below the number of groups: the best group only, the total still says two
    hits, total = hip.semantic_search_collapsed(q, k=1)
    assert total == 2 and [d["n"] for d, _ in hits] == [0]
    # a superseded chunk is tombstoned: alice's runner-up represents her, behind bob now
    indexer.add_documents(hip.index_name, [{"doc_id": "d0", "patientId": "alice", "doc_type": "unstructured", "n": 100}],
                          np.eye(1, DIM, 1, dtype=np.float32))
    hits, total = hip.semantic_search_collapsed(q, k=5)
    assert total == 2 and [d["n"] for d, _ in hits] == [1, 2]
    # a chunk without a patient is a group of its own (group 0), as OpenSearch collapses missing values together
    indexer.add_documents(hip.index_name, [{"doc_id": "anon", "doc_type": "unstructured", "n": 200}],
                          np.eye(1, DIM, 0, dtype=np.float32))
    hits, total = hip.semantic_search_collapsed(q, k=5)
    assert total == 3 and [d["n"] for d, _ in hits] == [200, 1, 2]


def test_collapse_by_doc_type(world):
    hip, idx, q, cos = world
    hits, total = hip.semantic_search_collapsed(q, k=5, collapse="doc_type")
    assert total == 2 and [(d["doc_type"], d["n"]) for d, _ in hits] == [("unstructured", 0), ("note", 3)]
    call = idx.calls[-1]
    assert call["group_mask"] == TAG_DOCTYPE_MASK and call["n_groups"] == 3
    for bad in ("patient", "", None, "doc_id"):
        with pytest.raises(ValueError, match="collapse"):
            hip.semantic_search_collapsed(q, collapse=bad)


def test_filters_are_prepared_as_in_knn(world):
    hip, idx, q, cos = world
    hits, total = hip.semantic_search_collapsed(q, k=5, patient_id="bob")
    assert total == 1 and [(d["patientId"], d["n"]) for d, _ in hits] == [("bob", 1)]
    call = idx.calls[-1]
    assert call["q_filter"].dtype == np.int32 and call["q_filter_mask"].dtype == np.int32
    assert int(call["q_filter_mask"][0]) == TAG_PATIENT_MASK
    assert hip.semantic_search_collapsed(q, k=5, filter_clause={"term": {"patientId": "bob"}}) == (hits, total)
    # doc types of one patient
    hits, total = hip.semantic_search_collapsed(q, k=5, collapse="doc_type", patient_id="bob")
    assert total == 2 and [(d["doc_type"], d["n"]) for d, _ in hits] == [("unstructured", 1), ("note", 3)]
    # patients under a doc_type term filter
    hits, total = hip.semantic_search_collapsed(q, k=5, filter_clause={"term": {"doc_type": "note"}})
    assert total == 1 and [(d["patientId"], d["n"]) for d, _ in hits] == [("bob", 3)]
    n_calls = len(idx.calls)
    assert hip.semantic_search_collapsed(q, patient_id="nobody") == ([], 0)                  # never indexed
    assert hip.semantic_search_collapsed(q, patient_id="bob", filter_clause={"term": {"patientId": "alice"}}) == ([], 0)
    assert hip.semantic_search_collapsed(np.zeros(0)) == ([], 0)
    assert hip.semantic_search_collapsed(None) == ([], 0)
    assert indexer.HipIndexer(None, "no-such-index").semantic_search_collapsed(q) == ([], 0)
    assert len(idx.calls) == n_calls                                                          # none of them searched


@pytest.mark.parametrize("mode", ["opensearch", "cosine"])
def test_scores_are_in_the_units_semantic_search_returns(world, monkeypatch, mode):
    hip, idx, q, cos = world
    monkeypatch.setattr(config, "RASS_SCORE_MODE", mode)
    hits, _ = hip.semantic_search_collapsed(q, k=2)
    for (_, score), c in zip(hits, (cos[0], cos[1])):
        assert isinstance(score, float) and score == pytest.approx(indexer._score_out(float(np.float32(c))), abs=1e-6)
    assert [s for _, s in hits] == sorted((s for _, s in hits), reverse=True)


def test_layout_epoch_retry(world):
    hip, idx, q, cos = world
    idx.compact_during_next = 2                     # two searches see a compaction land under them, the third is clean
    before = len(idx.calls)
    hits, total = hip.semantic_search_collapsed(q, k=4)
    assert len(idx.calls) - before == 3 and total == 2 and len(hits) == 2
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_search_collapsed(q, k=4)
    assert len(idx.calls) - before == 3 + indexer.LAYOUT_ATTEMPTS


def test_an_index_without_the_method_says_so():
    name = "group-cpu-plain"
    q, _ = _fill(name, PlainIndex())
    try:
        with pytest.raises(NotImplementedError, match="grouped search"):
            indexer.HipIndexer(None, name).semantic_search_collapsed(q)
        assert indexer.HipIndexer(None, name).semantic_search_collapsed(np.zeros(0)) == ([], 0)
    finally:
        REGISTRY.drop(name)


def test_flat_index_search_grouped_validates_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def rass_index_search_grouped(self, *a):
            raise AssertionError("the native entry point was reached with bad arguments")

        def rass_index_search_grouped_device(self, *a):
            raise AssertionError("the native entry point was reached with bad arguments")

    idx = FlatIndex(types.SimpleNamespace(_L=Lib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, k=5, group_mask=TAG_PATIENT_MASK, n_groups=10)
    bad = [
        dict(queries=np.zeros(DIM)),                                                  # queries must be [nq, dim]
        dict(queries=np.zeros((3, DIM + 1))),
        dict(k=0), dict(k=4097), dict(k=-3),
        dict(group_mask=0), dict(group_mask=-1), dict(group_mask=0x80000000), dict(group_mask=1 << 32),
        dict(n_groups=0), dict(n_groups=-1), dict(n_groups=(1 << 20) + 1),
        dict(q_filter=np.zeros(2, dtype=np.int32)),
        dict(q_filter_mask=np.zeros(3, dtype=np.int32)),                              # a mask needs a filter
        dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(4, dtype=np.int32)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_grouped(**dict(good, **kw))
    for kw in (dict(k=0), dict(k=4097), dict(group_mask=0), dict(group_mask=0x80000000), dict(n_groups=0), dict(n_groups=(1 << 20) + 1)):
        a = dict(dict(k=5, group_mask=TAG_PATIENT_MASK, n_groups=10), **kw)
        with pytest.raises(ValueError):
            idx.search_grouped_device(0, 3, a["k"], a["group_mask"], a["n_groups"], 0, 0, 0, 0, 0)
    # good arguments do reach it: both bounds of k, of n_groups and of the mask, the doc_type mask, a filter with its mask
    for kw in (dict(), dict(k=1), dict(k=4096), dict(n_groups=1), dict(n_groups=1 << 20), dict(group_mask=1), dict(group_mask=0x7FFFFFFF),
               dict(group_mask=TAG_DOCTYPE_MASK), dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(3, dtype=np.int32))):
        with pytest.raises(AssertionError, match="native entry point"):
            idx.search_grouped(**dict(good, **kw))
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_grouped_device(0, 3, 5, TAG_PATIENT_MASK, 10, 0, 0, 0, 0, 0)
