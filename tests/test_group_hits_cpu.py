"""The host-side layers of the grouped search with inner hits, without a GPU: ``HipIndexer.semantic_search_collapsed_hits``
and ``semantic_search_capped`` over a stand-in index that answers ``search_group_hits`` in numpy (``tests/grouphits_ref.py``),
the argument validation of ``FlatIndex.search_group_hits`` (which refuses before any native call is made), and the numpy
restatement of the scan's slot cascade against sorting."""
import types

import numpy as np
import pytest

import grouphits_ref as H
import test_group_by_attr_cpu as T
from rassengine_amd import indexer
from rassengine_amd.docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_PATIENT_MASK
from rassengine_amd.engine import FlatIndex

DIM = T.DIM


class HitsIndex(T.StandInIndex):
    """The stand-in of tests/test_group_by_attr_cpu.py plus ``search_group_hits`` in numpy."""

    def search_group_hits(self, queries, k, keys, n_groups, group_size, allow=None, q_filter=None, q_filter_mask=None, capped=False):
        self._note("search_group_hits", k=k, keys=np.array(keys), n_groups=n_groups, group_size=group_size, allow=allow, capped=capped,
                   q_filter=q_filter, q_filter_mask=q_filter_mask)
        keys = np.concatenate([keys, np.full(max(0, self.rows - len(keys)), -1)])
        got = H.expect_group_hits(self._scores(queries), self.tags, keys, n_groups, k, group_size, allow, q_filter, q_filter_mask)
        assert got[6] == 0, "a matching row's group key is >= n_groups"
        return got[:6] if capped else got[:4]


@pytest.fixture
def world():
    name = "ghits-cpu"
    idx = HitsIndex()
    q, cos, docs = T._fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, docs
    REGISTRY.drop(name)


def _ns(hits):
    return [d["n"] for d, _ in hits]


def test_shapes_and_the_first_inner_hit_is_the_collapsed_hit(world):
    hip, idx, q, docs = world
    # three patients (n % 3), the cosine falls with n: patient p's chunks best first are p, p + 3, p + 6, ...
    groups, total = hip.semantic_search_collapsed_hits(q, k=5, inner_hits=3)
    assert total == 3 and [_ns(g) for g in groups] == [[0, 3, 6], [1, 4, 7], [2, 5, 8]]
    call = idx.calls[-1]
    assert call["fn"] == "search_group_hits" and call["k"] == 5 and call["group_size"] == 3 and call["capped"] is False
    assert call["n_groups"] == 4 and call["allow"] is None                      # codes 1 .. 3 and 0 = none, through a key column
    assert [c["fn"] for c in idx.calls[-2:]] == ["group_keys_from_tag", "search_group_hits"] and idx.calls[-2]["mask"] == TAG_PATIENT_MASK
    for g in groups:
        assert all(isinstance(s, float) for _, s in g) and [s for _, s in g] == sorted((s for _, s in g), reverse=True)
    for collapse, kw in (("patientId", {}), ("doc_type", {}), ("resourceType", {}), ("code", {}),
                         ("patientId", dict(patient_id="bob")), ("doc_type", dict(filter_clause={"term": {"patientId": "carol"}}))):
        flat, total1 = hip.semantic_search_collapsed(q, k=3, collapse=collapse, **kw)
        for inner in (1, 2, 16):
            groups, total = hip.semantic_search_collapsed_hits(q, k=3, collapse=collapse, inner_hits=inner, **kw)
            assert total == total1 and [g[0] for g in groups] == flat, (collapse, kw, inner)
            assert all(1 <= len(g) <= inner for g in groups)
    # k below the number of groups; a group smaller than inner_hits is a shorter list (doc_type note: n % 4 == 3, 10 chunks)
    groups, total = hip.semantic_search_collapsed_hits(q, k=1, inner_hits=2)
    assert total == 3 and [_ns(g) for g in groups] == [[0, 3]]
    groups, total = hip.semantic_search_collapsed_hits(q, k=4, collapse="doc_type", inner_hits=16)
    assert total == 2 and [len(g) for g in groups] == [16, 10] and _ns(groups[1]) == list(range(3, 40, 4))
    assert idx.calls[-2]["mask"] == TAG_DOCTYPE_MASK
    # a tombstoned chunk: the runner-ups move up
    idx.delete(0)
    groups, _ = hip.semantic_search_collapsed_hits(q, k=5, inner_hits=2)
    assert [_ns(g) for g in groups] == [[1, 4], [2, 5], [3, 6]]


def test_capped(world):
    hip, idx, q, docs = world
    hits = hip.semantic_search_capped(q, k=5, max_per_group=1)
    assert _ns(hits) == [0, 1, 2] and idx.calls[-1]["capped"] is True and idx.calls[-1]["group_size"] == 1
    assert _ns(hip.semantic_search_capped(q, k=5, max_per_group=2)) == [0, 1, 2, 3, 4]
    assert _ns(hip.semantic_search_capped(q, k=8, max_per_group=2)) == [0, 1, 2, 3, 4, 5]
    # by doc_type (note: n % 4 == 3): at most two notes and two others
    assert _ns(hip.semantic_search_capped(q, k=10, per="doc_type", max_per_group=2)) == [0, 1, 3, 7]
    # a cap no group reaches: the plain top-k
    assert _ns(hip.semantic_search_capped(q, k=7, max_per_group=16)) == list(range(7))
    assert _ns(hip.semantic_search_capped(q, k=4, max_per_group=2, patient_id="bob")) == [1, 4]
    scores = [s for _, s in hip.semantic_search_capped(q, k=6, max_per_group=3)]
    assert scores == sorted(scores, reverse=True) and all(isinstance(s, float) for s in scores)


def test_empty_answers_search_nothing(world):
    hip, idx, q, docs = world
    n_calls = len(idx.calls)
    for kw in (dict(patient_id="nobody"), dict(patient_id="bob", filter_clause={"term": {"patientId": "alice"}})):
        assert hip.semantic_search_collapsed_hits(q, **kw) == ([], 0)
        assert hip.semantic_search_capped(q, **kw) == []
    for emb in (np.zeros(0), None):
        assert hip.semantic_search_collapsed_hits(emb) == ([], 0)
        assert hip.semantic_search_capped(emb) == []
    ghost = indexer.HipIndexer(None, "no-such-index")
    assert ghost.semantic_search_collapsed_hits(q) == ([], 0) and ghost.semantic_search_capped(q) == []
    assert len(idx.calls) == n_calls
    for bad in ("patient", "", None, "doc_id"):
        with pytest.raises(ValueError, match="collapse"):
            hip.semantic_search_collapsed_hits(q, collapse=bad)
        with pytest.raises(ValueError, match="per"):
            hip.semantic_search_capped(q, per=bad)


def test_layout_epoch_retry(world):
    hip, idx, q, docs = world
    idx.compact_during_next = 2                     # the key column of two attempts is built for a layout that then moves
    hits = hip.semantic_search_capped(q, k=4, max_per_group=1)
    assert _ns(hits) == [0, 1, 2]
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_search_collapsed_hits(q, k=4)


def test_an_index_without_the_method_says_so():
    for cls, dim, what in ((T.StandInIndex, DIM, "inner hits"), (HitsIndex, 1100, "dim <= 1024")):
        name = "ghits-cpu-plain"
        idx = cls()
        q, _, _ = T._fill(name, idx)
        idx.dim = dim
        try:
            hip = indexer.HipIndexer(None, name)
            with pytest.raises(NotImplementedError, match=what):
                hip.semantic_search_collapsed_hits(q)
            with pytest.raises(NotImplementedError, match=what):
                hip.semantic_search_capped(q)
            assert hip.semantic_search_collapsed_hits(np.zeros(0)) == ([], 0)
        finally:
            REGISTRY.drop(name)


def test_flat_index_search_group_hits_validates_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def __getattr__(self, name):
            def reached(*a):
                raise AssertionError("the native entry point was reached with bad arguments")
            return reached

    idx = FlatIndex(types.SimpleNamespace(_L=Lib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, k=5, keys=np.zeros(4, dtype=np.int32), n_groups=10, group_size=3)
    bad = [dict(k=0), dict(k=4097), dict(n_groups=0), dict(n_groups=(1 << 20) + 1), dict(group_size=0), dict(group_size=17),
           dict(group_size=-1), dict(n_groups=(1 << 20) // 2, group_size=3), dict(n_groups=1 << 20, group_size=2),
           dict(k=2048, group_size=3, capped=True), dict(k=4096, group_size=2, capped=True),
           dict(keys=np.zeros(4, dtype=np.float32)), dict(q_filter_mask=np.zeros(3, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_group_hits(**dict(good, **kw))
    for a in (dict(k=0), dict(group_size=0), dict(group_size=17), dict(n_groups=1 << 20, group_size=2)):
        a = dict(dict(k=5, n_groups=10, group_size=3), **a)
        with pytest.raises(ValueError):
            idx.search_group_hits_device(0, 3, a["k"], 0, 4, a["n_groups"], a["group_size"], 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):     # the capped bound holds only where the capped outputs are asked for
        idx.search_group_hits_device(0, 3, 2048, 0, 4, 10, 3, 0, 0, 0, 0, 0, d_out_capped_scores_ptr=8, d_out_capped_ids_ptr=8)
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_group_hits_device(0, 3, 2048, 0, 4, 10, 3, 0, 0, 0, 0, 0)
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_group_hits_device(0, 3, 4096, 0, 4, 1 << 16, 16, 0, 0, 0, 0, 0)


def test_the_cascade_keeps_the_largest_keys_under_any_interleaving():
    """The numpy restatement of the scan's emission (``grouphits_ref.cascade``): whatever order the threads' pre-reads and
    atomic steps interleave in, the chain ends as the ``levels`` largest keys, best first, zeros behind them."""
    rng = np.random.default_rng(2024)
    for case in range(600):
        n = int(rng.integers(0, 41))
        levels = int(rng.integers(1, 17))
        keys = rng.choice(np.arange(1, 10_000), size=n, replace=False)
        want = sorted(keys.tolist(), reverse=True)[:levels]
        want += [0] * (levels - len(want))
        assert H.cascade(keys, levels, rng) == want, (case, n, levels)
    # one level is the group-max scan's slot
    assert H.cascade(np.array([5, 9, 2]), 1, rng) == [9]
