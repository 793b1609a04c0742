"""The host-side layers of the terms aggregation with top hits, without a GPU: the numpy restatement
(``tests/tophits_ref.py``) against a brute-force loop, the restated emission (counter + slot cascade) against sorting,
``HipIndexer.semantic_aggregate(top_hits=, order=)`` over a stand-in index that answers ``search_counts_hits_by_keys`` in
numpy, the default arguments making exactly the calls they made before, and the argument validation of
``FlatIndex.search_counts_hits_by_keys`` (which refuses before any native call is made)."""
import types

import numpy as np
import pytest

import grouphits_ref as H
import test_group_by_attr_cpu as T
import tophits_ref as R
from rassengine_amd import _native as N
from rassengine_amd import attrfilter, indexer
from rassengine_amd.docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_PATIENT_MASK
from rassengine_amd.engine import FlatIndex

DIM = T.DIM
ORDER_OF = {"_count": R.BY_COUNT, "max_score": R.BY_SCORE}


class TopHitsIndex(T.StandInIndex):
    """The stand-in of tests/test_group_by_attr_cpu.py plus ``search_counts_hits_by_keys`` in numpy."""

    def search_counts_hits_by_keys(self, queries, min_score, size, keys, n_groups, top_hits, order_by="_count", allow=None,
                                   q_filter=None, q_filter_mask=None):
        self._note("search_counts_hits_by_keys", size=size, keys=np.array(keys), n_groups=n_groups, top_hits=top_hits,
                   order_by=order_by, allow=allow)
        keys = np.concatenate([keys, np.full(max(0, self.rows - len(keys)), -1)])
        got = R.expect_top_hits(self._scores(queries), self.tags, keys, n_groups, size, top_hits, min_score, ORDER_OF[order_by],
                                allow, q_filter, q_filter_mask)
        assert got[6] == 0, "a hit's group key is >= n_groups"
        return got[:6]


@pytest.fixture
def world():
    name = "tophits-cpu"
    idx = TopHitsIndex()
    q, cos, docs = T._fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, docs, cos
    REGISTRY.drop(name)


def _ns(hits):
    return [d["n"] for d, _ in hits]


def test_the_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(77)
    for case in range(60):
        n, nq = int(rng.integers(1, 90)), int(rng.integers(1, 4))
        n_groups = int(rng.integers(1, 9))
        scores = rng.integers(-3, 4, size=(nq, n)).astype(np.float32) / 4     # many ties: the row order decides
        if case % 5 == 0:
            scores[0, rng.integers(n)] = -np.inf
            scores[0, rng.integers(n)] = np.nan
        tags = rng.integers(0, 4, size=n).astype(np.int32)
        tags[rng.random(n) < 0.1] = -1
        keys = rng.integers(-1, n_groups + (1 if case % 7 == 0 else 0), size=n)
        thr = rng.choice(np.array([-np.inf, -0.5, 0.0, 0.25, 5.0], dtype=np.float32), size=nq)
        allow = None if case % 3 else (rng.random((nq, n)) < 0.6 if case % 2 else rng.random(n) < 0.6)
        qfilter = None if case % 4 else rng.integers(-1, 4, size=nq).astype(np.int32)
        qmask = None if qfilter is None or case % 8 else np.full(nq, 1, dtype=np.int32)
        for order in (R.BY_COUNT, R.BY_SCORE):
            size, top_hits = int(rng.integers(1, 10)), int(rng.integers(1, 17))
            got = R.expect_top_hits(scores, tags, keys, n_groups, size, top_hits, thr, order, allow, qfilter, qmask)
            want, status = R.brute_force(scores, tags, keys, n_groups, size, top_hits, thr, order, allow, qfilter, qmask)
            assert got[6] == status, case
            for q in range(nq):
                w = want[q]
                assert (got[4][q], got[5][q]) == (w["n_buckets"], w["total"]), case
                listed = [(int(g), int(c)) for g, c in zip(got[0][q], got[1][q]) if g >= 0]
                assert listed == [(g, c) for g, c, _ in w["buckets"]], (case, q, order)
                assert np.all(got[0][q, len(listed):] == -1) and not got[1][q, len(listed):].any()
                for j, (_, _, hits) in enumerate(w["buckets"]):
                    m = len(hits)
                    assert got[3][q, j, :m].tolist() == [r for r, _ in hits], (case, q, j)
                    assert got[2][q, j, :m].tolist() == [s for _, s in hits]
                    assert np.all(got[3][q, j, m:] == -1) and np.all(np.isneginf(got[2][q, j, m:]))
                assert np.all(got[3][q, len(listed):] == -1) and np.all(np.isneginf(got[2][q, len(listed):]))


def test_the_counter_and_the_cascade_under_any_interleaving():
    """The restated emission: whatever order the threads' counter adds, pre-reads and atomic steps interleave in, the counter
    ends as the number of keys — the pre-read that ends a thread comes after its add — and the chain as the ``levels`` largest
    keys, best first: what ``grouphits_ref.cascade`` leaves, and what sorting gives."""
    rng = np.random.default_rng(2025)
    for case in range(600):
        n = int(rng.integers(0, 41))
        levels = int(rng.integers(1, 17))
        keys = rng.choice(np.arange(1, 10_000), size=n, replace=False)
        want = sorted(keys.tolist(), reverse=True)[:levels]
        want += [0] * (levels - len(want))
        count, slots = R.count_and_cascade(keys, levels, rng)
        assert count == n and slots == want == H.cascade(keys, levels, rng), (case, n, levels)


def test_top_hits_per_bucket(world):
    hip, idx, q, docs, cos = world
    # three patients (n % 3), the cosine falls with n: patient p's chunks best first are p, p + 3, p + 6, ...
    agg = hip.semantic_aggregate(q, 0.0, by="patientId", top_hits=3)
    assert [(b["key"], b["doc_count"], _ns(b["top_hits"])) for b in agg["buckets"]] == \
        [("alice", 14, [0, 3, 6]), ("bob", 13, [1, 4, 7]), ("carol", 13, [2, 5, 8])]
    assert all(b["top_hit"] == b["top_hits"][0] for b in agg["buckets"]) and agg["total"] == 40 and agg["cardinality"] == 3
    assert [c["fn"] for c in idx.calls[-2:]] == ["group_keys_from_tag", "search_counts_hits_by_keys"]
    assert idx.calls[-2]["mask"] == TAG_PATIENT_MASK
    call = idx.calls[-1]
    assert (call["size"], call["n_groups"], call["top_hits"], call["order_by"], call["allow"]) == (5, 4, 3, "_count", None)
    for b in agg["buckets"]:
        assert all(isinstance(s, float) for _, s in b["top_hits"])
        assert [s for _, s in b["top_hits"]] == sorted((s for _, s in b["top_hits"]), reverse=True)
    # the counts, the order and the first hit are the plain aggregation's, for every kind of field
    for by, kw in (("patientId", {}), ("doc_type", {}), ("resourceType", {}), ("code", {}), ("patientId", dict(patient_id="bob")),
                   ("chunkDate", dict(interval="month")),
                   ("code", dict(interval=2))):
        plain = hip.semantic_aggregate(q, 0.3, by=by, size=3, **kw)
        for th in (2, 16):
            got = hip.semantic_aggregate(q, 0.3, by=by, size=3, top_hits=th, **kw)
            assert {k: v for k, v in got.items() if k != "buckets"} == {k: v for k, v in plain.items() if k != "buckets"}, (by, kw)
            assert [{k: v for k, v in b.items() if k != "top_hits"} for b in got["buckets"]] == plain["buckets"], (by, kw, th)
            assert all(1 <= len(b["top_hits"]) <= min(th, b["doc_count"]) for b in got["buckets"])
            assert all(len(b["top_hits"]) == min(th, b["doc_count"]) for b in got["buckets"])
    # a bucket with fewer hits than top_hits is a shorter list; a threshold cuts the lists as it cuts the counts
    agg = hip.semantic_aggregate(q, 0.8, by="patientId", top_hits=16)
    first = {"alice": 0, "bob": 1, "carol": 2}
    assert len(agg["buckets"]) == 3 and 3 <= agg["total"] < 40 and len({b["doc_count"] for b in agg["buckets"]}) == 2
    for b in agg["buckets"]:
        assert _ns(b["top_hits"]) == [first[b["key"]] + 3 * i for i in range(b["doc_count"])] and b["doc_count"] < 16
    # a tombstoned chunk: the runner-ups move up
    idx.delete(0)
    agg = hip.semantic_aggregate(q, 0.0, by="patientId", top_hits=2)
    assert [(b["key"], b["doc_count"], _ns(b["top_hits"])) for b in agg["buckets"]] == \
        [("alice", 13, [3, 6]), ("bob", 13, [1, 4]), ("carol", 13, [2, 5])]


def test_where_restricts_the_counts_and_the_lists(world, monkeypatch):
    hip, idx, q, docs, cos = world

    def run_plan(index, plan):      # the one shape these filters compile to, through the stand-in's builder
        assert plan[0] == "all"
        return index.allow_from_attr_clauses(np.array([(0, c, lo, hi, neg) for c, lo, hi, neg in plan[1]]).reshape(-1, 5),
                                             nq=1, shared=True, mode="all")

    monkeypatch.setattr(attrfilter, "run_plan", run_plan)
    where = {"range": {"chunkDate": {"gte": "2024-02-01", "lt": "2024-03-01"}}}
    inside = [d for d in docs if "2024-02-01" <= d.get("chunkDate", "") < "2024-03-01"]
    for by in ("resourceType", "patientId"):
        agg = hip.semantic_aggregate(q, 0.0, by=by, where=where, top_hits=3)
        want = {}
        for d in inside:
            want.setdefault(d.get(by), []).append(d["n"])
        assert {b["key"]: (b["doc_count"], _ns(b["top_hits"])) for b in agg["buckets"]} == {k: (len(v), sorted(v)[:3]) for k, v in want.items()}
        call = idx.calls[-1]
        assert call["fn"] == "search_counts_hits_by_keys" and call["allow"].dtype == bool and call["allow"].sum() == len(inside)
        assert agg["total"] == len(inside)


def test_order_by_max_score(world):
    hip, idx, q, docs, cos = world
    # doc_type: 30 unstructured chunks (best n = 0), 10 notes (best n = 3); resourceType None (n % 4 == 2) has the third-best chunk
    by_count = hip.semantic_aggregate(q, 0.0, by="resourceType", size=4)
    assert [b["key"] for b in by_count["buckets"]] == [None, "Condition", "Observation", "Procedure"]       # 10 each: by key
    idx.delete(0)
    idx.delete(4)                                               # Condition loses its two best chunks: n = 8 is its best now
    by_score = hip.semantic_aggregate(q, 0.0, by="resourceType", size=4, order="max_score")
    assert [(b["key"], b["top_hit"][0]["n"]) for b in by_score["buckets"]] == [("Observation", 1), (None, 2), ("Procedure", 3), ("Condition", 8)]
    assert all(len(b["top_hits"]) == 1 and b["top_hits"][0] == b["top_hit"] for b in by_score["buckets"])
    assert idx.calls[-1]["order_by"] == "max_score" and idx.calls[-1]["top_hits"] == 1
    cut = hip.semantic_aggregate(q, 0.0, by="resourceType", size=2, order="max_score", top_hits=2)
    assert [(b["key"], b["doc_count"], _ns(b["top_hits"])) for b in cut["buckets"]] == [("Observation", 10, [1, 5]), (None, 10, [2, 6])]
    assert cut["cardinality"] == 4 and cut["total"] == 38 and cut["sum_other_doc_count"] == 18
    with pytest.raises(ValueError, match="key order"):
        hip.semantic_aggregate(q, 0.0, by="code", interval=2, order="max_score")


def test_the_defaults_make_the_calls_they_made(world):
    hip, idx, q, docs, cos = world
    hip.semantic_aggregate(q, 0.0, by="doc_type")
    assert idx.calls[-1] == dict(fn="search_counts", size=5, group_mask=TAG_DOCTYPE_MASK, n_groups=3)
    hip.semantic_aggregate(q, 0.0, by="patientId", top_hits=1, order="_count")
    assert idx.calls[-1] == dict(fn="search_counts", size=5, group_mask=TAG_PATIENT_MASK, n_groups=4)
    agg = hip.semantic_aggregate(q, 0.0, by="resourceType")
    assert idx.calls[-1]["fn"] == "search_counts_by_keys" and all("top_hits" not in b for b in agg["buckets"])
    assert not any(c["fn"] == "search_counts_hits_by_keys" for c in idx.calls)


def test_value_errors_and_empty_answers(world):
    hip, idx, q, docs, cos = world
    n_calls = len(idx.calls)
    for bad in (0, 17, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="top_hits"):
            hip.semantic_aggregate(q, 0.0, top_hits=bad)
    for bad in ("count", "score", None, {"max_score": "desc"}):
        with pytest.raises(ValueError, match="order must be"):
            hip.semantic_aggregate(q, 0.0, order=bad)
    with pytest.raises(ValueError, match="by must be"):
        hip.semantic_aggregate(q, 0.0, by="doc_id", top_hits=3)
    assert hip.semantic_aggregate(np.zeros(0), 0.0, top_hits=3) == T.EMPTY
    assert hip.semantic_aggregate(q, 0.0, top_hits=3, patient_id="nobody") == T.EMPTY
    assert indexer.HipIndexer(None, "no-such-index").semantic_aggregate(q, 0.0, top_hits=3, order="max_score") == T.EMPTY
    assert len(idx.calls) == n_calls
    idx.compact_during_next = 2                     # the key column of two attempts is built for a layout that then moves
    agg = hip.semantic_aggregate(q, 0.0, top_hits=2)
    assert [_ns(b["top_hits"]) for b in agg["buckets"]] == [[0, 3], [1, 4], [2, 5]]


def test_an_index_without_the_method_says_so():
    for cls, dim, what in ((T.StandInIndex, DIM, "top hits"), (TopHitsIndex, 1100, "dim <= 1024")):
        name = "tophits-cpu-plain"
        idx = cls()
        q, _, _ = T._fill(name, idx)
        idx.dim = dim
        try:
            hip = indexer.HipIndexer(None, name)
            with pytest.raises(NotImplementedError, match=what):
                hip.semantic_aggregate(q, 0.0, top_hits=2)
            with pytest.raises(NotImplementedError, match=what):
                hip.semantic_aggregate(q, 0.0, order="max_score")
            assert hip.semantic_aggregate(q, 0.0)["total"] == 40      # the defaults still go the way they went
        finally:
            REGISTRY.drop(name)


def test_flat_index_validates_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def __getattr__(self, name):
            def reached(*a):
                raise AssertionError("the native entry point was reached with bad arguments")
            return reached

    idx = FlatIndex(types.SimpleNamespace(_L=Lib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, min_score=0.5, size=5, keys=np.zeros(4, dtype=np.int32), n_groups=10, top_hits=3)
    bad = [dict(size=0), dict(size=4097), dict(n_groups=0), dict(n_groups=(1 << 20) + 1), dict(top_hits=0), dict(top_hits=17),
           dict(top_hits=-1), dict(n_groups=(1 << 20) // 2, top_hits=3), dict(n_groups=1 << 20, top_hits=2), dict(order_by="score"),
           dict(order_by=None), dict(order_by=1), dict(min_score=float("nan")), dict(min_score=[0.1, 0.2]),
           dict(keys=np.zeros(4, dtype=np.float32)), dict(q_filter_mask=np.zeros(3, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_counts_hits_by_keys(**dict(good, **kw))
    for a in (dict(size=0), dict(top_hits=0), dict(top_hits=17), dict(n_groups=1 << 20, top_hits=2), dict(order_by="min")):
        a = dict(dict(size=5, n_groups=10, top_hits=3, order_by="_count"), **a)
        with pytest.raises(ValueError):
            idx.search_counts_hits_by_keys_device(0, 3, 0, a["size"], 0, 4, a["n_groups"], a["top_hits"], 0, 0, 0, 0, 0, 0, 0,
                                                  order_by=a["order_by"])
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_counts_hits_by_keys_device(0, 3, 0, 4096, 0, 4, 1 << 16, 16, 0, 0, 0, 0, 0, 0, 0, order_by="max_score")
    assert (N.RASS_AGG_BY_COUNT, N.RASS_AGG_BY_SCORE) == (0, 1) == (R.BY_COUNT, R.BY_SCORE)
    assert FlatIndex.AGG_ORDERS == {"_count": 0, "max_score": 1}
