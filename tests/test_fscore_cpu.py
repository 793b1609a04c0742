"""The host-side layers of the function-score search, without a GPU: ``attrfilter.compile_functions`` on every function shape
(date math at a pinned ``now``) and its refusals, the numpy restatement (``fscore_ref``) against hand-computed values, and
``HipIndexer.semantic_search_scored`` / ``semantic_search_recent`` over a stand-in index that answers ``fn_from_attr`` and
``search_scored`` with ``fscore_ref``; the record layout of the binding table against the header's struct."""
import ctypes
import datetime as dt
import math
import os
import re

import numpy as np
import pytest

import attr_ref as AR
import boost_ref as B
import fscore_ref as F
from rassengine_amd import _native, attrfilter, config, indexer
from rassengine_amd.docstore import REGISTRY, IndexState
from rassengine_amd.engine import FlatIndex
from test_boost_search_cpu import DIM, KINDS, NOW, StandInIndex, _docs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = np.float32(-np.inf)
TODAY = (NOW.date() - dt.date(1970, 1, 1)).days


def day(s):
    return (dt.date.fromisoformat(s) - dt.date(1970, 1, 1)).days


# ---------------------------------------------------------------------------------------------- the stand-in index
class ScoredIndex(StandInIndex):
    """``StandInIndex`` plus the function column builder and the function-score search in numpy (``fscore_ref``)."""

    def attr_minmax(self, col):
        v = self.cols.get(col, np.zeros(0, dtype=np.int64))
        have = v[v != F.ATTR_MISSING]
        return (int(have.min()), int(have.max()), int(len(have))) if len(have) else (None, None, 0)

    def fn_from_attr(self, column, functions, score_mode="multiply", max_boost=None, filters=None):
        self.calls.append(dict(fn="fn", functions=[dict(f) for f in functions], score_mode=score_mode, max_boost=max_boost,
                               n_filters=len(filters or [])))
        bits = np.stack([np.asarray(f, dtype=bool) for f in filters]) if filters else None
        column[:self.rows] = F.build_column(functions, self.cols, self.rows, 1, score_mode, max_boost, bits)[0]
        return column

    def search_scored(self, queries, k, column, boost=None, transform="raw", combine="multiply", min_score=None, q_filter=None,
                      q_filter_mask=None):
        self.calls.append(dict(fn="scored", k=k, boost=boost, transform=transform, combine=combine, min_score=min_score))
        s = self.cosines(queries)
        bst = None if boost is None else np.full(len(s), boost, dtype=np.float32)
        gate = None if min_score is None else np.full(len(s), min_score, dtype=np.float32)
        return F.search(s, k, column, bst, transform, combine, gate, self.live(len(s), q_filter, q_filter_mask))


@pytest.fixture
def world(monkeypatch):
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,chunkDate:date,pages:int")
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "opensearch")
    name = "fscore-cpu"
    idx = ScoredIndex()
    st = IndexState(name, idx)
    st.attrs.clock = lambda: NOW
    REGISTRY.put(st)
    cos = np.linspace(0.99, 0.02, 40)
    emb = np.zeros((40, DIM), dtype=np.float32)
    emb[:, 0] = cos
    emb[:, 1] = np.sqrt(1.0 - cos ** 2)
    indexer.add_documents(name, _docs(), emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    # a filter plan is evaluated in numpy here (attrfilter.run_plan needs the GPU)
    monkeypatch.setattr(attrfilter, "run_plan", lambda index, plan: AR.eval_plan(plan, index.cols, index.tags))
    yield indexer.HipIndexer(None, name), idx, st, q
    REGISTRY.drop(name)


def ids(hits):
    return [d["n"] for d, _ in hits]


# ---------------------------------------------------------------------------------------------- compile_functions
def test_compile_functions_every_shape(world):
    hip, idx, st, q = world
    comp = lambda fns: attrfilter.compile_functions(fns, st.attrs, st.patients, st.doc_types)
    cond = {"term": {"resourceType": "Condition"}}
    recs, flts = comp([
        {"gauss": {"chunkDate": {"origin": "now-30d/d", "scale": "30d", "offset": "1w", "decay": 0.25}}},
        {"exp": {"pages": {"origin": 10, "scale": 5}}, "weight": 2},
        {"linear": {"chunkDate": {"scale": 90}}, "filter": cond},
        {"gauss": {"chunkDate": {"origin": "2023-06-01", "scale": "2w"}}},
        {"field_value_factor": {"field": "pages", "factor": 1.2, "modifier": "log1p", "missing": 1}},
        {"field_value_factor": {"field": "chunkDate"}},
        {"weight": 3.5, "filter": {"range": {"chunkDate": {"gte": "now-1y"}}}},
    ])
    plan = lambda f: attrfilter.compile_filter(f, st.attrs, st.patients, st.doc_types)
    assert flts == [plan(cond), plan({"range": {"chunkDate": {"gte": "now-1y"}}})]     # each filter compiled once, as a filter is
    assert recs[0] == dict(kind="gauss", col=1, origin=float(TODAY - 30), scale=30.0, offset=7.0, decay=0.25, weight=1.0, filter=None)
    assert recs[1] == dict(kind="exp", col=2, origin=10.0, scale=5.0, offset=0.0, decay=0.5, weight=2.0, filter=None)
    assert recs[2] == dict(kind="linear", col=1, origin=float(TODAY), scale=90.0, offset=0.0, decay=0.5, weight=1.0, filter=0)
    assert recs[3]["origin"] == float(day("2023-06-01")) and recs[3]["scale"] == 14.0
    assert recs[4] == dict(kind="field_value_factor", col=2, factor=1.2, modifier="log1p", missing=1.0, weight=1.0, filter=None)
    assert recs[5] == dict(kind="field_value_factor", col=1, factor=1.0, modifier="none", missing=None, weight=1.0, filter=None)
    assert recs[6] == dict(kind="weight", col=0, weight=3.5, filter=1)
    assert comp(None) == ([], []) and comp([]) == ([], [])
    pinned = attrfilter.compile_functions([{"gauss": {"chunkDate": {"origin": "now", "scale": "1d"}}}], st.attrs, st.patients,
                                          st.doc_types, now=dt.datetime(2020, 1, 2, 23, 59, tzinfo=dt.timezone.utc))
    assert pinned[0][0]["origin"] == float(day("2020-01-02"))
    # the records are what FlatIndex.fn_from_attr packs
    packed, n = FlatIndex._fn_records(recs)
    assert n == 7 and packed[0].kind == _native.RASS_FN_GAUSS and packed[0].col == 1 and packed[0].filter == -1
    assert packed[2].filter == 0 and packed[4].modifier == _native.RASS_FN_MOD_LOG1P and packed[4].missing == 1.0
    assert math.isnan(packed[5].missing) and packed[6].kind == _native.RASS_FN_WEIGHT and packed[6].weight == 3.5


@pytest.mark.parametrize("bad", [
    {"gauss": {"chunkDate": {"scale": "12h"}}},                       # finer than a day
    {"gauss": {"chunkDate": {"scale": "500ms"}}},
    {"gauss": {"chunkDate": {"scale": "30d", "offset": "90m"}}},
    {"gauss": {"chunkDate": {"scale": "soon"}}},
    {"gauss": {"chunkDate": {"origin": "yesterday-ish", "scale": "3d"}}},
    {"gauss": {"chunkDate": {"origin": "now"}}},                      # no scale
    {"gauss": {"chunkDate": {"scale": "0d"}}},
    {"gauss": {"pages": {"scale": 5}}},                               # an int field needs an origin
    {"gauss": {"pages": {"origin": 1, "scale": -5}}},
    {"exp": {"pages": {"origin": 1, "scale": 5, "decay": 1.0}}},
    {"exp": {"pages": {"origin": 1, "scale": 5, "decay": 0}}},
    {"linear": {"pages": {"origin": 1, "scale": 5, "offset": -1}}},
    {"linear": {"pages": {"origin": 1, "scale": 5, "multi_value_mode": "min"}}},
    {"gauss": {"resourceType": {"origin": 1, "scale": 5}}},           # a keyword has no numeric value
    {"gauss": {"nope": {"origin": 1, "scale": 5}}},
    {"field_value_factor": {"field": "resourceType"}},
    {"field_value_factor": {"field": "pages", "modifier": "cube"}},
    {"field_value_factor": {"field": "pages", "factor": float("nan")}},
    {"field_value_factor": {"factor": 2}},
    {"weight": float("inf")},
    {"weight": "3"},
    {},
    {"filter": {"term": {"resourceType": "Condition"}}},              # a filter function needs a weight
    {"gauss": {"pages": {"origin": 1, "scale": 5}}, "exp": {"pages": {"origin": 1, "scale": 5}}},
    {"random_score": {}},
    {"script_score": {"script": "1"}},
    {"weight": 2, "filter": {"match": {"text": "x"}}},               # a filter the compiler refuses
    "gauss",
])
def test_compile_functions_refusals(world, bad):
    hip, idx, st, q = world
    with pytest.raises(ValueError):
        attrfilter.compile_functions([bad], st.attrs, st.patients, st.doc_types)


# ---------------------------------------------------------------------------------------------- the restatement
def test_restatement_builder_hand_values():
    cols = {0: np.array([100, 110, 90, 130, 105, F.ATTR_MISSING, 95]), 1: np.array([4, 0, -3, 9, F.ATTR_MISSING, 16, 1])}
    n = 7
    gauss = {"kind": "gauss", "col": 0, "origin": 100.0, "scale": 10.0, "offset": 0.0, "decay": 0.3}
    col = F.build_column([gauss], cols, n, as_f64=True)[0]
    assert col[0] == 1.0 and col[5] == 1.0                                       # at the origin; a missing field
    assert np.isclose(col[1], 0.3, rtol=1e-14, atol=0) and col[1] == col[2]      # a gauss at d = scale is decay
    assert np.isclose(col[3], 0.3 ** 9, rtol=1e-13, atol=0)                      # d = 3 scale: decay^9
    assert F.build_column([gauss], cols, n)[0][1] == np.float32(0.3)
    off = F.build_column([dict(gauss, offset=5.0)], cols, n, as_f64=True)[0]
    assert off[4] == 1.0 and off[6] == 1.0 and np.isclose(off[1], 0.3 ** 0.25, rtol=1e-14)    # d = max(0, |v - o| - offset)
    e = F.build_column([dict(gauss, kind="exp")], cols, n, as_f64=True)[0]
    assert np.isclose(e[1], 0.3, rtol=1e-14) and np.isclose(e[3], 0.3 ** 3, rtol=1e-14)
    lin = F.build_column([dict(gauss, kind="linear", decay=0.5)], cols, n, as_f64=True)[0]     # s = 10 / 0.5 = 20
    assert lin[1] == 0.5 and lin[0] == 1.0 and lin[3] == 0.0 and lin[5] == 1.0                # 0.5 at d = scale, 0 from d = s on
    assert F.build_column([dict(gauss, kind="linear", decay=0.5, origin=80.0)], cols, n, as_f64=True)[0][0] == 0.0   # exactly d = s
    # field_value_factor: the modifiers, `missing`, and "does not apply" -> 1.0
    fv = lambda **kw: F.build_column([dict({"kind": "field_value_factor", "col": 1}, **kw)], cols, n, as_f64=True)[0]
    assert fv(factor=2.0).tolist() == [8.0, 0.0, -6.0, 18.0, 1.0, 32.0, 2.0]
    assert fv(factor=2.0, missing=5.0)[4] == 10.0
    assert fv(modifier="sqrt")[[0, 3, 5]].tolist() == [2.0, 3.0, 4.0] and np.isnan(fv(modifier="sqrt")[2])
    assert fv(modifier="square", factor=0.5)[5] == 64.0 and fv(modifier="reciprocal")[0] == 0.25 and np.isinf(fv(modifier="reciprocal")[1])
    assert fv(modifier="log1p")[3] == 1.0 and fv(modifier="log2p", factor=98.0)[6] == 2.0 and fv(modifier="log", factor=10.0)[6] == 1.0
    assert np.isclose(fv(modifier="ln")[0], math.log(4)) and np.isclose(fv(modifier="ln1p")[0], math.log(5)) and \
        np.isclose(fv(modifier="ln2p")[0], math.log(6))
    assert fv(modifier="ln")[1] == -np.inf and np.isnan(fv(modifier="ln")[2])  # OpenSearch raises; here the scan drops the row
    # score modes over two functions and a filtered weight; the weighted average
    bits = np.array([[1, 1, 0, 0, 1, 1, 0]], dtype=bool)
    a = {"kind": "field_value_factor", "col": 1, "factor": 1.0, "weight": 2.0}   # 2 v; skips row 4
    b = {"kind": "weight", "weight": 3.0, "filter": 0}                           # 3 on rows 0, 1, 4, 5
    both = lambda mode, cap=None: F.build_column([a, b], cols, n, 1, mode, cap, bits, as_f64=True)[0].tolist()
    assert both("multiply") == [24.0, 0.0, -6.0, 18.0, 3.0, 96.0, 2.0]
    assert both("sum") == [11.0, 3.0, -6.0, 18.0, 3.0, 35.0, 2.0]
    assert both("avg") == [11.0 / 5, 3.0 / 5, -6.0 / 2, 18.0 / 2, 3.0 / 3, 35.0 / 5, 2.0 / 2]    # sum(w x) / sum(w)
    assert both("first") == [8.0, 0.0, -6.0, 18.0, 3.0, 32.0, 2.0]
    assert both("max") == [8.0, 3.0, -6.0, 18.0, 3.0, 32.0, 2.0] and both("min") == [3.0, 0.0, -6.0, 18.0, 3.0, 3.0, 2.0]
    assert both("sum", 10.0) == [10.0, 3.0, -6.0, 10.0, 3.0, 10.0, 2.0]         # max_boost caps
    none = F.build_column([dict(b, filter=0)], cols, n, 1, "sum", None, np.zeros((1, n), dtype=bool))[0]
    assert (none == 1.0).all() and (F.build_column([], cols, n, 2) == 1.0).all()  # no function applies: 1.0
    two = F.build_column([dict(a, query=1), b], cols, n, 2, "sum", None, bits, as_f64=True)
    assert two[0].tolist() == [3.0, 3.0, 1.0, 1.0, 3.0, 3.0, 1.0] and two[1].tolist() == [8.0, 0.0, -6.0, 18.0, 1.0, 32.0, 2.0]
    assert F.libm_cells([gauss, dict(a, query=1)], cols, n, 2).tolist() == [[True] * 7, [False] * 7]
    assert F.ulp_distance(np.float32([1.0, np.nan, 0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), np.nan, -0.0])).tolist() == [1, 0, 0]


def test_restatement_scan_rules():
    cos = np.array([[0.5, np.nan, 0.4, 0.3, -np.inf, 0.2, 0.2, 0.1]], dtype=np.float32)
    f = np.array([2.0, 9.0, -np.inf, np.nan, 9.0, 0.25, 0.25, -3.0], dtype=np.float32)
    top = lambda mode, **kw: F.search(cos, 4, f, mode=mode, **kw)
    eq = lambda got, want: np.array_equal(got, np.asarray(want, dtype=np.float32))
    assert top("sum")[1][0].tolist() == [0, 5, 6, 7] and eq(top("sum")[0][0], cos[0, [0, 5, 6, 7]] + f[[0, 5, 6, 7]])
    assert top("multiply")[1][0].tolist() == [0, 5, 6, 7] and top("multiply")[0][0, 3] == np.float32(0.1) * np.float32(-3.0)
    assert top("avg")[0][0, 0] == 1.25 and eq(top("replace")[0][0], [2.0, 0.25, 0.25, -3.0])
    # a -inf or NaN cell excludes the row in every mode: max would otherwise report the cosine, replace the cell
    for mode in F.COMBINE:
        assert set(top(mode)[1][0].tolist()) == {0, 5, 6, 7}, mode
    assert eq(top("max")[0][0], [2.0, 0.25, 0.25, 0.1]) and top("min")[1][0].tolist() == [0, 5, 6, 7]
    assert eq(top("min")[0][0], [0.5, 0.2, 0.2, -3.0])
    # the gate is on T(cos), before the boost: equal stays, one ulp above goes, -inf is no gate
    g = np.float32(0.2)
    assert top("sum", min_score=[g])[1][0].tolist() == [0, 5, 6, -1]
    assert top("sum", min_score=[np.nextafter(g, np.float32(1))])[1][0].tolist() == [0, -1, -1, -1]
    assert top("sum", min_score=[NEG_INF])[1][0].tolist() == [0, 5, 6, 7] and top("sum", min_score=[9.0])[1][0].tolist() == [-1] * 4
    assert top("replace", min_score=[0.25], boost=np.float32([100.0]))[1][0].tolist() == [0, -1, -1, -1]
    t_gate = np.float32(1) / (np.float32(2) - np.float32(0.2))
    assert top("replace", transform=1, min_score=[t_gate])[1][0].tolist() == [0, 5, 6, -1]
    # max / min are a compare and a select: with a = -0.0 and f = +0.0 neither compare holds and a is reported
    z = F.combine(np.float32([-0.0, 0.0]), np.float32([0.0, -0.0]), "max")
    assert np.signbit(z).tolist() == [True, False] and np.signbit(F.combine(np.float32([-0.0]), np.float32([0.0]), "min")).tolist() == [True]
    # avg is a rounded add, then a rounded product; sum after the boost is not an fma
    a, t, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)
    assert F.fused_scores(t, a, b, 0, "sum")[1] == np.float32(np.float32(a * t) + b) != np.float32(float(a) * float(t) + float(b))
    big = np.float32(3e38)
    assert np.isinf(F.combine(big, big, "avg"))                                 # (a + f) overflows before the halving
    live = np.array([1, 1, 1, 1, 1, 0, 1, 1], dtype=bool)
    assert F.search(cos, 3, f, mode="sum", live=live)[1][0].tolist() == [0, 6, 7]
    per_q = np.stack([f, np.where(np.arange(8) == 7, np.float32(5.0), f)])
    assert F.search(np.repeat(cos, 2, 0), 1, per_q, mode="replace")[1][:, 0].tolist() == [0, 7]


# ---------------------------------------------------------------------------------------------- the shim
def test_shim_scored_search(world):
    hip, idx, st, q = world
    cos = idx.cosines(q[None, :])[0]
    functions = [{"gauss": {"chunkDate": {"origin": "2023-06-01", "scale": "60d", "offset": "5d", "decay": 0.4}}},
                 {"filter": {"term": {"resourceType": "Condition"}}, "weight": 2.0}]
    where = {"bool": {"must_not": {"term": {"resourceType": "Encounter"}}}}
    idx.calls.clear()
    got = hip.semantic_search_scored(q, k=6, functions=functions, boost=1.5, where=where, patient_id="p1", min_score=0.55)
    assert [c["fn"] for c in idx.calls] == ["fn", "mask", "scored"]
    assert idx.calls[0]["score_mode"] == "multiply" and idx.calls[0]["n_filters"] == 1 and idx.calls[0]["functions"][1]["filter"] == 0
    assert idx.calls[2] == dict(fn="scored", k=6, boost=1.5, transform="opensearch", combine="multiply", min_score=0.55)
    docs = _docs()
    days = np.array([day(d["chunkDate"]) if "chunkDate" in d else F.ATTR_MISSING for d in docs])
    cond = np.array([d.get("resourceType") == "Condition" for d in docs])
    recs = [dict(kind="gauss", col=0, origin=float(day("2023-06-01")), scale=60.0, offset=5.0, decay=0.4), dict(kind="weight", weight=2.0, filter=0)]
    column = F.build_column(recs, {0: days}, 40, 1, "multiply", None, cond[None, :])[0]
    keep = np.array([d.get("resourceType") != "Encounter" and d["patientId"] == "p1" for d in docs])
    s, i = F.search(cos[None, :], 6, column, np.float32([1.5]), 1, "multiply", np.float32([0.55]), keep)
    want = [(int(r), float(v)) for v, r in zip(s[0], i[0]) if r >= 0]
    assert want and [(d["n"], v) for d, v in got] == want
    t = B.transform(cos, 1)
    assert all(t[n] >= np.float32(0.55) and keep[n] for n in ids(got))
    # the other modes reach the index as given; the cosine units pick the raw transform
    idx.calls.clear()
    hip.semantic_search_scored(q, k=3, functions=functions, score_mode="max", boost_mode="avg", max_boost=1.5, knn_score_mode="cosine")
    assert idx.calls[0]["score_mode"] == "max" and idx.calls[0]["max_boost"] == 1.5
    assert idx.calls[-1] == dict(fn="scored", k=3, boost=1.0, transform="raw", combine="avg", min_score=None)
    assert len(hip.semantic_search_scored(q, k=3)) == 3                           # no function: every chunk is worth 1.0
    plain = hip.semantic_search_scored(q, k=3, functions=[], boost_mode="multiply")
    assert ids(plain) == [0, 1, 2] and [v for _, v in plain] == [float(t[r]) for r in range(3)]
    # refusals are logged and answered with []
    assert hip.semantic_search_scored(q, k=5, functions=[{"gauss": {"chunkDate": {"scale": "12h"}}}]) == []
    assert hip.semantic_search_scored(q, k=5, functions=functions, boost=float("inf")) == []
    assert hip.semantic_search_scored(q, k=5, functions=functions, min_score=float("nan")) == []
    assert hip.semantic_search_scored(np.zeros(0, dtype=np.float32), k=5, functions=functions) == []
    assert hip.semantic_search_scored(q, k=5, functions=functions, patient_id="never-seen") == []


def test_shim_recent_search(world):
    hip, idx, st, q = world
    cos = idx.cosines(q[None, :])[0]
    t = B.transform(cos, 1)
    docs = _docs()
    gate = float(t[24])                                                           # rows 0 .. 24 pass
    dated = [n for n in range(25) if "chunkDate" in docs[n]]
    undated = [n for n in range(25) if "chunkDate" not in docs[n]]
    got = hip.semantic_search_recent(q, k=10, field="chunkDate", min_score=gate)
    assert ids(got) == sorted(dated, reverse=True)[:10]                           # the dates grow with n
    assert [v for _, v in got] == [float(day(docs[n]["chunkDate"])) for n in ids(got)]
    assert [c["fn"] for c in idx.calls[-3:]] == ["fn", "mask", "scored"] and idx.calls[-1]["combine"] == "replace"
    got = hip.semantic_search_recent(q, k=10, field="chunkDate", min_score=gate, order="asc")
    assert ids(got) == sorted(dated)[:10] and [v for _, v in got] == [float(day(docs[n]["chunkDate"])) for n in ids(got)]
    for order in ("desc", "asc"):
        got = hip.semantic_search_recent(q, k=40, field="chunkDate", min_score=gate, order=order, missing="_last")
        assert ids(got) == sorted(dated, reverse=order == "desc") + undated       # undated chunks after every dated one, by row
        assert all(np.isnan(v) for _, v in got[len(dated):]) and not any(np.isnan(v) for _, v in got[:len(dated)])
    assert ids(hip.semantic_search_recent(q, k=40, field="chunkDate", min_score=gate, missing="exclude")) == sorted(dated, reverse=True)
    paged = [n for n in range(40) if "pages" in docs[n] and docs[n]["patientId"] == "p2"]
    assert ids(hip.semantic_search_recent(q, k=4, field="pages", patient_id="p2")) == sorted(paged, reverse=True)[:4]   # an int field, no gate
    # values beyond +-2^24 are not exact in fp32: refused (logged, [])
    idx.cols[2][3] = (1 << 24) + 1
    assert hip.semantic_search_recent(q, k=4, field="pages") == []
    idx.cols[2][3] = 3
    assert hip.semantic_search_recent(q, k=4, field="resourceType") == []
    assert hip.semantic_search_recent(q, k=4, field="nope") == []
    assert hip.semantic_search_recent(q, k=4, field="chunkDate", order="up") == []
    assert hip.semantic_search_recent(q, k=4, field="chunkDate", missing="first") == []
    assert hip.semantic_search_recent(np.zeros(0, dtype=np.float32), k=4, field="chunkDate") == []


def test_index_without_a_scored_search_is_refused(monkeypatch):
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,chunkDate:date,pages:int")
    name = "fscore-cpu-plain"
    st = IndexState(name, StandInIndex())
    REGISTRY.put(st)
    try:
        indexer.add_documents(name, _docs(8), np.eye(8, DIM, dtype=np.float32))
        hip = indexer.HipIndexer(None, name)
        q = np.ones(DIM, dtype=np.float32)
        with pytest.raises(NotImplementedError):
            hip._scored(q, 3, [], "multiply", "multiply", None, None, 1.0, None, None, None, None, None)
        assert hip.semantic_search_scored(q, k=3) == [] and hip.semantic_search_recent(q, k=3, field="chunkDate") == []
    finally:
        REGISTRY.drop(name)


# ---------------------------------------------------------------------------------------------- the binding
def test_record_layout_and_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    for name, value in re.findall(r"^#define (RASS_(?:COMBINE|FN|MAX_SCORE)_[A-Z0-9_]+) (\d+)$", text, flags=re.M):
        assert getattr(_native, name) == int(value), name
    assert len(re.findall(r"^#define RASS_COMBINE_", text, flags=re.M)) == 6 == len(FlatIndex.COMBINE_MODES)
    assert len(re.findall(r"^#define RASS_FN_MOD_", text, flags=re.M)) == 10 == len(FlatIndex.FN_MODIFIERS)
    assert len(re.findall(r"^#define RASS_FN_SCORE_", text, flags=re.M)) == 6 == len(FlatIndex.FN_SCORE_MODES)
    body = re.search(r"typedef struct rass_score_fn \{(.*?)\} rass_score_fn_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|double)\s+([a-z_, ]+);", body):
        fields += [(n.strip(), ctypes.c_int32 if ctype == "int32_t" else ctypes.c_double) for n in names.split(",")]
    assert fields == list(_native.ScoreFn._fields_) and ctypes.sizeof(_native.ScoreFn) == 80
    for name in ("rass_index_search_scored", "rass_index_search_scored_device", "rass_index_fn_from_attr"):
        assert name in _native.SIGNATURES and re.search(r"\b%s\s*\(" % name, text)
    with pytest.raises(ValueError):
        FlatIndex._fn_records([{"kind": "decay"}])
    with pytest.raises(ValueError):
        FlatIndex._fn_records([{"kind": "weight", "colour": 1}])
    with pytest.raises(ValueError):
        FlatIndex._fn_records([{"kind": "field_value_factor", "modifier": "cube"}])
