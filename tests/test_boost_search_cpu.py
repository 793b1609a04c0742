"""The host-side layers of the boosted search, without a GPU: the numpy restatement (``boost_ref``) against a plain fp64
ranking, ``HipIndexer.semantic_search_boosted`` and ``RASS_HYBRID_EXACT`` over a stand-in index that answers the bonus
builders and ``search_boosted`` in numpy, the ``should`` compiler's encodings and refusals, the argument validation of
``FlatIndex.search_boosted`` (which refuses before any native call is made), and the new entry points' presence in the
header, the binding table and the built library."""
import datetime as dt
import os
import re
import subprocess
import types

import numpy as np
import pytest

import attr_ref as AR
import boost_ref as B
from rassengine_amd import _native, attrfilter, config, indexer
from rassengine_amd.docstore import REGISTRY, IndexState
from rassengine_amd.engine import FlatIndex

DIM = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("rass_index_search_boosted", "rass_index_search_boosted_device", "rass_index_bonus_scatter",
                    "rass_index_bonus_scatter_device", "rass_index_bonus_from_attr_clauses", "rass_index_bonus_mask")
NOW = dt.datetime(2024, 2, 29, 15, 30, tzinfo=dt.timezone.utc)
KINDS = {"resourceType": "keyword", "chunkDate": "date", "pages": "int", "patientId": "keyword", "doc_type": "keyword"}


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("mode", [0, 1])
def test_restatement_against_fp64_on_separated_scores(mode):
    """Well-separated fused scores (gaps far above an fp32 ulp): the fp32 restatement ranks as exact arithmetic does."""
    rng = np.random.default_rng(3 + mode)
    n, nq, k = 400, 6, 25
    cos = rng.permutation(np.linspace(-0.9, 0.9, n)).astype(np.float32)[None, :].repeat(nq, 0)
    cos = np.stack([rng.permutation(cos[q]) for q in range(nq)])
    bonus = (rng.integers(0, 8, size=(nq, n)) * 0.37).astype(np.float32)
    boost = np.array([2.0, 1.5, -1.0, 0.0, 0.3, 1.0], dtype=np.float32)
    live = rng.random(n) > 0.1
    s, i = B.search(cos, k, boost, bonus, mode, live)
    for q in range(nq):
        t = cos[q].astype(np.float64) if mode == 0 else 1.0 / (2.0 - cos[q].astype(np.float64))
        exact = float(boost[q]) * t + bonus[q].astype(np.float64)
        gaps = np.diff(np.sort(exact[live]))
        rows = np.flatnonzero(live)
        order = rows[np.lexsort((rows, -exact[rows]))][:k]
        if boost[q] != 0 and gaps.min() > 1e-5:
            assert np.array_equal(i[q], order), q
        else:       # ties (boost 0: the bonus has 8 levels): the order inside a level is by id, the levels are exact
            assert np.array_equal(np.sort(exact[i[q]])[::-1], np.sort(exact[order])[::-1]) or np.allclose(exact[i[q]], exact[order], atol=1e-6)
        assert np.allclose(s[q], exact[i[q]], rtol=0, atol=1e-6)


def test_restatement_rules():
    cos = np.array([[0.5, np.nan, 0.4, 0.3, -np.inf, 0.2, 0.2]], dtype=np.float32)
    bonus = np.array([0.0, 9.0, -np.inf, np.nan, 9.0, 0.25, 0.25], dtype=np.float32)
    s, i = B.search(cos, 5, None, bonus, 0)
    assert i[0].tolist() == [0, 5, 6, -1, -1] and s[0, :3].tolist() == [0.5] + [float(np.float32(0.2) + np.float32(0.25))] * 2
    assert B.search(cos, 3, np.zeros(1, np.float32), bonus, 1)[1][0].tolist() == [5, 6, 0]        # boost 0: bonus, then id
    assert B.search(cos, 3, None, bonus, 0, bonus_rows=5)[1][0].tolist() == [0, 5, 6]             # rows 5, 6 read 0
    assert B.search(cos, 2, None, bonus, 0, live=np.array([0, 1, 1, 1, 1, 1, 1], bool))[1][0].tolist() == [5, 6]
    # a product and a sum, each rounded: not an fma
    a, t, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)     # a * t = 1 + 2^-11 + 2^-24: a tie, rounded away
    assert B.fused_scores(t, a, b, 0) == np.float32(np.float32(a * t) + b) != np.float32(float(a) * float(t) + float(b))
    col = B.from_attr_clauses(np.zeros((2, 32), np.float32), {0: np.array([1, 5, B.ATTR_MISSING, 9])},
                              [(1, 0, 0, 5, 0), (0, 0, 5, 9, 0), (1, 0, 5, 5, 1), (0, 3, 0, 0, 1)], [1.0, 2.0, 4.0, 8.0], 4)
    assert col[:, :4].tolist() == [[8.0, 10.0, 8.0, 10.0], [5.0, 1.0, 4.0, 4.0]]


# ---------------------------------------------------------------------------------------------- the stand-in index
class StandInIndex:
    """``FlatIndex``'s write path, attribute columns, bonus builders and boosted search in numpy (``boost_ref``)."""

    def __init__(self):
        self.x = np.zeros((0, DIM), dtype=np.float32)
        self.tags = np.zeros(0, dtype=np.int32)
        self.cols = {}
        self.layout_epoch = 0
        self.calls = []

    rows = property(lambda self: self.x.shape[0])
    count = property(lambda self: int(np.count_nonzero(self.tags != -1)))

    def add(self, vecs, tags=None, normalize=True):
        v = np.asarray(vecs, dtype=np.float32)
        v = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
        first = self.rows
        self.x = np.concatenate([self.x, v.astype(np.float32)])
        self.tags = np.concatenate([self.tags, np.asarray(tags, dtype=np.int32)])
        for c in self.cols:
            self.cols[c] = np.concatenate([self.cols[c], np.full(len(v), B.ATTR_MISSING, dtype=np.int64)])
        return first

    def delete(self, row):
        self.tags[row] = -1

    def set_attr(self, col, first, values):
        self.cols.setdefault(col, np.full(self.rows, B.ATTR_MISSING, dtype=np.int64))[first:first + len(values)] = values

    def cosines(self, queries):
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        return (q @ self.x.T).astype(np.float32)

    def live(self, nq, q_filter, q_filter_mask):
        ok = np.tile(self.tags != -1, (nq, 1))
        for j in range(nq):
            if q_filter is not None and q_filter[j] >= 0:
                ok[j] &= ((self.tags & q_filter_mask[j]) if q_filter_mask is not None else self.tags) == q_filter[j]
        return ok

    def search(self, queries, k, q_filter=None, q_filter_mask=None):
        self.calls.append(dict(fn="search", k=k))
        s = self.cosines(queries)
        return B.search(s, k, None, None, 0, self.live(len(s), q_filter, q_filter_mask))

    def new_bonus(self, nq=None):
        stride = (self.rows + 63) // 32 * 32
        return np.zeros(stride if nq is None else (nq, stride), dtype=np.float32)

    def bonus_scatter(self, bonus, q_of, rows, values):
        self.calls.append(dict(fn="scatter", rows=list(rows), values=list(values)))
        assert len(set(rows)) == len(rows)
        return B.scatter(bonus, np.zeros(len(rows), dtype=np.int32) if q_of is None else q_of, rows, values)

    def bonus_from_attr_clauses(self, bonus, clauses, weights, op="replace"):
        self.calls.append(dict(fn="clauses", clauses=[tuple(int(x) for x in c) for c in clauses], weights=list(weights), op=op))
        assert len(clauses) <= 64
        cols = self.cols or {0: np.full(self.rows, B.ATTR_MISSING, dtype=np.int64)}
        return B.from_attr_clauses(bonus, cols, clauses, weights, self.rows, op)

    def bonus_mask(self, bonus, allow):
        self.calls.append(dict(fn="mask", allowed=int(np.count_nonzero(allow))))
        return B.mask(bonus, np.asarray(allow, dtype=bool)[None, :], self.rows)

    def search_boosted(self, queries, k, bonus, boost=None, transform="raw", bonus_rows=None, q_filter=None, q_filter_mask=None):
        self.calls.append(dict(fn="boosted", k=k, boost=boost, transform=transform))
        s = self.cosines(queries)
        bst = None if boost is None else np.full(len(s), boost, dtype=np.float32)
        return B.search(s, k, bst, bonus, transform, self.live(len(s), q_filter, q_filter_mask), bonus_rows)


def _docs(n=40):
    types_ = ["Observation", "Condition", "Encounter", "Procedure"]
    docs = []
    for i in range(n):
        d = {"doc_id": f"d{i}", "patientId": f"p{i % 4}", "doc_type": "note" if i % 5 == 0 else "unstructured", "n": i}
        if i % 7:
            d["resourceType"] = types_[i % 4]
        if i % 3:
            d["chunkDate"] = (dt.date(2023, 1, 1) + dt.timedelta(days=11 * i)).isoformat()
        if i % 6:
            d["pages"] = i
        docs.append(d)
    return docs


@pytest.fixture
def world(monkeypatch):
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,chunkDate:date,pages:int")
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "opensearch")
    name = "boost-cpu"
    idx = StandInIndex()
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
    # a `where` plan is evaluated in numpy here (attrfilter.run_plan needs the GPU)
    monkeypatch.setattr(attrfilter, "run_plan", lambda index, plan: AR.eval_plan(plan, index.cols, index.tags))
    yield indexer.HipIndexer(None, name), idx, st, q
    REGISTRY.drop(name)


def ids(hits):
    return [d["n"] for d, _ in hits]


def test_text_hits_duplicates_unknown_and_deleted_ids(world):
    hip, idx, st, q = world
    cos = idx.cosines(q[None, :])[0]
    idx.calls.clear()
    text = [("d30", 0.5), ({"doc_id": "d35", "junk": 1}, 0.25), ("d30", 0.125), ("nope", 9.0), (None, 9.0), ("d39", 1.0)]
    got = hip.semantic_search_boosted(q, k=5, boost=2.0, text_hits=text)
    assert [c["fn"] for c in idx.calls] == ["scatter", "boosted"]
    assert idx.calls[0]["rows"] == [30, 35, 39] and idx.calls[0]["values"] == [0.625, 0.25, 1.0]
    assert idx.calls[1] == dict(fn="boosted", k=5, boost=2.0, transform="opensearch")
    bonus = np.zeros(40, dtype=np.float32)
    bonus[[30, 35, 39]] = (0.625, 0.25, 1.0)
    fused = B.fused_scores(cos, 2.0, bonus, 1)
    order = np.lexsort((np.arange(40), -fused))[:5]
    assert ids(got) == order.tolist() and [s for _, s in got] == [float(fused[r]) for r in order]
    assert 39 in ids(got)           # a text hit at the bottom of the cosine order still got its cosine
    # an overwritten doc is found at its current row; a deleted one is ignored
    indexer.add_documents("boost-cpu", [dict(_docs()[39], n=39)], np.eye(1, DIM, 1, dtype=np.float32))
    assert st.doc_row["d39"] == 40 and st.row_doc[39] is None
    idx.calls.clear()
    hip.semantic_search_boosted(q, k=5, text_hits=[("d39", 1.0)], score_mode="cosine")
    assert idx.calls[0]["rows"] == [40] and idx.calls[1]["transform"] == "raw" and idx.calls[1]["boost"] == 1.0
    assert hip.semantic_search_boosted(np.zeros(0, dtype=np.float32), k=5, text_hits=text) == []
    assert hip.semantic_search_boosted(q, k=5, boost=float("nan")) == []           # logged, answered with []
    assert hip.semantic_search_boosted(q, k=5, patient_id="never-seen") == []


def test_should_compiler_encodings_and_refusals(world):
    hip, idx, st, q = world
    comp = lambda should: attrfilter.compile_should(should, st.attrs, st.patients, st.doc_types)
    code = st.attrs.dicts["resourceType"].lookup
    day = lambda s: (dt.date.fromisoformat(s) - dt.date(1970, 1, 1)).days
    got = comp([({"term": {"resourceType": "Condition"}}, 2.0),
                ({"terms": {"resourceType": ["Observation", "Encounter", "NeverIndexed", "Observation"]}}, -0.5),
                ({"range": {"chunkDate": {"gte": "now-1y", "lt": "2024-01-01"}}}, 0.5),
                ({"range": {"pages": {"gt": 3, "lte": 10}}}, 0.25),
                ({"exists": {"field": "pages"}}, 1)])
    assert got == [(0, code("Condition"), code("Condition"), 0, 2.0)] + \
        sorted([(0, code(v), code(v), 0, -0.5) for v in ("Observation", "Encounter")]) + \
        [(1, day("2023-02-28"), day("2023-12-31"), 0, 0.5), (2, 4, 10, 0, 0.25), (2, attrfilter.EXISTS[0], attrfilter.EXISTS[1], 0, 1.0)]
    assert comp([({"term": {"resourceType": "NeverIndexed"}}, 1.0)]) == [] and comp(None) == [] and comp([]) == []
    for bad in ([({"term": {"patientId": "p1"}}, 1.0)], [({"terms": {"doc_type": ["note"]}}, 1.0)], [({"exists": {"field": "patientId"}}, 1.0)],
                [({"bool": {"must": [{"term": {"pages": 3}}]}}, 1.0)], [({"match": {"resourceType": "x"}}, 1.0)],
                [({"term": {"color": "red"}}, 1.0)], [({"term": {"pages": 3}}, float("inf"))], [({"term": {"pages": 3}}, "1")],
                [{"term": {"pages": 3}}], [({"term": {"pages": 3}, "exists": {"field": "pages"}}, 1.0)]):
        with pytest.raises(ValueError):
            comp(bad)
    # through the shim: clauses in list order, added onto the text hits, then the where mask, then one search
    idx.calls.clear()
    should = [({"range": {"chunkDate": {"gte": "2023-06-01"}}}, 0.5), ({"term": {"resourceType": "Procedure"}}, -0.25)]
    where = {"range": {"pages": {"lte": 30}}}
    hits = hip.semantic_search_boosted(q, k=40, boost=1.5, text_hits=[("d33", 0.75)], should=should, where=where, patient_id="p1")
    assert [c["fn"] for c in idx.calls] == ["scatter", "clauses", "mask", "boosted"]
    assert idx.calls[1]["op"] == "add" and idx.calls[1]["weights"] == [0.5, -0.25] and [c[0] for c in idx.calls[1]["clauses"]] == [0, 0]
    docs = _docs()
    cos = idx.cosines(q[None, :])[0]
    bonus = np.zeros(40, dtype=np.float32)
    bonus[33] = 0.75
    for leaf, wgt in should:
        hit = np.array([AR.doc_matches(leaf, d, KINDS, NOW) for d in docs])
        bonus = np.where(hit, (bonus + np.float32(wgt)).astype(np.float32), bonus)
    keep = np.array([AR.doc_matches(where, d, KINDS, NOW) and d["patientId"] == "p1" for d in docs])
    fused = B.fused_scores(cos, 1.5, bonus, 1)
    rows = np.flatnonzero(keep)
    order = rows[np.lexsort((rows, -fused[rows]))]
    assert ids(hits) == order.tolist() and [s for _, s in hits] == [float(fused[r]) for r in order]
    # more than 64 clauses go in chunks, every one an add
    idx.calls.clear()
    hip.semantic_search_boosted(q, k=3, should=[({"term": {"pages": i}}, 0.01) for i in range(70)])
    assert [(c["fn"], len(c.get("clauses", []))) for c in idx.calls] == [("clauses", 64), ("clauses", 6), ("boosted", 0)]
    assert hip.semantic_search_boosted(q, k=3, should=[({"term": {"patientId": "p1"}}, 1.0)]) == []       # refused, logged


class TextEngine:
    def __init__(self, hits):
        self.hits, self.calls = hits, []

    def hybrid_search(self, query, query_emb, k=3, filter_clause=None, patient_id=None):
        self.calls.append(k)
        return self.hits[:k]

    hybrid_structured_search = multi_intent_search = hybrid_search


def test_hybrid_exact_switch(world, monkeypatch):
    hip, idx, st, q = world
    docs = _docs()
    text = TextEngine([(dict(docs[38]), 0.2), (dict(docs[2]), 0.1), ({"doc_id": "text-only"}, 0.05)])
    monkeypatch.setattr(indexer.HipIndexer, "_text_engine", lambda self: text)
    # the switch off: the calls and the answer of the over-fetch path, unchanged
    assert config.RASS_HYBRID_EXACT is False
    idx.calls.clear()
    old = hip.hybrid_search("x", q, k=3)
    assert [c["fn"] for c in idx.calls] == ["search"] and idx.calls[0]["k"] == 3 * indexer.FUSION_OVERFETCH and text.calls == [12]
    cos = idx.cosines(q[None, :])[0]
    assert ids(old) == [2, 0, 1] and old[0][1] == pytest.approx(2.0 / (2.0 - float(cos[2])) + 0.1)
    assert 38 not in ids(hip.hybrid_search("x", q, k=12))[:11]      # d38 sits outside the 48-deep knn list's top: text score alone
    # the switch on: the same text list, through the boosted scan
    monkeypatch.setattr(config, "RASS_HYBRID_EXACT", True)
    idx.calls.clear()
    text.calls.clear()
    new = hip.hybrid_search("x", q, k=3)
    assert text.calls == [12] and [c["fn"] for c in idx.calls] == ["scatter", "boosted"]
    assert idx.calls[0]["rows"] == [38, 2] and idx.calls[1] == dict(fn="boosted", k=3, boost=2.0, transform="opensearch")
    bonus = np.zeros(40, dtype=np.float32)
    bonus[[38, 2]] = (0.2, 0.1)
    fused = B.fused_scores(cos, 2.0, bonus, 1)
    order = np.lexsort((np.arange(40), -fused))[:3]
    assert ids(new) == order.tolist() and [s for _, s in new] == [float(fused[r]) for r in order]
    idx.calls.clear()
    hip.multi_intent_search("x", q, k=3)
    assert idx.calls[-1]["fn"] == "boosted" and idx.calls[-1]["boost"] == 1.5
    assert hip.hybrid_structured_search("x", q, k=3) == []       # no chunk of doc_type "structured" here: as with the switch off


def test_an_index_without_the_method_answers_empty(world, monkeypatch):
    hip, idx, st, q = world
    monkeypatch.setattr(StandInIndex, "search_boosted", property(), raising=True)      # hasattr() is False
    assert hip.semantic_search_boosted(q, k=3) == []
    with pytest.raises(NotImplementedError, match="boosted search"):
        hip._boosted(q, 3, 1.0, None, None, None, None, None, None, None)


# ---------------------------------------------------------------------------------------------- FlatIndex validation
def test_flat_index_search_boosted_validates_before_the_native_call():
    class Lib:
        dtype, stride = 0, 128

        def rass_index_dim(self, h):
            return DIM

        def rass_index_dtype(self, h):
            return self.dtype

        def rass_index_row_stride(self, h):
            return self.stride

        def rass_index_search_boosted(self, *a):
            raise AssertionError("the native entry point was reached")

    lib = Lib()
    idx = FlatIndex(types.SimpleNamespace(_L=lib, device=0), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, k=5, bonus=np.zeros(64, dtype=np.float32))
    bad = [dict(queries=np.zeros(DIM)), dict(queries=np.zeros((3, DIM + 1))), dict(k=0), dict(k=4097), dict(k=-3),
           dict(bonus=np.zeros((2, 64), dtype=np.float32)), dict(bonus=np.zeros((3, 2, 64), dtype=np.float32)),
           dict(bonus=np.zeros(50, dtype=np.float32)), dict(bonus=[0.0] * 64),
           dict(queries=np.zeros((4097, DIM), dtype=np.float32)),
           dict(boost=[1.0, 2.0]), dict(boost=[1.0, np.inf, 1.0]), dict(boost=np.nan), dict(transform="cosine"),
           dict(bonus_rows=65), dict(bonus_rows=-1),
           dict(q_filter=np.zeros(2, dtype=np.int32)), dict(q_filter_mask=np.zeros(3, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_boosted(**dict(good, **kw))
    for attr, value in (("dtype", 1), ("stride", 1280)):     # a bf16 index, a wide-row index
        setattr(lib, attr, value)
        with pytest.raises(ValueError, match="fp32 index with dim <= 1024"):
            idx.search_boosted(**good)
        setattr(lib, attr, getattr(Lib, attr))
    s, i = idx.search_boosted(np.zeros((0, DIM), dtype=np.float32), 5, np.zeros(64, dtype=np.float32))      # no query, no call
    assert s.shape == (0, 5) and i.shape == (0, 5)


# ---------------------------------------------------------------------------------------------- header / table / library
def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in _native.SIGNATURES, f"{name} is not in the binding table"
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), f"{name}: header and binding table disagree"
    assert re.search(r"rass_abi_version", header) and "RASS_BOOST_OPENSEARCH 1" in header and "RASS_BONUS_ADD 1" in header
    assert os.path.exists(_native.LIB_PATH), "librass_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [name for name in NEW_ENTRY_POINTS if name not in exported]
    assert not missing, f"not exported by the built library: {missing}"
    assert _native.lib().rass_abi_version() == 1
