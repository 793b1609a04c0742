"""The host-side layers of the attribute filter, without a GPU: the numpy restatement the GPU tests compare against
(``attr_ref``) held to hand-written answers; the filter compiler (``attrfilter.compile_filter``) held to a plain Python
evaluator over the doc dicts on random nested ``bool`` trees; the date / int / keyword encodings of ``docstore.AttrSchema``;
and the manifest with and without a schema.  Everything is integer or bit-exact: no tolerance anywhere."""
import datetime as dt
import json
import os

import numpy as np
import pytest

import attr_ref as R
from rassengine_amd import _native, attrfilter, config
from rassengine_amd.docstore import (ATTR_MISSING, TAG_DOCTYPE_SHIFT, AttrSchema, IndexState, date_bound_days, date_days)

NOW = dt.datetime(2024, 2, 29, 15, 30, tzinfo=dt.timezone.utc)
SPEC = "resourceType:keyword,file_type:keyword,chunkDate:date,pages:int"
KINDS = {"resourceType": "keyword", "file_type": "keyword", "chunkDate": "date", "pages": "int", "patientId": "keyword",
         "doc_type": "keyword"}


def day(s):
    return (dt.date.fromisoformat(s) - dt.date(1970, 1, 1)).days


# ------------------------------------------------------------------------------------------------ constants and the reference
def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rass_engine.h")).read()
    for name, value in (("RASS_MAX_ATTRS", 8), ("RASS_MAX_ATTR_CLAUSES", 64), ("RASS_ATTR_ALL", 0), ("RASS_ATTR_ANY", 1),
                        ("RASS_ATTR_REPLACE", 0), ("RASS_ATTR_AND", 1), ("RASS_ATTR_OR", 2)):
        assert f"#define {name} {value}" in " ".join(text.split()), name
        assert getattr(_native, name) == value
    assert "#define RASS_ATTR_MISSING INT32_MIN" in " ".join(text.split())
    assert _native.RASS_ATTR_MISSING == R.MISSING == ATTR_MISSING == -2 ** 31
    for fn in ("rass_index_set_attr", "rass_index_get_attr", "rass_index_attr_mask", "rass_index_device_attr",
               "rass_index_allow_from_attr_clauses"):
        assert fn in _native.SIGNATURES


def test_clause_semantics_missing_negate_and_empty_range():
    v = np.array([R.MISSING, R.INT_MIN, -1, 0, 5, R.INT_MAX], dtype=np.int32)
    assert R.holds(v, 0, 5, 0).tolist() == [False, False, False, True, True, False]
    assert R.holds(v, 0, 5, 1).tolist() == [True, True, True, False, False, True]          # a missing value passes under negate
    assert R.holds(v, 5, 0, 0).tolist() == [False] * 6                                      # lo > hi holds for nothing
    assert R.holds(v, 5, 0, 1).tolist() == [True] * 6
    assert R.holds(v, R.INT_MIN, R.INT_MAX, 0).tolist() == [False, True, True, True, True, True]   # exists
    assert R.holds(v, 5, 5, 0).tolist() == [False, False, False, False, True, False]        # equality
    assert R.holds(v, R.MISSING, R.INT_MAX, 0)[0] == False                                  # noqa: E712  MISSING is never a value


def test_modes_combines_tombstones_and_tails():
    cols = {0: np.array([1, 2, 3, R.MISSING, 5], dtype=np.int32), 3: np.array([9, 9, 0, 0, 9], dtype=np.int32)}
    tags = np.array([0, 0, 0, 0, -1], dtype=np.int32)                       # row 4 is a tombstone
    cl = [(0, 0, 2, 5, 0), (0, 3, 9, 9, 0), (1, 0, 1, 1, 0), (1, 7, 0, 0, 0)]  # column 7 was never set
    assert R.allowed(cols, tags, cl, 3, R.ALL).tolist() == [[False, True, False, False, False], [False] * 5, [True] * 4 + [False]]
    assert R.allowed(cols, tags, cl, 3, R.ANY).tolist() == [[True, True, True, False, False], [True] + [False] * 4, [False] * 5]
    prior = np.array([[0xFFFFFFFF, 0xFFFFFFFF]] * 3, dtype=np.uint32)      # ones in the tail bits and a surplus word
    rep = R.build(cols, tags, cl, 3, 3, R.ALL, R.REPLACE, prior)
    assert rep.tolist() == [[0b00010, 0], [0, 0], [0b01111, 0]]
    assert R.build(cols, tags, cl, 3, 3, R.ALL, R.AND, prior).tolist() == rep.tolist()      # tails come out 0
    orr = R.build(cols, tags, cl, 3, 3, R.ALL, R.OR, np.array([[0xFFFFFF00, 7]] * 3, dtype=np.uint32))
    assert orr.tolist() == [[0xFFFFFF02, 7], [0xFFFFFF00, 7], [0xFFFFFF0F, 7]]              # ... and stay under OR
    assert np.array_equal(R.unpack(R.pack(np.eye(3, 40, dtype=bool), 2), 40), np.eye(3, 40, dtype=bool))


# ------------------------------------------------------------------------------------------------ encodings
def test_date_encoding_three_forms_offsets_and_date_math():
    assert date_days("1970-01-01") == 0 and date_days("2024-03-01") == day("2024-03-01")
    assert date_days("2024-03-01T23:59:59") == day("2024-03-01")                    # no offset: UTC
    assert date_days("2024-03-01T00:00:00Z") == day("2024-03-01")
    assert date_days("2024-03-01T01:00:00+05:30") == day("2024-02-29")              # crosses the UTC day backwards
    assert date_days("2024-03-01T22:00:00-03:00") == day("2024-03-02")              # ... and forwards
    assert date_days("1969-12-31T23:00:00Z") == -1                                  # floored, not truncated
    assert date_days(1709251200000) == day("2024-03-01") and date_days(1709251199999) == day("2024-02-29")
    assert date_days(-1) == -1
    for bad in ("yesterday", "2024-13-01", "", None, 3.5, True, "20240301"):
        assert date_days(bad) is None, bad
    assert date_bound_days("now", NOW) == day("2024-02-29")
    assert date_bound_days("now-1y", NOW) == day("2023-02-28")                      # the day clamped to the month
    assert date_bound_days("now-1M", NOW) == day("2024-01-29") and date_bound_days("now-12M", NOW) == day("2023-02-28")
    assert date_bound_days("now-3d", NOW) == day("2024-02-26") and date_bound_days("now-2w", NOW) == day("2024-02-15")
    assert date_bound_days("now+1d", NOW) == day("2024-03-01")
    assert date_bound_days("2024-01-01", NOW) == day("2024-01-01") and date_bound_days("now-1h", NOW) is None
    for expr in ("now", "now-1y", "now-1M", "now-3d", "now-2w"):
        assert date_bound_days(expr, NOW) == R.bound_day(expr, NOW)


def test_schema_encodes_keywords_ints_and_dates(caplog):
    s = AttrSchema.parse(SPEC)
    assert s and len(s) == 4 and s.column("chunkDate") == (2, "date") and s.column("nope") is None
    docs = [{"resourceType": "Observation", "file_type": "pdf", "chunkDate": "2024-03-01T01:00:00+05:30", "pages": 7},
            {"resourceType": "Condition", "chunkDate": 1709251200000, "pages": -2 ** 31 + 1},
            {"resourceType": "Observation", "file_type": None, "chunkDate": "soon", "pages": 2 ** 31 - 1},
            {"resourceType": "", "chunkDate": "also soon"}]
    with caplog.at_level("WARNING", logger="rassengine_amd"):
        cols = s.encode_docs(docs)
    assert cols.dtype == np.int32 and cols.shape == (4, 4)
    assert cols[0].tolist() == [1, 2, 1, R.MISSING] and cols[1].tolist() == [1, R.MISSING, R.MISSING, R.MISSING]
    assert cols[2].tolist() == [day("2024-02-29"), day("2024-03-01"), R.MISSING, R.MISSING]
    assert cols[3].tolist() == [7, -2 ** 31 + 1, 2 ** 31 - 1, R.MISSING]
    assert sum("chunkDate" in r.message for r in caplog.records) == 1               # logged once per field
    assert s.dicts["resourceType"].names() == ["Observation", "Condition"]
    again = AttrSchema.from_meta(json.loads(json.dumps(s.to_meta())))
    assert again == s and again.dicts["resourceType"].lookup("Condition") == 2 and again.dicts["file_type"].names() == ["pdf"]


@pytest.mark.parametrize("value", [2 ** 31, -2 ** 31, 10 ** 12])
def test_int_outside_int32_raises(value):
    s = AttrSchema.parse("pages:int")
    with pytest.raises(OverflowError):
        s.encode_docs([{"pages": value}])       # -2**31 is RASS_ATTR_MISSING: not a value
    with pytest.raises(ValueError):
        s.encode_docs([{"pages": "7"}])


def test_schema_refuses_bad_specs():
    assert not AttrSchema.parse("") and not AttrSchema.parse(None) and len(AttrSchema()) == 0
    for bad in ("a", "a:float", "a:int,a:date", ",".join(f"f{i}:int" for i in range(9)), "patientId:keyword"):
        with pytest.raises(ValueError):
            AttrSchema.parse(bad)


# ------------------------------------------------------------------------------------------------ the compiler
def make_docs(rng, n=200):
    types, files, pats = ["Observation", "Condition", "Encounter", "Procedure"], ["pdf", "txt", "json"], [f"p{i}" for i in range(6)]
    docs = []
    for i in range(n):
        d = {"doc_id": f"d{i}", "doc_type": "unstructured" if i % 7 else "note"}
        if rng.random() < 0.9:
            d["resourceType"] = types[rng.integers(len(types))]
        if rng.random() < 0.8:
            d["file_type"] = files[rng.integers(len(files))]
        if rng.random() < 0.85:
            stamp = dt.datetime(2022, 1, 1, tzinfo=dt.timezone.utc) + dt.timedelta(hours=int(rng.integers(0, 24 * 900)))
            form = rng.integers(3)
            d["chunkDate"] = stamp.date().isoformat() if form == 0 else int(stamp.timestamp() * 1000) if form == 1 else \
                stamp.astimezone(dt.timezone(dt.timedelta(hours=int(rng.integers(-11, 12))))).isoformat()
        if rng.random() < 0.9:
            d["pages"] = int(rng.integers(-5, 40))
        if rng.random() < 0.9:
            d["patientId"] = pats[rng.integers(len(pats))]
        docs.append(d)
    return docs


def random_leaf(rng):
    kind = rng.integers(9)
    if kind == 0:
        return {"term": {"resourceType": ["Observation", "Condition", "NeverIndexed"][rng.integers(3)]}}
    if kind == 1:
        return {"terms": {"file_type": [["pdf", "txt"], ["json", "NeverIndexed"], ["NeverIndexed"], []][rng.integers(4)]}}
    if kind == 2:
        ops = {}
        if rng.random() < 0.7:
            ops[["gte", "gt"][rng.integers(2)]] = ["2022-06-01", "now-1y", "2023-03-15T12:00:00+02:00", 1672531200000][rng.integers(4)]
        if rng.random() < 0.7:
            ops[["lte", "lt"][rng.integers(2)]] = ["now", "2023-12-31", "now-6M", "2021-01-01"][rng.integers(4)]
        return {"range": {"chunkDate": ops}}
    if kind == 3:
        return {"range": {"pages": {["gte", "gt"][rng.integers(2)]: int(rng.integers(-6, 20)),
                                    ["lte", "lt"][rng.integers(2)]: int(rng.integers(0, 41))}}}
    if kind == 4:
        return {"exists": {"field": ["resourceType", "chunkDate", "pages", "patientId", "file_type"][rng.integers(5)]}}
    if kind == 5:
        return {"term": {"patientId": ["p1", "p4", "nobody"][rng.integers(3)]}}
    if kind == 6:
        return {"terms": {"patientId": [["p0", "p2", "p5"], ["nobody"]][rng.integers(2)]}}
    if kind == 7:
        return {"term": {"doc_type": ["note", "unstructured", "structured"][rng.integers(3)]}}
    return {"term": {"pages": int(rng.integers(-5, 40))}}


def random_tree(rng, depth):
    if depth == 0 or rng.random() < 0.3:
        return random_leaf(rng)
    body = {}
    for key in ("must", "filter", "should", "must_not"):
        if rng.random() < 0.45:
            subs = [random_tree(rng, depth - 1) for _ in range(int(rng.integers(1, 4)))]
            body[key] = subs[0] if len(subs) == 1 and rng.random() < 0.5 else subs
    return {"bool": body}


class World:
    def __init__(self, seed=5):
        rng = np.random.default_rng(seed)
        self.docs = make_docs(rng)
        self.st = IndexState("attr-cpu", index=None)
        self.st.attrs = AttrSchema.parse(SPEC)
        self.tags = np.array([self.st.tag_of(d) for d in self.docs], dtype=np.int32)
        enc = self.st.attrs.encode_docs(self.docs)
        self.dead = [31, 32, len(self.docs) - 1]
        self.tags[self.dead] = -1
        self.cols = {c: enc[c] for c in range(enc.shape[0])}

    def plan(self, where):
        return attrfilter.compile_filter(where, self.st.attrs, self.st.patients, self.st.doc_types, now=NOW)

    def want(self, where):
        return np.array([self.tags[i] != -1 and R.doc_matches(where, d, KINDS, NOW) for i, d in enumerate(self.docs)])


@pytest.fixture(scope="module")
def world():
    return World()


def test_compiler_equals_the_doc_evaluator_on_random_trees(world):
    rng = np.random.default_rng(99)
    shapes = set()
    for i in range(300):
        where = random_tree(rng, depth=3)
        plan = world.plan(where)
        got = R.eval_plan(plan, world.cols, world.tags)
        assert np.array_equal(got, world.want(where)), (i, where, plan)
        shapes.add(plan[0])
    assert shapes >= {"all", "any", "and", "or", "tags"}        # every node kind was exercised


def test_compiler_folds_leaves_into_single_calls(world):
    plan = world.plan({"bool": {"must": [{"term": {"resourceType": "Observation"}}, {"range": {"chunkDate": {"gte": "now-1y", "lt": "now"}}}],
                                "must_not": {"term": {"file_type": "pdf"}}, "filter": {"exists": {"field": "pages"}}}})
    assert plan[0] == "all" and len(plan[1]) == 4 and attrfilter.plan_calls(plan) == 1
    pdf = world.st.attrs.dicts["file_type"].lookup("pdf")
    assert (2, day("2023-02-28"), day("2024-02-28"), 0) in plan[1] and (1, pdf, pdf, 1) in plan[1]
    assert (3, R.INT_MIN, R.INT_MAX, 0) in plan[1]
    plan = world.plan({"bool": {"should": [{"term": {"resourceType": "Condition"}}, {"term": {"pages": 3}}]}})
    assert plan[0] == "any" and len(plan[1]) == 2
    plan = world.plan({"terms": {"pages": list(range(100))}})
    assert plan[0] == "any" and len(plan[1]) == 100 and attrfilter.plan_calls(plan) == 2      # chunked with OR
    assert world.plan({"term": {"resourceType": "NeverIndexed"}}) == ("any", [])             # matches nothing
    assert world.plan({"bool": {}}) == ("all", [])
    plan = world.plan({"term": {"patientId": "p1"}})
    assert plan == ("tags", [world.st.patients.lookup("p1")], 0x00FFFFFF, False)
    plan = world.plan({"term": {"doc_type": "note"}})
    assert plan == ("tags", [world.st.doc_types.lookup("note") << TAG_DOCTYPE_SHIFT], 0x7F000000, False)
    gt = world.plan({"range": {"chunkDate": {"gt": "2023-01-01", "lte": "2023-01-31"}}})
    assert gt == ("all", [(2, day("2023-01-02"), day("2023-01-31"), 0)])                      # gt = the next day


@pytest.mark.parametrize("where,word", [
    ({"term": {"color": "red"}}, "color"), ({"match": {"resourceType": "x"}}, "match"),
    ({"match_phrase": {"unstructuredText": "x"}}, "match_phrase"), ({"range": {"resourceType": {"gte": "a"}}}, "resourceType"),
    ({"range": {"patientId": {"gte": 1}}}, "patientId"), ({"bool": {"must": [{"wildcard": {"file_type": "p*"}}]}}, "wildcard"),
    ({"range": {"chunkDate": {"gte": "next tuesday"}}}, "next tuesday"), ({"bool": {"should": [], "minimum_should_match": 2}}, "minimum_should_match"),
    ({"range": {"pages": {"gte": "3"}}}, "pages"), ({"exists": {"field": "color"}}, "color")])
def test_compiler_names_what_it_refuses(world, where, word):
    with pytest.raises(ValueError, match=word):
        world.plan(where)


# ------------------------------------------------------------------------------------------------ the manifest
class FileIndex:
    """What ``IndexState.save`` / ``load`` need of an index, with a dummy vector file."""
    rows, count = 3, 3

    def save(self, path):
        open(path, "wb").write(b"vectors")


def _state(monkeypatch, spec):
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", spec)
    st = IndexState("attr-meta", FileIndex())
    st.row_doc = [{"doc_id": f"d{i}", "resourceType": "Observation" if i else "Condition"} for i in range(3)]
    st.doc_row = {d["doc_id"]: i for i, d in enumerate(st.row_doc)}
    if st.attrs:
        st.attrs.encode_docs(st.row_doc)
    return st


def test_manifest_with_and_without_a_schema(tmp_path, monkeypatch):
    plain = _state(monkeypatch, "")
    assert not plain.attrs
    plain.save(str(tmp_path / "plain"))
    keys = set(json.load(open(tmp_path / "plain.meta.json")))
    assert keys == {"version", "name", "generation", "vectors", "rows", "live", "row_doc", "structured", "patients", "doc_types"}
    with_schema = _state(monkeypatch, "resourceType:keyword,chunkDate:date")
    with_schema.save(str(tmp_path / "typed"))
    meta = json.load(open(tmp_path / "typed.meta.json"))
    assert set(meta) == keys | {"attrs"} and meta["version"] == 2
    assert meta["attrs"] == {"fields": [["resourceType", "keyword"], ["chunkDate", "date"]],
                             "keywords": {"resourceType": ["Condition", "Observation"]}}
    # a manifest without the key loads as no schema, whatever is configured; one with it keeps the saved schema
    loaded = IndexState.load("attr-meta", str(tmp_path / "plain"), lambda name, path: FileIndex())
    assert not loaded.attrs
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "pages:int")
    loaded = IndexState.load("attr-meta", str(tmp_path / "typed"), lambda name, path: FileIndex())
    assert loaded.attrs.fields == [("resourceType", "keyword"), ("chunkDate", "date")]
    assert loaded.attrs.dicts["resourceType"].lookup("Observation") == 2
