"""The host-side layers of grouping and aggregating by an attribute field, without a GPU: ``HipIndexer.semantic_search_collapsed``
/ ``semantic_aggregate`` over a stand-in index that answers the key-column calls in numpy (``tests/groupkeys_ref.py``), the
calendar edges of a ``date_histogram``, and the argument validation of ``FlatIndex``'s key-column methods (which refuse
before any native call is made)."""
import datetime as dt
import types

import numpy as np
import pytest

import groupkeys_ref as R
from rassengine_amd import attrfilter, indexer
from rassengine_amd.docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_PATIENT_MASK, AttrSchema, IndexState
from rassengine_amd.engine import FlatIndex

DIM = 16
SCHEMA = "resourceType:keyword,code:int,chunkDate:date"
EMPTY = {"buckets": [], "sum_other_doc_count": 0, "cardinality": 0, "total": 0}


def day(s):
    return (dt.date.fromisoformat(s) - dt.date(1970, 1, 1)).days


class PlainIndex:
    """``FlatIndex``'s write path in numpy and the tag-keyed searches: an index object WITHOUT the key-column methods."""

    def __init__(self):
        self.x = np.zeros((0, DIM), dtype=np.float32)
        self.tags = np.zeros(0, dtype=np.int32)
        self.attr = np.zeros((8, 0), dtype=np.int64)
        self.layout_epoch = 0
        self.dim = DIM
        self.calls = []
        self.compact_during_next = 0

    rows = property(lambda self: self.x.shape[0])
    count = property(lambda self: int(np.count_nonzero(self.tags != -1)))

    def add(self, vecs, tags=None, normalize=True):
        v = np.asarray(vecs, dtype=np.float32)
        v = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
        first = self.rows
        self.x = np.concatenate([self.x, v.astype(np.float32)])
        self.tags = np.concatenate([self.tags, np.asarray(tags, dtype=np.int32)])
        self.attr = np.concatenate([self.attr, np.full((8, len(v)), R.MISSING, dtype=np.int64)], axis=1)
        return first

    def set_attr(self, col, first_row, values):
        self.attr[col, first_row:first_row + len(values)] = values

    def delete(self, row):
        self.tags[row] = -1

    def _scores(self, queries):
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        return (q @ self.x.T).astype(np.float32)

    def _note(self, name, **kw):
        self.calls.append(dict(kw, fn=name))
        if self.compact_during_next > 0:
            self.compact_during_next -= 1
            self.layout_epoch += 1

    def _tag_keys(self, group_mask):
        return (self.tags.astype(np.int64) & group_mask) >> ((group_mask & -group_mask).bit_length() - 1)

    def search_grouped(self, queries, k, group_mask, n_groups, q_filter=None, q_filter_mask=None):
        self._note("search_grouped", k=k, group_mask=group_mask, n_groups=n_groups)
        return R.expect_grouped(self._scores(queries), self.tags, self._tag_keys(group_mask), n_groups, k, None, q_filter, q_filter_mask)[:4]

    def search_counts(self, queries, min_score, size, group_mask, n_groups, q_filter=None, q_filter_mask=None):
        self._note("search_counts", size=size, group_mask=group_mask, n_groups=n_groups)
        return R.expect_counts(self._scores(queries), self.tags, self._tag_keys(group_mask), n_groups, size, min_score, None, q_filter,
                               q_filter_mask)[:6]


class StandInIndex(PlainIndex):
    """... plus the key-column methods and the one bitmap builder a range / term filter compiles to, in numpy.  A key column
    is an int64 array, a bitmap a bool array."""

    def group_keys_from_attr(self, col, base=0, missing=-1, edges=None):
        self._note("group_keys_from_attr", col=col, base=base, missing=missing, edges=None if edges is None else list(edges))
        if edges is None:
            return R.keys_from_attr(self.attr[col], base, missing, self.rows + 5)
        return R.keys_from_edges(self.attr[col], edges, missing, self.rows + 5)

    def group_keys_from_tag(self, mask):
        self._note("group_keys_from_tag", mask=mask)
        return np.where(self.tags == -1, -1, self._tag_keys(mask))

    def attr_minmax(self, col):
        self._note("attr_minmax", col=col)
        return R.attr_minmax(self.attr[col], self.tags)

    def allow_from_attr_clauses(self, clauses, nq=1, shared=False, mode="all", combine="replace", allow=None):
        self._note("allow_from_attr_clauses")
        assert shared and nq == 1 and combine == "replace" and allow is None and mode == "all"
        ok = self.tags != -1
        for _, col, lo, hi, neg in np.asarray(clauses).reshape(-1, 5):
            v = self.attr[col]
            ok &= ((v != R.MISSING) & (lo <= v) & (v <= hi)) != bool(neg)
        return ok

    def search_grouped_by_keys(self, queries, k, keys, n_groups, allow=None, q_filter=None, q_filter_mask=None):
        self._note("search_grouped_by_keys", k=k, keys=np.array(keys), n_groups=n_groups, allow=allow)
        keys = np.concatenate([keys, np.full(max(0, self.rows - len(keys)), -1)])
        got = R.expect_grouped(self._scores(queries), self.tags, keys, n_groups, k, allow, q_filter, q_filter_mask)
        assert got[4] == 0, "a matching row's group key is >= n_groups"
        return got[:4]

    def search_counts_by_keys(self, queries, min_score, size, keys, n_groups, allow=None, q_filter=None, q_filter_mask=None):
        self._note("search_counts_by_keys", size=size, keys=np.array(keys), n_groups=n_groups, allow=allow)
        keys = np.concatenate([keys, np.full(max(0, self.rows - len(keys)), -1)])
        got = R.expect_counts(self._scores(queries), self.tags, keys, n_groups, size, min_score, allow, q_filter, q_filter_mask)
        assert got[6] == 0, "a hit's group key is >= n_groups"
        return got[:6]


TYPES = ["Condition", "Observation", None, "Procedure"]


def _fill(name, idx, schema=SCHEMA):
    """40 chunks whose cosine to the query e0 falls with n.  resourceType cycles through TYPES (every n % 4 == 2 has none),
    code = n // 10 (missing for n % 7 == 0), chunkDate = 2024-01-25 + 3 n days (missing for n % 9 == 0)."""
    st = IndexState(name, idx)
    st.attrs = AttrSchema.parse(schema)
    REGISTRY.put(st)
    cos = np.linspace(0.99, 0.02, 40)
    emb = np.zeros((40, DIM), dtype=np.float32)
    emb[:, 0] = cos
    emb[:, 1] = np.sqrt(1.0 - cos ** 2)
    docs = []
    for n in range(40):
        d = {"doc_id": f"d{n}", "patientId": ["alice", "bob", "carol"][n % 3], "doc_type": "note" if n % 4 == 3 else "unstructured", "n": n}
        if TYPES[n % 4] is not None:
            d["resourceType"] = TYPES[n % 4]
        if n % 7:
            d["code"] = n // 10
        if n % 9:
            d["chunkDate"] = (dt.date(2024, 1, 25) + dt.timedelta(days=3 * n)).isoformat()
        docs.append(d)
    indexer.add_documents(name, docs, emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    return q, cos, docs


@pytest.fixture
def world():
    name = "gba-cpu"
    idx = StandInIndex()
    q, cos, docs = _fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, docs
    REGISTRY.drop(name)


def _shape(agg):
    return [(b["key"], b["doc_count"], b["top_hit"][0]["n"]) for b in agg["buckets"]]


def test_tag_fields_keep_the_tag_path_call_for_call(world):
    """The routing pin: patientId / doc_type without where= make the calls they made before attribute fields could group.
    (By its nature this one test also passes on the code before the feature; every other test of the file needs it.)"""
    hip, idx, q, docs = world
    hits, total = hip.semantic_search_collapsed(q, k=5)
    assert [h[0]["n"] for h in hits] == [0, 1, 2] and total == 3
    assert idx.calls[-1] == dict(fn="search_grouped", k=5, group_mask=TAG_PATIENT_MASK, n_groups=4)
    hip.semantic_search_collapsed(q, k=5, collapse="doc_type")
    assert idx.calls[-1] == dict(fn="search_grouped", k=5, group_mask=TAG_DOCTYPE_MASK, n_groups=3)
    agg = hip.semantic_aggregate(q, 0.0, by="doc_type")
    assert _shape(agg) == [("unstructured", 30, 0), ("note", 10, 3)]
    assert idx.calls[-1] == dict(fn="search_counts", size=5, group_mask=TAG_DOCTYPE_MASK, n_groups=3)
    assert not any(c["fn"].endswith("by_keys") or c["fn"] in ("group_keys_from_attr", "group_keys_from_tag", "attr_minmax") for c in idx.calls)


def test_value_errors(world):
    hip, idx, q, docs = world
    for bad in ("patient", "", None, "doc_id", "conditionCodeText", 3):
        with pytest.raises(ValueError, match="collapse must be"):
            hip.semantic_search_collapsed(q, collapse=bad)
        with pytest.raises(ValueError, match="by must be"):
            hip.semantic_aggregate(q, 0.0, by=bad)
    with pytest.raises(ValueError, match="by must be"):                  # no such index: no schema to find the field in
        indexer.HipIndexer(None, "no-such-index").semantic_aggregate(q, 0.0, by="resourceType")
    for by, interval in (("resourceType", 7), ("patientId", "month"), ("doc_type", 1)):
        with pytest.raises(ValueError, match="interval needs an int or date"):
            hip.semantic_aggregate(q, 0.0, by=by, interval=interval)
    for by, interval in (("code", "month"), ("code", 0), ("code", -2), ("code", 1.5), ("code", True), ("chunkDate", "hour"),
                         ("chunkDate", "fortnight")):
        with pytest.raises(ValueError, match="interval must be"):
            hip.semantic_aggregate(q, 0.0, by=by, interval=interval)
    n = len(idx.calls)
    assert hip.semantic_aggregate(np.zeros(0), 0.0, by="resourceType") == EMPTY
    assert hip.semantic_search_collapsed(None, collapse="code") == ([], 0)
    assert hip.semantic_aggregate(q, 0.0, by="code", patient_id="nobody") == EMPTY and len(idx.calls) == n


def test_collapse_and_terms_by_keyword(world):
    hip, idx, q, docs = world
    hits, total = hip.semantic_search_collapsed(q, k=10, collapse="resourceType")
    assert [(h[0].get("resourceType"), h[0]["n"]) for h in hits] == [("Condition", 0), ("Observation", 1), (None, 2), ("Procedure", 3)]
    assert total == 4 and hits[0][1] > hits[1][1] > hits[2][1]
    call = idx.calls[-1]
    assert call["fn"] == "search_grouped_by_keys" and call["n_groups"] == 4 and call["allow"] is None and call["k"] == 10
    assert [c for c in idx.calls if c["fn"] == "group_keys_from_attr"][-1] == dict(fn="group_keys_from_attr", col=0, base=0, missing=0, edges=None)
    hits, total = hip.semantic_search_collapsed(q, k=2, collapse="resourceType", patient_id="bob")    # bob: n % 3 == 1
    assert [h[0]["n"] for h in hits] == [1, 4] and total == 4
    agg = hip.semantic_aggregate(q, 0.0, by="resourceType")
    assert _shape(agg) == [(None, 10, 2), ("Condition", 10, 0), ("Observation", 10, 1), ("Procedure", 10, 3)]    # a tie: key order
    assert agg["cardinality"] == 4 and agg["total"] == 40 and agg["sum_other_doc_count"] == 0
    agg = hip.semantic_aggregate(q, 0.0, by="resourceType", size=1)
    assert _shape(agg) == [(None, 10, 2)] and agg["sum_other_doc_count"] == 30


def test_group_by_value_on_int_and_date_fields(world):
    hip, idx, q, docs = world
    agg = hip.semantic_aggregate(q, 0.0, by="code", size=10)
    codes = [d.get("code") for d in docs]
    want = sorted(((codes.count(v), v) for v in set(codes)), key=lambda t: (-t[0], 10 ** 9 if t[1] is None else t[1]))
    assert [(b["key"], b["doc_count"]) for b in agg["buckets"]] == [(v, c) for c, v in want]
    assert agg["total"] == 40 and [c for c in idx.calls if c["fn"] == "group_keys_from_attr"][-1]["base"] == 0
    hits, total = hip.semantic_search_collapsed(q, k=3, collapse="chunkDate")
    assert total == len({d.get("chunkDate") for d in docs}) and [h[0]["n"] for h in hits] == [0, 1, 2]
    base = [c for c in idx.calls if c["fn"] == "group_keys_from_attr"][-1]
    assert base["base"] == day("2024-01-28") and base["missing"] == day("2024-05-21") - day("2024-01-28") + 1
    agg = hip.semantic_aggregate(q, 0.0, by="chunkDate", size=2)
    assert agg["buckets"][0]["key"] is None and agg["buckets"][0]["doc_count"] == 5 and agg["buckets"][1]["key"] == "2024-01-28"
    # a span the table cannot hold
    idx.set_attr(1, 0, np.array([-5_000_000]))
    with pytest.raises(ValueError, match="spans 5000004 values"):
        hip.semantic_aggregate(q, 0.0, by="code")
    # a field nobody has a value in: every chunk is in the one group None, as for any other missing value; a histogram counts none
    idx.attr[1, :] = R.MISSING
    assert _shape(hip.semantic_aggregate(q, 0.0, by="code")) == [(None, 40, 0)]
    hits, total = hip.semantic_search_collapsed(q, collapse="code")
    assert [h[0]["n"] for h in hits] == [0] and total == 1
    assert hip.semantic_aggregate(q, 0.0, by="code", interval=5) == EMPTY


def test_calendar_edges():
    E = indexer.histogram_edges
    assert E(day("2024-01-31"), day("2024-03-01"), "month", "date") == [day(s) for s in ("2024-01-01", "2024-02-01", "2024-03-01", "2024-04-01")]
    assert E(day("2023-12-31"), day("2024-01-01"), "month", "date") == [day(s) for s in ("2023-12-01", "2024-01-01", "2024-02-01")]
    assert E(day("2024-02-29"), day("2024-02-29"), "month", "date") == [day("2024-02-01"), day("2024-03-01")]       # leap day
    assert E(day("2024-02-29"), day("2024-02-29"), "day", "date") == [day("2024-02-29"), day("2024-03-01")]
    assert E(day("2023-06-15"), day("2025-01-01"), "year", "date") == [day(s) for s in ("2023-01-01", "2024-01-01", "2025-01-01", "2026-01-01")]
    assert E(day("1969-12-31"), day("1970-01-01"), "year", "date") == [day("1969-01-01"), 0, 365]
    # weeks start on Monday: 2024-02-26 is one; a Sunday belongs to the week before, a Monday starts its own
    assert E(day("2024-02-29"), day("2024-03-04"), "week", "date") == [day("2024-02-26"), day("2024-03-04"), day("2024-03-11")]
    assert E(day("2024-03-03"), day("2024-03-03"), "week", "date") == [day("2024-02-26"), day("2024-03-04")]
    assert E(day("1969-12-28"), day("1970-01-01"), "week", "date") == [day("1969-12-22"), day("1969-12-29"), day("1970-01-05")]
    assert dt.date(2024, 2, 26).weekday() == 0
    # plain intervals: multiples of the interval, negatives floor
    assert E(3, 21, 7, "int") == [0, 7, 14, 21, 28] and E(-8, -1, 7, "int") == [-14, -7, 0] and E(5, 5, 1, "int") == [5, 6]
    assert E(day("2024-01-25"), day("2024-02-05"), 7, "date") == [day("2024-01-25") // 7 * 7 + 7 * j for j in range(3)]
    # the refusals name the count
    assert len(E(0, 4095, 1, "int")) == 4097
    with pytest.raises(ValueError, match="4097 buckets"):
        E(0, 4096, 1, "int")
    with pytest.raises(ValueError, match="4097 month buckets"):
        E(day("1700-01-15"), day("2041-05-01"), "month", "date")
    assert len(E(day("1700-01-15"), day("2041-04-30"), "month", "date")) == 4097
    with pytest.raises(ValueError, match="5000 buckets"):
        E(day("2000-01-01"), day("2000-01-01") + 4999, "day", "date")
    with pytest.raises(ValueError, match="beyond int32"):
        E((1 << 31) - 10, (1 << 31) - 2, 1000, "int")
    for bad in ("month", "hour", 0, None, 2.0):
        with pytest.raises(ValueError, match="interval must be"):
            E(0, 10, bad, "int")


def test_histograms_come_in_key_order(world):
    hip, idx, q, docs = world
    agg = hip.semantic_aggregate(q, 0.0, by="chunkDate", interval="month", size=1)
    by_month = {}
    for d in docs:
        if "chunkDate" in d:
            by_month.setdefault(d["chunkDate"][:7] + "-01", []).append(d["n"])
    assert [(b["key_as_string"], b["doc_count"], b["top_hit"][0]["n"]) for b in agg["buckets"]] == \
        [(m, len(ns), min(ns)) for m, ns in sorted(by_month.items())]
    assert [b["key"] for b in agg["buckets"]] == [day(b["key_as_string"]) for b in agg["buckets"]]
    assert agg["total"] == 35 and agg["cardinality"] == len(by_month) == 5 and agg["sum_other_doc_count"] == 0    # size is not used
    call = idx.calls[-1]
    assert call["fn"] == "search_counts_by_keys" and call["size"] == call["n_groups"] == 5
    assert [c for c in idx.calls if c["fn"] == "group_keys_from_attr"][-1]["missing"] == -1          # rows without a date are not counted
    # an int field in buckets of 2 units
    agg = hip.semantic_aggregate(q, 0.0, by="code", interval=2)
    assert [(b["key"], b["doc_count"]) for b in agg["buckets"]] == [(0, sum(1 for d in docs if d.get("code") in (0, 1))),
                                                                   (2, sum(1 for d in docs if d.get("code") in (2, 3)))]
    assert "key_as_string" not in agg["buckets"][0]
    weekly = hip.semantic_aggregate(q, indexer._score_out(0.9), by="chunkDate", interval="week")
    keys = [b["key"] for b in weekly["buckets"]]
    assert keys == sorted(keys) and all(dt.date.fromisoformat(b["key_as_string"]).weekday() == 0 for b in weekly["buckets"])
    assert sum(b["doc_count"] for b in weekly["buckets"]) == weekly["total"] > 0
    # too many buckets: refused with the count, before any search
    idx.set_attr(2, 5, np.array([day("2024-01-28") + 6000]))
    n = len([c for c in idx.calls if c["fn"].startswith("search")])
    with pytest.raises(ValueError, match="6001 buckets"):
        hip.semantic_aggregate(q, 0.0, by="chunkDate", interval="day")
    assert len([c for c in idx.calls if c["fn"].startswith("search")]) == n


def test_where_is_compiled_once_under_the_lock(world, monkeypatch):
    hip, idx, q, docs = world
    st = REGISTRY.get(hip.index_name, create=False)
    seen = []
    real = attrfilter.compile_filter

    def spy(where, schema, patients, doc_types, *a, **kw):
        seen.append(st.lock._is_owned())
        return real(where, schema, patients, doc_types, *a, **kw)

    def run_plan(index, plan):      # the one shape these filters compile to, through the stand-in's builder
        assert plan[0] == "all" and st.lock._is_owned()
        return index.allow_from_attr_clauses(np.array([(0, c, lo, hi, neg) for c, lo, hi, neg in plan[1]]).reshape(-1, 5),
                                             nq=1, shared=True, mode="all")

    monkeypatch.setattr(attrfilter, "compile_filter", spy)
    monkeypatch.setattr(attrfilter, "run_plan", run_plan)
    where = {"range": {"chunkDate": {"gte": "2024-02-01", "lt": "2024-03-01"}}}
    inside = [d for d in docs if "2024-02-01" <= d.get("chunkDate", "") < "2024-03-01"]
    agg = hip.semantic_aggregate(q, 0.0, by="resourceType", where=where)
    assert seen == [True]
    want = {}
    for d in inside:
        want.setdefault(d.get("resourceType"), []).append(d["n"])
    assert {b["key"]: (b["doc_count"], b["top_hit"][0]["n"]) for b in agg["buckets"]} == {k: (len(v), min(v)) for k, v in want.items()}
    assert agg["total"] == len(inside)
    call = idx.calls[-1]
    assert call["fn"] == "search_counts_by_keys" and call["allow"].dtype == bool and call["allow"].sum() == len(inside)
    # with where= the tag fields go through the key path too, keys from the tag
    agg = hip.semantic_aggregate(q, 0.0, by="patientId", where=where)
    call = idx.calls[-1]
    assert call["fn"] == "search_counts_by_keys" and call["n_groups"] == 4 and seen == [True, True]
    assert np.array_equal(call["keys"], [1 + n % 3 for n in range(40)]) and dict(fn="group_keys_from_tag", mask=TAG_PATIENT_MASK) in idx.calls[-3:]
    assert {b["key"]: b["doc_count"] for b in agg["buckets"]} == {p: sum(1 for d in inside if d["patientId"] == p) for p in ("alice", "bob", "carol")}
    hits, total = hip.semantic_search_collapsed(q, k=5, collapse="doc_type", where=where)
    assert idx.calls[-1]["fn"] == "search_grouped_by_keys" and total == 2 and [h[0]["n"] for h in hits] == sorted(min(d["n"] for d in inside if d["doc_type"] == t) for t in ("unstructured", "note"))
    with pytest.raises(ValueError, match="nope"):
        hip.semantic_aggregate(q, 0.0, by="code", where={"term": {"nope": 1}})
    idx.dim = 1536                                     # wide rows take no bitmap
    with pytest.raises(NotImplementedError, match="dim <= 1024"):
        hip.semantic_aggregate(q, 0.0, by="code", where=where)
    with pytest.raises(NotImplementedError, match="dim <= 1024"):
        hip.semantic_search_collapsed(q, collapse="patientId", where=where)
    agg = hip.semantic_aggregate(q, 0.0, by="code", size=10)                      # ... and keys alone are fine there
    assert agg["total"] == 40 and {b["key"]: b["doc_count"] for b in agg["buckets"]}[None] == 6


def test_layout_epoch_retry(world):
    hip, idx, q, docs = world
    idx.compact_during_next = 2       # the key build and then the search of the first attempt see a compaction; the second is clean
    before = len([c for c in idx.calls if c["fn"] == "search_counts_by_keys"])
    agg = hip.semantic_aggregate(q, 0.0, by="resourceType")
    assert agg["total"] == 40 and len([c for c in idx.calls if c["fn"] == "search_counts_by_keys"]) - before == 2
    assert len([c for c in idx.calls if c["fn"] == "group_keys_from_attr"]) == 2                   # the keys are rebuilt per attempt
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_search_collapsed(q, collapse="resourceType")


def test_an_index_without_the_methods_says_so():
    name = "gba-cpu-plain"
    q, _, _ = _fill(name, PlainIndex())
    try:
        hip = indexer.HipIndexer(None, name)
        with pytest.raises(NotImplementedError, match="PlainIndex has no aggregation over a key column"):
            hip.semantic_aggregate(q, 0.0, by="resourceType")
        with pytest.raises(NotImplementedError, match="PlainIndex has no grouped search over a key column"):
            hip.semantic_search_collapsed(q, collapse="code")
        with pytest.raises(NotImplementedError, match="over a key column"):
            hip.semantic_aggregate(q, 0.0, by="patientId", where={"term": {"code": 1}})
        assert hip.semantic_aggregate(q, 0.0)["total"] == 40 and hip.semantic_search_collapsed(q)[1] == 3    # the tag path is whole
    finally:
        REGISTRY.drop(name)


def test_flat_index_key_methods_validate_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def __getattr__(self, name):
            def reached(*a):
                raise AssertionError("the native entry point was reached with bad arguments")
            return reached

    idx = FlatIndex(types.SimpleNamespace(_L=Lib(), device=0), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    keys = np.zeros(10, dtype=np.int32)
    good = dict(queries=q, k=5, keys=keys, n_groups=10)
    bad = [dict(queries=np.zeros(DIM)), dict(k=0), dict(k=4097), dict(n_groups=0), dict(n_groups=(1 << 20) + 1),
           dict(keys=np.zeros((2, 5), dtype=np.int32)), dict(keys=np.zeros(5)), dict(keys=np.array([1 << 31])), dict(keys="abc"),
           dict(allow=np.zeros((2, 4), dtype=np.uint32)), dict(allow=np.zeros((3, 2, 2), dtype=np.uint32)),
           dict(q_filter=np.zeros(2, dtype=np.int32)), dict(q_filter_mask=np.zeros(3, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_grouped_by_keys(**dict(good, **kw))
        kw = {("size" if k == "k" else k): v for k, v in kw.items()}
        with pytest.raises(ValueError):
            idx.search_counts_by_keys(**dict(dict(queries=q, min_score=0.5, size=5, keys=keys, n_groups=10), **kw))
    for ms in (float("nan"), np.zeros(2), None):
        with pytest.raises(ValueError):
            idx.search_counts_by_keys(q, ms, 5, keys, 10)
    for kw in (dict(k=0), dict(k=4097), dict(n_groups=0), dict(n_groups=(1 << 20) + 1)):
        a = dict(dict(k=5, n_groups=10), **kw)
        with pytest.raises(ValueError):
            idx.search_grouped_by_keys_device(0, 3, a["k"], 0, 10, a["n_groups"], 0, 0, 0, 0, 0)
        with pytest.raises(ValueError):
            idx.search_counts_by_keys_device(0, 3, 0, a["k"], 0, 10, a["n_groups"], 0, 0, 0, 0, 0, 0, 0)
    for kw in (dict(col=8), dict(col=-1), dict(missing=-2), dict(base=1 << 31), dict(edges=[1]), dict(edges=[2, 2]), dict(edges=[3, 1]),
               dict(edges=np.arange(4098)), dict(edges=[0.5, 1.5]), dict(edges=[[0, 1]]), dict(edges=[0, 1], base=3), dict(edges=[0, 1 << 31])):
        with pytest.raises(ValueError):
            idx.group_keys_from_attr(**dict(dict(col=2), **kw))
    with pytest.raises(ValueError):
        idx.attr_minmax(8)
    # good arguments do reach it
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_grouped_by_keys_device(0, 3, 5, 0, 10, 10, 0, 0, 0, 0, 0)
    with pytest.raises(AssertionError, match="native entry point"):
        idx.search_counts_by_keys_device(0, 3, 0, 4096, 0, 10, 1 << 20, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(AssertionError, match="native entry point"):
        idx.attr_minmax(7)
