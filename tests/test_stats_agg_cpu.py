"""The host-side layers of the stats sub-aggregation, without a GPU: ``HipIndexer.semantic_stats`` over a stand-in index that
answers ``search_stats_by_keys`` in numpy (``tests/stats_ref.py``) — routing, the global form, histograms and date strings,
``avg`` and its None case, the host-side ``sum`` / ``avg`` order and its refusal, the keyword / IVF / sharded refusals and
the layout-epoch retry — and the two new symbols in the header and the ctypes table."""
import ctypes
import datetime as dt
import os
import re

import numpy as np
import pytest

import stats_ref as R
from rassengine_amd import _native, attrfilter, indexer
from rassengine_amd.docstore import REGISTRY
from test_group_by_attr_cpu import PlainIndex, StandInIndex, _fill, day

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = {"buckets": [], "sum_other_doc_count": 0, "cardinality": 0, "total": 0}
ORDER = {"_count": R.BY_COUNT, "value_count": R.BY_VALUE_COUNT, "min": R.BY_MIN, "max": R.BY_MAX}


class StatsIndex(StandInIndex):
    """... plus ``search_stats_by_keys``.  ``keys`` None is the global form."""

    def search_stats_by_keys(self, queries, min_score, size, keys, n_groups, value_col, order_by="_count", descending=True,
                             allow=None, q_filter=None, q_filter_mask=None):
        self._note("search_stats_by_keys", size=size, keys=None if keys is None else np.array(keys), n_groups=n_groups,
                   value_col=value_col, order_by=order_by, descending=descending, allow=allow)
        if keys is not None:
            keys = np.concatenate([keys, np.full(max(0, self.rows - len(keys)), -1)])
        got = R.expect(self._scores(queries), self.tags, keys, self.attr[value_col], n_groups, size, min_score, ORDER[order_by],
                       descending, allow, q_filter, q_filter_mask)
        assert got[10] == 0, "a hit's group key is >= n_groups"
        return got[:10]


@pytest.fixture
def world():
    name = "stats-cpu"
    idx = StatsIndex()
    q, cos, docs = _fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, docs
    REGISTRY.drop(name)


def _stats_of(docs, field, conv=lambda v: v):
    v = [conv(d[field]) for d in docs if field in d]
    return {"count": len(v), "min": min(v) if v else None, "max": max(v) if v else None, "sum": sum(v),
            "avg": float(sum(v)) / float(len(v)) if v else None}


def _plain(stats):
    return {k: stats[k] for k in ("count", "min", "max", "sum", "avg")}


def test_global_stats_and_routing(world):
    hip, idx, q, docs = world
    agg = hip.semantic_stats(q, 0.0, "code")
    call = idx.calls[-1]
    assert call["fn"] == "search_stats_by_keys" and call["keys"] is None and call["n_groups"] == 1 and call["value_col"] == 1
    assert call["order_by"] == "_count" and call["descending"] is True and call["allow"] is None and call["size"] == 5
    assert not any(c["fn"].startswith("group_keys") for c in idx.calls)       # no key column is built for the global form
    assert len(agg["buckets"]) == 1 and agg["cardinality"] == 1 and agg["total"] == 40 and agg["sum_other_doc_count"] == 0
    b = agg["buckets"][0]
    assert b["key"] is None and b["doc_count"] == 40 and b["top_hit"][0]["n"] == 0
    assert b["stats"] == _stats_of(docs, "code") and isinstance(b["stats"]["avg"], float)
    # a threshold keeps the best chunks only (cos falls with n): fewer hits, their stats
    few = hip.semantic_stats(q, 0.9, "code")
    assert 0 < few["total"] < 40
    assert _plain(few["buckets"][0]["stats"]) == _stats_of(docs[:few["total"]], "code")


def test_where_goes_through_a_bitmap_in_the_global_form_too(world, monkeypatch):
    hip, idx, q, docs = world

    def run_plan(index, plan):      # the one shape this filter compiles to, through the stand-in's builder
        assert plan[0] == "all"
        return index.allow_from_attr_clauses(np.array([(0, c, lo, hi, neg) for c, lo, hi, neg in plan[1]]).reshape(-1, 5),
                                             nq=1, shared=True, mode="all")

    monkeypatch.setattr(attrfilter, "run_plan", run_plan)
    for by in (None, "patientId"):
        agg = hip.semantic_stats(q, 0.0, "code", by=by, where={"range": {"code": {"gte": 2}}})
        assert idx.calls[-1]["fn"] == "search_stats_by_keys" and idx.calls[-1]["allow"] is not None
        inside = [d for d in docs if d.get("code", -1) >= 2]
        assert agg["total"] == len(inside) and sum(b["stats"]["sum"] for b in agg["buckets"]) == sum(d["code"] for d in inside)
    assert _plain(hip.semantic_stats(q, 0.0, "code", where={"range": {"code": {"gte": 2}}})["buckets"][0]["stats"]) == _stats_of(inside, "code")


def test_per_patient_through_the_tag_key_column_and_device_orders(world):
    hip, idx, q, docs = world
    agg = hip.semantic_stats(q, 0.0, "code", by="patientId", order={"max": "desc"})
    call = idx.calls[-1]
    assert call["order_by"] == "max" and call["descending"] is True and call["n_groups"] == 4
    assert any(c["fn"] == "group_keys_from_tag" for c in idx.calls) and not any(c["fn"] == "search_counts" for c in idx.calls)
    per = {p: _stats_of([d for d in docs if d["patientId"] == p], "code") for p in ("alice", "bob", "carol")}
    names = ["alice", "bob", "carol"]
    want = sorted(names, key=lambda p: (-per[p]["max"], names.index(p)))
    assert [b["key"] for b in agg["buckets"]] == want
    for b in agg["buckets"]:
        assert b["stats"] == per[b["key"]] and b["doc_count"] == sum(d["patientId"] == b["key"] for d in docs)
    agg = hip.semantic_stats(q, 0.0, "code", by="patientId", order={"value_count": "asc"}, size=2)
    assert idx.calls[-1]["order_by"] == "value_count" and idx.calls[-1]["descending"] is False and idx.calls[-1]["size"] == 2
    assert [b["key"] for b in agg["buckets"]] == sorted(names, key=lambda p: (per[p]["count"], names.index(p)))[:2]
    assert agg["cardinality"] == 3 and agg["sum_other_doc_count"] == 40 - sum(b["doc_count"] for b in agg["buckets"])


def test_date_field_histogram_and_strings(world):
    hip, idx, q, docs = world
    agg = hip.semantic_stats(q, 0.0, "chunkDate", by="chunkDate", interval="month")
    assert idx.calls[-1]["size"] == idx.calls[-1]["n_groups"] and idx.calls[-1]["order_by"] == "_count"
    keys = [b["key"] for b in agg["buckets"]]
    assert keys == sorted(keys) and len(keys) > 2                           # no order: key order
    for b in agg["buckets"]:
        first = dt.date(1970, 1, 1) + dt.timedelta(days=b["key"])
        inside = [d for d in docs if "chunkDate" in d and d["chunkDate"][:7] == first.isoformat()[:7]]
        want = _stats_of(inside, "chunkDate", day)
        assert b["key_as_string"] == first.isoformat() and b["doc_count"] == len(inside)
        assert _plain(b["stats"]) == want
        assert b["stats"]["min_as_string"] == min(d["chunkDate"] for d in inside)
        assert b["stats"]["max_as_string"] == max(d["chunkDate"] for d in inside)
    # a histogram ordered by a device metric lists every bucket in that order
    by_min = hip.semantic_stats(q, 0.0, "code", by="chunkDate", interval="month", order={"min": "desc"})
    mins = [(b["stats"]["min"] is None, -(b["stats"]["min"] or 0), b["key"]) for b in by_min["buckets"]]
    assert mins == sorted(mins) and len(by_min["buckets"]) == len(keys)


def test_avg_none_and_buckets_without_a_value_last(world):
    hip, idx, q, docs = world
    idx.attr[1, [n for n in range(40) if n % 3 == 1]] = R.MISSING            # bob's chunks have no code at all
    for direction in ("asc", "desc"):
        for by in ("min", "max", "value_count", "sum", "avg"):
            agg = hip.semantic_stats(q, 0.0, "code", by="patientId", order={by: direction})
            assert [b["key"] for b in agg["buckets"]][-1] == "bob", (by, direction)
            last = agg["buckets"][-1]
            assert last["doc_count"] > 0 and last["stats"] == {"count": 0, "min": None, "max": None, "sum": 0, "avg": None}
    idx.attr[2, :] = R.MISSING
    b = hip.semantic_stats(q, 0.0, "chunkDate")["buckets"][0]
    assert b["stats"]["avg"] is None and b["stats"]["min_as_string"] is None and b["stats"]["max_as_string"] is None


def test_sum_and_avg_are_ordered_on_the_host_or_refused(world):
    hip, idx, q, docs = world
    names = ["alice", "bob", "carol"]
    per = {p: _stats_of([d for d in docs if d["patientId"] == p], "code") for p in names}
    for by in ("sum", "avg"):
        for direction, sign in (("asc", 1), ("desc", -1)):
            agg = hip.semantic_stats(q, 0.0, "code", by="patientId", order={by: direction})
            assert idx.calls[-1]["order_by"] == "_count"                      # the device lists, the host orders
            assert [b["key"] for b in agg["buckets"]] == sorted(names, key=lambda p: (sign * per[p][by], names.index(p)))
        with pytest.raises(ValueError, match="needs every bucket listed"):     # 3 buckets, 2 asked for
            hip.semantic_stats(q, 0.0, "code", by="patientId", order={by: "desc"}, size=2)
        agg = hip.semantic_stats(q, 0.0, "code", by="chunkDate", interval="month", order={by: "desc"})    # a histogram: always
        got = [b["stats"][by] for b in agg["buckets"] if b["stats"]["count"]]
        assert got == sorted(got, reverse=True) and len(got) > 1


def test_refusals(world):
    hip, idx, q, docs = world
    with pytest.raises(ValueError, match="codes have no arithmetic"):
        hip.semantic_stats(q, 0.0, "resourceType")
    with pytest.raises(ValueError, match="field must be"):
        hip.semantic_stats(q, 0.0, "nonesuch")
    for bad in ({"median": "asc"}, {"min": "up"}, {"min": "asc", "max": "asc"}, "min"):
        with pytest.raises(ValueError, match="order must be"):
            hip.semantic_stats(q, 0.0, "code", order=bad)
    with pytest.raises(ValueError, match="interval needs by="):
        hip.semantic_stats(q, 0.0, "code", interval=5)
    with pytest.raises(ValueError, match="NaN"):
        hip.semantic_stats(q, float("nan"), "code")
    n = len(idx.calls)
    assert hip.semantic_stats(np.zeros(0), 0.0, "code") == EMPTY
    assert hip.semantic_stats(q, 0.0, "code", patient_id="nobody") == EMPTY and len(idx.calls) == n
    assert indexer.HipIndexer(None, "no-such-index").semantic_stats(q, 0.0, "code") == EMPTY


@pytest.mark.parametrize("cls", [PlainIndex, StandInIndex], ids=["ivf-like", "sharded-like"])
def test_indices_without_the_stats_scan_refuse(cls):
    name = "stats-cpu-plain"
    idx = cls()
    q, cos, docs = _fill(name, idx)
    try:
        with pytest.raises(NotImplementedError, match="no stats aggregation"):
            indexer.HipIndexer(None, name).semantic_stats(q, 0.0, "code")
    finally:
        REGISTRY.drop(name)


def test_a_compaction_between_build_and_answer_is_retried(world):
    hip, idx, q, docs = world
    want = hip.semantic_stats(q, 0.0, "code", by="patientId")
    calls = lambda: sum(c["fn"] == "search_stats_by_keys" for c in idx.calls)
    n, epoch = calls(), idx.layout_epoch
    idx.compact_during_next = 1          # the layout moves under the next native call: that attempt is thrown away
    assert hip.semantic_stats(q, 0.0, "code", by="patientId") == want
    assert idx.layout_epoch == epoch + 1 and calls() > n + 1


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    for sym, n_args in (("rass_index_aggregate_stats_keys", 26), ("rass_index_aggregate_stats_keys_device", 28)):
        decl = re.search(r"^int %s\(([^;]*)\);" % sym, header, flags=re.M)
        assert decl and len(decl.group(1).split(",")) == n_args, sym
        restype, argtypes = _native.SIGNATURES[sym]
        assert restype is ctypes.c_int and len(argtypes) == n_args, sym
    for k, name in enumerate(("RASS_STATS_BY_COUNT", "RASS_STATS_BY_VALUE_COUNT", "RASS_STATS_BY_MIN", "RASS_STATS_BY_MAX")):
        assert re.search(r"^#define %s %d$" % (name, k), header, flags=re.M) and getattr(_native, name) == k
