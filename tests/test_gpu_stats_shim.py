"""The stats sub-aggregation end to end: ``HipIndexer.semantic_stats`` over a real index of ~300 docs with an int and a date
field (schema ``resourceType:keyword,code:int,chunkDate:date``), overwrites, deletes and a compaction between build and
search, against a host loop over the stored docs.  Scores are the oracle's (``KIND_F32_MFMA``) over the rows as the index
stores them and the query as the GPU normalised it; nothing expected comes from a search."""
import datetime as dt

import numpy as np
import pytest

from test_gpu_group_by_attr import DIM, EPOCH, Host, _docs, day

pytestmark = pytest.mark.gpu


def _stats(values, date=False):
    v = list(values)
    out = {"count": len(v), "min": min(v) if v else None, "max": max(v) if v else None, "sum": sum(v),
           "avg": float(sum(v)) / float(len(v)) if v else None}
    if date:
        iso = lambda d: None if d is None else (EPOCH + dt.timedelta(days=d)).isoformat()
        out["min_as_string"], out["max_as_string"] = iso(out["min"]), iso(out["max"])
    return out


def _want(host, thr, key_of, value_of, keep=lambda d: True, date=False):
    """key -> (doc_count, (best doc_id, score), stats) over the docs scoring >= thr; key_of(d) None = left out."""
    per = {}
    for s, r, d in host.live:                    # score desc, row asc: the first doc of a key is its top hit
        k = key_of(d)
        if s >= thr and keep(d) and k is not None:
            per.setdefault(k, [0, (d["doc_id"], s), []])
            per[k][0] += 1
            if value_of(d) is not None:
                per[k][2].append(value_of(d))
    return {k: (c, top, _stats(v, date)) for k, (c, top, v) in per.items()}


def _listed(agg):
    return [(b["key"], b["doc_count"], (b["top_hit"][0]["doc_id"], b["top_hit"][1]), b["stats"]) for b in agg["buckets"]]


def test_shim_stats(gpu, oracle, monkeypatch):
    from rassengine_amd import config, indexer
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,code:int,chunkDate:date")
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "cosine")
    eng = Engine(0, DIM)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: eng.open_index(name))
    try:
        rng = np.random.default_rng(29)
        name, n = "rass-idx-stats", 300
        docs = _docs(rng, n)
        emb = rng.standard_normal((n, DIM), dtype=np.float32)
        indexer.add_documents(name, docs[:200], emb[:200])
        st = REGISTRY.get(name)
        over = [dict(docs[i], code=int(100 + i), chunkDate="2024-02-29") for i in range(40, 60)]      # overwritten
        for d in over:
            docs[int(d["doc_id"][1:])] = d
        indexer.add_documents(name, docs[200:] + over, np.concatenate([emb[200:], emb[40:60]]))
        with st.lock:                                                                                 # deleted outright
            for i in range(100, 110):
                r = st.doc_row.pop(f"d{i}")
                st.index.delete(r)
                st.row_doc[r] = None
        hip = indexer.HipIndexer(None, name)
        q = rng.standard_normal(DIM).astype(np.float32)
        code = lambda d: d.get("code")
        date = lambda d: day(d["chunkDate"]) if "chunkDate" in d else None
        patients = st.patients.names()

        def check_all(host):
            thr = host.live[119][0]                                               # the 120 best chunks are the hits
            # global: one bucket, over the hits and over everything
            for t, total in ((thr, 120), (-np.inf, len(host.live))):
                agg = hip.semantic_stats(q, t, "code")
                want = _want(host, t, lambda d: "all", code)["all"]
                assert _listed(agg) == [(None,) + want] and agg["total"] == total and agg["cardinality"] == 1
            agg = hip.semantic_stats(q, thr, "chunkDate")
            assert _listed(agg) == [(None,) + _want(host, thr, lambda d: "all", date, date=True)["all"]]
            # per patient, the latest date first; and by the smallest code ascending, cut at 2
            want = _want(host, thr, lambda d: d["patientId"], date, date=True)
            order = sorted(want, key=lambda p: (-want[p][2]["max"], patients.index(p)))
            agg = hip.semantic_stats(q, thr, "chunkDate", by="patientId", order={"max": "desc"})
            assert _listed(agg) == [(p,) + want[p] for p in order] and len(order) == 4
            want = _want(host, thr, lambda d: d["patientId"], code)
            order = sorted(want, key=lambda p: (want[p][2]["min"], patients.index(p)))[:2]
            agg = hip.semantic_stats(q, thr, "code", by="patientId", order={"min": "asc"}, size=2)
            assert _listed(agg) == [(p,) + want[p] for p in order] and agg["cardinality"] == 4
            assert agg["sum_other_doc_count"] == 120 - sum(want[p][0] for p in order)
            # per month: key order; the mean code of the relevant chunks of each month
            month = lambda d: day(d["chunkDate"][:7] + "-01") if "chunkDate" in d else None
            want = _want(host, thr, month, code)
            agg = hip.semantic_stats(q, thr, "code", by="chunkDate", interval="month")
            assert _listed(agg) == [(k,) + want[k] for k in sorted(want)] and len(want) >= 5
            agg = hip.semantic_stats(q, thr, "code", by="chunkDate", interval="month", order={"avg": "desc"})
            have = [k for k in want if want[k][2]["count"]]
            order = sorted(have, key=lambda k: (-want[k][2]["avg"], k)) + sorted(k for k in want if not want[k][2]["count"])
            assert _listed(agg) == [(k,) + want[k] for k in order]
            # under where= and a patient filter
            where = {"range": {"chunkDate": {"gte": "2024-01-01", "lt": "2024-03-01"}}}
            inside = lambda d: "2024-01-01" <= d.get("chunkDate", "") < "2024-03-01"
            want = _want(host, thr, lambda d: "all", code, keep=inside)["all"]
            assert _listed(hip.semantic_stats(q, thr, "code", where=where)) == [(None,) + want] and 0 < want[0] < 120
            want = _want(host, thr, lambda d: d["doc_type"], date, keep=lambda d: inside(d) and d["patientId"] == "p1", date=True)
            agg = hip.semantic_stats(q, thr, "chunkDate", by="doc_type", where=where, patient_id="p1", order={"value_count": "desc"})
            types = st.doc_types.names()
            order = sorted(want, key=lambda k: (-want[k][2]["count"], types.index(k)))
            assert _listed(agg) == [(k,) + want[k] for k in order]

        check_all(Host(gpu, oracle, st, q))
        st.compact()
        assert st.index.rows == st.index.count == 290
        check_all(Host(gpu, oracle, st, q))
        with pytest.raises(ValueError, match="codes have no arithmetic"):
            hip.semantic_stats(q, 0.0, "resourceType")
        with pytest.raises(ValueError, match="needs every bucket listed"):
            hip.semantic_stats(q, -np.inf, "code", by="patientId", order={"sum": "asc"}, size=2)
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()
