"""Grouping and aggregating by attribute fields end to end: ``HipIndexer.semantic_search_collapsed`` / ``semantic_aggregate``
over a real index with the schema ``resourceType:keyword,code:int,chunkDate:date``, against a host computation over the
stored docs.  Scores are the oracle's (``KIND_F32_MFMA``) over the rows as the index stores them and the query as the GPU
normalised it; nothing expected comes from a search."""
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 128
EPOCH = dt.date(1970, 1, 1)


def day(s):
    return (dt.date.fromisoformat(s) - EPOCH).days


def _docs(rng, n):
    types = ["Observation", "Condition", "Encounter", "Procedure"]
    docs = []
    for i in range(n):
        d = {"doc_id": f"d{i}", "doc_type": "note" if i % 5 == 0 else "unstructured", "patientId": f"p{i % 4}"}
        if rng.random() < 0.9:
            d["resourceType"] = types[int(rng.integers(4))]
        if rng.random() < 0.8:
            d["code"] = int(rng.integers(-3, 25))
        if rng.random() < 0.85:
            d["chunkDate"] = (dt.date(2023, 11, 20) + dt.timedelta(days=int(rng.integers(0, 130)))).isoformat()
        docs.append(d)
    return docs


class Host:
    """The live docs of the index with their oracle scores for one query: what every expectation below is computed from."""

    def __init__(self, torch, oracle, st, q):
        from rassengine_amd import ops
        rows = st.index.rows
        xn = np.stack([st.index.get_row(r) for r in range(rows)]).astype(np.float32)
        qn = ops.normalize_rows(torch.from_numpy(q[None, :]).cuda()).cpu().numpy()
        s = oracle.scores(xn, qn, kind=oracle.KIND_F32_MFMA).astype(np.float32)[0]
        self.live = [(float(s[r]), r, st.row_doc[r]) for r in range(rows) if st.row_doc[r] is not None]
        self.live.sort(key=lambda t: (-t[0], t[1]))                      # score desc, row asc

    def collapse(self, field, k, keep=lambda d: True):
        best = {}
        for s, r, d in self.live:
            if keep(d):
                best.setdefault(d.get(field), (d["doc_id"], s))
        return list(best.values())[:k], len(best)

    def buckets(self, key_of, thr, keep=lambda d: True):
        """key -> (doc_count, the best hit's doc_id and score) over the docs scoring >= thr whose key is not the marker SKIP."""
        out = {}
        for s, r, d in self.live:
            k = key_of(d)
            if s >= thr and keep(d) and k is not SKIP:
                c, top = out.get(k, (0, (d["doc_id"], s)))
                out[k] = (c + 1, top)
        return out


SKIP = object()


def _listed(agg):
    return [(b["key"], b["doc_count"], (b["top_hit"][0]["doc_id"], b["top_hit"][1])) for b in agg["buckets"]]


def test_shim_groups_by_attribute_fields(gpu, oracle, monkeypatch):
    from rassengine_amd import config, indexer
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,code:int,chunkDate:date")
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "cosine")
    eng = Engine(0, DIM)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: eng.open_index(name))
    try:
        rng = np.random.default_rng(23)
        name, n = "rass-idx-gba", 300
        docs = _docs(rng, n)
        emb = rng.standard_normal((n, DIM), dtype=np.float32)
        indexer.add_documents(name, docs[:200], emb[:200])
        st = REGISTRY.get(name)
        # the rest, 20 docs overwritten with other field values, and 10 docs deleted outright
        over = [dict(docs[i], resourceType="Encounter", code=int(i % 7), chunkDate="2024-02-29") for i in range(40, 60)]
        for d in over:
            docs[int(d["doc_id"][1:])] = d
        indexer.add_documents(name, docs[200:] + over, np.concatenate([emb[200:], emb[40:60]]))
        with st.lock:
            for i in range(100, 110):
                r = st.doc_row.pop(f"d{i}")
                st.index.delete(r)
                st.row_doc[r] = None
        assert st.index.rows == 320 and st.index.count == 290
        hip = indexer.HipIndexer(None, name)
        q = rng.standard_normal(DIM).astype(np.float32)
        types = st.attrs.dicts["resourceType"].names()
        kw_order = lambda key: 0 if key is None else 1 + types.index(key)          # a keyword's code: 0 = none

        def check_all(host):
            thr = host.live[119][0]                                               # the 120 best chunks are the hits
            # collapse by keyword: the best chunk of every type, the chunks without one as one group
            for k in (1, 3, 10):
                hits, total = hip.semantic_search_collapsed(q, k=k, collapse="resourceType")
                want, n_groups = host.collapse("resourceType", k)
                assert [(d["doc_id"], s) for d, s in hits] == want and total == n_groups == 5
            hits, total = hip.semantic_search_collapsed(q, k=50, collapse="code", patient_id="p1")
            want, n_groups = host.collapse("code", 50, keep=lambda d: d["patientId"] == "p1")
            assert [(d["doc_id"], s) for d, s in hits] == want and total == n_groups
            # terms by keyword, the None bucket included; count desc, then code asc
            want = host.buckets(lambda d: d.get("resourceType"), thr)
            order = sorted(want, key=lambda key: (-want[key][0], kw_order(key)))
            agg = hip.semantic_aggregate(q, thr, by="resourceType", size=10)
            assert _listed(agg) == [(key,) + want[key] for key in order] and None in want
            assert agg["total"] == 120 and agg["cardinality"] == 5 and agg["sum_other_doc_count"] == 0
            agg = hip.semantic_aggregate(q, thr, by="resourceType", size=2)
            assert _listed(agg) == [(key,) + want[key] for key in order[:2]] and agg["sum_other_doc_count"] == 120 - sum(want[key][0] for key in order[:2])
            # terms by an int field, by value
            want = host.buckets(lambda d: d.get("code"), thr)
            order = sorted(want, key=lambda key: (-want[key][0], 10 ** 6 if key is None else key))
            assert _listed(hip.semantic_aggregate(q, thr, by="code", size=40)) == [(key,) + want[key] for key in order]
            # monthly and 7-day histograms: key order, the chunks without a date left out
            month = lambda d: day(d["chunkDate"][:7] + "-01") if "chunkDate" in d else SKIP
            want = host.buckets(month, thr)
            agg = hip.semantic_aggregate(q, thr, by="chunkDate", interval="month")
            assert _listed(agg) == [(key,) + want[key] for key in sorted(want)] and len(want) >= 5
            assert [b["key_as_string"] for b in agg["buckets"]] == [(EPOCH + dt.timedelta(days=key)).isoformat() for key in sorted(want)]
            assert agg["total"] == sum(c for c, _ in want.values()) < 120 and agg["cardinality"] == len(want)
            week = lambda d: day(d["chunkDate"]) // 7 * 7 if "chunkDate" in d else SKIP
            want = host.buckets(week, -np.inf)
            agg = hip.semantic_aggregate(q, -np.inf, by="chunkDate", interval=7)  # every chunk
            assert _listed(agg) == [(key,) + want[key] for key in sorted(want)] and len(want) >= 18
            # where= a date range together with by= a keyword, a tag field, and a collapse
            where = {"range": {"chunkDate": {"gte": "2024-01-01", "lt": "2024-03-01"}}}
            inside = lambda d: "2024-01-01" <= d.get("chunkDate", "") < "2024-03-01"
            want = host.buckets(lambda d: d.get("resourceType"), thr, keep=inside)
            order = sorted(want, key=lambda key: (-want[key][0], kw_order(key)))
            agg = hip.semantic_aggregate(q, thr, by="resourceType", size=10, where=where)
            assert _listed(agg) == [(key,) + want[key] for key in order] and 0 < agg["total"] < 120
            want = host.buckets(lambda d: d["patientId"], thr, keep=lambda d: inside(d) and d["doc_type"] == "note")
            order = sorted(want, key=lambda key: (-want[key][0], int(key[1:])))
            agg = hip.semantic_aggregate(q, thr, by="patientId", where=where, filter_clause={"term": {"doc_type": "note"}})
            assert _listed(agg) == [(key,) + want[key] for key in order]
            hits, total = hip.semantic_search_collapsed(q, k=3, collapse="resourceType", where=where)
            want, n_groups = host.collapse("resourceType", 3, keep=inside)
            assert [(d["doc_id"], s) for d, s in hits] == want and total == n_groups

        check_all(Host(gpu, oracle, st, q))
        # a compaction lands between the key build and the search: the attempt is void, the next one answers the new layout
        real, fired = st.index.group_keys_from_attr, []

        def racing(*a, **kw):
            out = real(*a, **kw)
            if not fired:
                fired.append(st.compact())
            return out

        monkeypatch.setattr(st.index, "group_keys_from_attr", racing)
        epoch = st.index.layout_epoch
        agg = hip.semantic_aggregate(q, -np.inf, by="resourceType", size=10)
        assert fired == [(320, 290)] and st.index.layout_epoch == epoch + 1 and agg["total"] == 290
        monkeypatch.setattr(st.index, "group_keys_from_attr", real)
        host = Host(gpu, oracle, st, q)
        want = host.buckets(lambda d: d.get("resourceType"), -np.inf)
        assert {b["key"]: (b["doc_count"], (b["top_hit"][0]["doc_id"], b["top_hit"][1])) for b in agg["buckets"]} == want
        check_all(host)
        with pytest.raises(ValueError, match="by must be"):
            hip.semantic_aggregate(q, 0.0, by="color")
        with pytest.raises(ValueError, match="buckets"):
            st.index.set_attr(2, 0, np.array([day("2000-01-01")]))
            hip.semantic_aggregate(q, 0.0, by="chunkDate", interval="day")
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()
