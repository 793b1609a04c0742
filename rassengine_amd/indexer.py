"""``HipIndexer`` — drop-in for the reference's ``OpenSearchIndexer`` (app/main.py:1395-2150) —
and ``store_fhir_docs_in_opensearch`` / ``ensure_index_exists`` for the write side
(app/main.py:350-579, 1211-1282).

What moves to the GPU and what stays:

* the four knn-bearing builders are answered here: ``semantic_search`` (1527-1560), ``hybrid_search``
  (knn clause 1595, boost 2.0), ``hybrid_structured_search`` (1754, boost 2.0, ``term: doc_type =
  structured`` 1765) and ``multi_intent_search`` (2003, boost 1.5) — exact cosine over the HBM index;
* ``has_any_data`` (1470-1478) is answered from the host-side maps;
* the eight BM25 / aggregate builders (``exact_match_search`` 1480, ``structured_search`` 1617,
  ``aggregate_search`` 1777, ``comparison_search`` 1810, ``temporal_search`` 1866, ``explanatory_search``
  1920, ``entity_specific_search`` 2029, ``document_fetch_search`` 2120) are Lucene text search: every
  attribute this class does not define is DELEGATED to a lazily built instance of the module's own
  ``OpenSearchIndexer`` (``install()`` keeps it), so ``ask()``'s 11-entry method table (2855-2867) and the
  DOCUMENT_FETCH branch (2805) keep working.  When a text engine is kept, the BM25 ``should`` clauses of
  the three hybrid builders are fetched from it and summed with the knn sub-score by ``doc_id``.

Same names, argument meaning and error behaviour as the reference:

* ``OpenSearchIndexer(client, index_name)`` is built per request (2802) -> construction is O(1);
* every knn-bearing method returns ``[(doc_dict, float(score))]`` best first, ``[]`` on an empty query
  embedding / blank query text (1534, 1570, 1712, 1970) and on ANY exception (log + ``[]``, 1558-1560);
* ``ask()`` passes ``query=`` to ``semantic_search`` too (2879-2885), which the reference's own signature
  does not accept (TypeError -> HTTP 500): accepted and ignored here;
* the query is re-normalised with ``e / (||e|| + 1e-9)`` (1536-1537) — on the GPU; only row 0 is searched
  (``[0].tolist()``);
* ``patient_id`` -> ``term: patientId`` (1549) as an exact PRE-filter on the row tag; ``k`` is passed
  through as is (k > 32 is served in passes; nothing is clamped);
* ``filter_clause``: ``ask()`` passes the NER entity list there (2770), which makes the reference's query
  malformed.  Tolerated, not replicated: only ``{"term": {"patientId": ...}}`` /
  ``{"term": {"doc_type": ...}}`` dicts are honoured, anything else is ignored;
* quirk 3 (``hybrid_structured_search`` raises ``KeyError`` without filter / patient, 1764): not
  replicated — the ``doc_type`` filter is applied on its own;
* ``_score``: OpenSearch k-NN cosinesimil reports ``1 / (2 - cos)`` (unverified offline, so
  configurable: ``RASS_SCORE_MODE=opensearch|cosine``); a knn ``should`` clause contributes
  ``boost * _score``.  ``ask()`` never reads it.
"""
from __future__ import annotations

import asyncio
import inspect
import logging
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from . import config, prefetch
from .docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_DOCTYPE_SHIFT, TAG_PATIENT_MASK, IndexState

logger = logging.getLogger("rassengine_amd")

TOP_K = config.TOP_K

# the reference's knn boosts
BOOST_HYBRID = 2.0             # app/main.py:1595
BOOST_HYBRID_STRUCTURED = 2.0  # app/main.py:1754
BOOST_MULTI_INTENT = 1.5       # app/main.py:2003
# how much deeper than k the two ranked lists are read before they are fused by doc_id
FUSION_OVERFETCH = 4
# semantic_search_recent sorts by an fp32 copy of an int32 field: exact for |v| < 2^24, and +-2^24 stands for "no value"
RECENT_MAX_ABS = float(1 << 24)


def _score_out(cos: float, mode: Optional[str] = None) -> float:
    mode = mode or config.RASS_SCORE_MODE
    if mode == "cosine":
        return float(cos)
    return float(1.0 / (2.0 - float(cos)))  # OpenSearch k-NN cosinesimil: 1 / (1 + (1 - cos))


def _cos_of_score(score: float, mode: Optional[str] = None) -> float:
    """The inverse of ``_score_out``: the cosine a reported score stands for.  OpenSearch scores lie in [1/3, 1]: a bound at
    or below 0 is below every row (-inf), one above 1 names a cosine no row reaches."""
    mode = mode or config.RASS_SCORE_MODE
    score = float(score)
    if mode == "cosine" or score != score:
        return score
    if score <= 0.0:
        return float("-inf")
    return 2.0 - 1.0 / score


def _term_from_filter(filter_clause: Any, field: str) -> Optional[Any]:
    if isinstance(filter_clause, dict):
        term = filter_clause.get("term")
        if isinstance(term, dict) and field in term:
            return term[field]
    return None


LAYOUT_ATTEMPTS = 8   # searches tried before giving up on an index that is compacted during every one of them


def _layout_epoch(index: Any) -> int:
    """Compactions the index has been through (``FlatIndex.layout_epoch``; 0 for an index that cannot compact)."""
    return int(getattr(index, "layout_epoch", 0))


def _empty(query_emb) -> bool:
    return query_emb is None or np.size(query_emb) == 0


MAX_VALUE_SPAN = 1 << 20        # group by value on an int / date field: max - min + 1 may not exceed FlatIndex.MAX_GROUPS
MAX_HISTOGRAM_BUCKETS = 4096    # = RASS_MAX_KEY_EDGES - 1
CALENDAR_INTERVALS = ("day", "week", "month", "year")
_EPOCH_ORDINAL = 719163         # datetime.date(1970, 1, 1).toordinal()


def _day_date(day: int):
    import datetime as _dt
    return _dt.date.fromordinal(_EPOCH_ORDINAL + int(day))


def histogram_edges(lo: int, hi: int, interval: Any, kind: str) -> List[int]:
    """The ascending bucket edges of a ``histogram`` (``interval`` an int >= 1: buckets ``[m * interval, (m + 1) * interval)``,
    as OpenSearch keys them) or a ``date_histogram`` (``"day" | "week" | "month" | "year"`` on a date field, days since
    1970-01-01 UTC; weeks start on Monday) that cover the values ``lo .. hi``: the first edge is <= lo, the last > hi.  More
    than 4 096 buckets, or edges outside int32, raise ``ValueError``."""
    lo, hi = int(lo), int(hi)
    if isinstance(interval, str):
        if kind != "date" or interval not in CALENDAR_INTERVALS:
            raise ValueError(f"interval must be an int >= 1, or one of {CALENDAR_INTERVALS} on a date field, not {interval!r}")
        if interval == "day":
            step, first = 1, lo
        elif interval == "week":
            step, first = 7, lo - (lo + 3) % 7      # 1970-01-01 was a Thursday: Monday = day -3
        else:
            a, b = _day_date(lo), _day_date(hi)
            months = 1 if interval == "month" else 12
            m0 = (a.year * 12 + a.month - 1) // months * months       # months since year 0 of the first bucket's first day
            n = ((b.year * 12 + b.month - 1) - m0) // months + 1
            if n > MAX_HISTOGRAM_BUCKETS:
                raise ValueError(f"{n} {interval} buckets between the smallest and the largest value: at most {MAX_HISTOGRAM_BUCKETS}")
            return [type(a)(divmod(m0 + j * months, 12)[0], divmod(m0 + j * months, 12)[1] + 1, 1).toordinal() - _EPOCH_ORDINAL
                    for j in range(n + 1)]
    else:
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or int(interval) < 1:
            raise ValueError(f"interval must be an int >= 1, or one of {CALENDAR_INTERVALS} on a date field, not {interval!r}")
        step = int(interval)
        first = lo // step * step
    n = (hi - first) // step + 1
    if n > MAX_HISTOGRAM_BUCKETS:
        raise ValueError(f"{n} buckets of {interval!r} between the smallest and the largest value: at most {MAX_HISTOGRAM_BUCKETS}")
    if first < -(1 << 31) + 1 or first + n * step > (1 << 31) - 1:
        raise ValueError(f"the buckets of {interval!r} over [{lo}, {hi}] reach beyond int32")
    return [first + j * step for j in range(n + 1)]


class _GroupBy:
    """How one collapse / aggregation call groups its rows: by a bit field of the tag (``tag_mask``: the tag-keyed native
    calls, as before attribute columns could group) or by a key column built per attempt (``keys(st)``)."""

    def __init__(self, what: str, field: Any, st: Optional[IndexState], interval: Any = None):
        self.field, self.interval = field, interval
        self.tag_mask = {"patientId": TAG_PATIENT_MASK, "doc_type": TAG_DOCTYPE_MASK}.get(field) if isinstance(field, str) else None
        self.col = self.kind = None
        if self.tag_mask is None:
            found = st.attrs.column(field) if st is not None and isinstance(field, str) and getattr(st, "attrs", None) else None
            if found is None:
                raise ValueError(f"{what} must be 'patientId', 'doc_type' or an attribute field of the index, not {field!r}")
            self.col, self.kind = found
        if interval is not None and self.kind not in ("int", "date"):
            raise ValueError(f"interval needs an int or date attribute field, and {field!r} is not one")

    def tag_names(self, st: IndexState) -> List[str]:
        return (st.patients if self.field == "patientId" else st.doc_types).names()

    def keys(self, st: IndexState):
        """(device key column, n_groups, label) for the index as it is now, or None when no live row has a value; label(g) ->
        the bucket's ``key``.  Called under ``st.lock``."""
        index = st.index
        if self.tag_mask is not None:          # the tag's own field: one pass over the tags on the device
            names = self.tag_names(st)
            return index.group_keys_from_tag(self.tag_mask), len(names) + 1, lambda g: names[g - 1] if g > 0 else None
        if self.kind == "keyword":             # key = code, 0 = the rows without the field
            names = st.attrs.dicts[self.field].names()
            return index.group_keys_from_attr(self.col, base=0, missing=0), len(names) + 1, lambda g: names[g - 1] if g > 0 else None
        lo, hi, present = index.attr_minmax(self.col)
        if not present:                        # no live row has a value
            if self.interval is not None:      # ... and a histogram counts only rows that have one
                return None
            return index.group_keys_from_attr(self.col, base=0, missing=0), 1, lambda g: None     # one group: None
        as_key = (lambda v: v) if self.kind == "int" else (lambda v: _day_date(v).isoformat())
        if self.interval is None:              # by value: key = value - min, the rows without the field in one more group
            if hi - lo + 1 > MAX_VALUE_SPAN:
                raise ValueError(f"{self.field!r} spans {hi - lo + 1} values ({lo} .. {hi}): at most {MAX_VALUE_SPAN} "
                                 "can be grouped by value (use interval=)")
            span = hi - lo + 1
            if span == MAX_VALUE_SPAN:         # the table is full of values: no slot is left for the rows without the field
                return index.group_keys_from_attr(self.col, base=lo, missing=-1), span, lambda g: as_key(lo + g)
            return (index.group_keys_from_attr(self.col, base=lo, missing=span), span + 1,
                    lambda g: as_key(lo + g) if g < span else None)
        edges = histogram_edges(lo, hi, self.interval, self.kind)
        return (index.group_keys_from_attr(self.col, missing=-1, edges=np.asarray(edges, dtype=np.int64)), len(edges) - 1,
                lambda g: edges[g])


class HipIndexer:
    """Exact cosine k-NN over the HBM-resident index named ``index_name``; everything that is not
    k-NN is delegated to the original ``OpenSearchIndexer`` (``_original_cls``, set by ``install``)."""

    _original_cls: Optional[type] = None

    def __init__(self, client: Any = None, index_name: str = ""):
        self.client = client          # handed to the delegate; the k-NN path has no HTTP hop any more
        self.index_name = index_name
        self._delegate = None

    # ------------------------------------------------------------------ delegation (BM25 builders)
    def _original(self):
        if self._delegate is None:
            cls = type(self)._original_cls
            if cls is None:
                return None
            self._delegate = cls(self.client, self.index_name)
        return self._delegate

    def __getattr__(self, name: str):
        # only reached for attributes this class does not define: the 8 text / aggregate builders,
        # text_fields / keyword_fields / date_fields, ...
        if name.startswith("_"):
            raise AttributeError(name)
        orig = self._original()
        if orig is None:
            raise AttributeError(
                f"{type(self).__name__!s} has no attribute {name!r}: it is one of the reference's text-search "
                "builders and no original OpenSearchIndexer was kept (use rassengine_amd.indexer.install(module))")
        return getattr(orig, name)

    def _text_engine(self):
        """The delegate, when it can actually reach a text engine (a client was given)."""
        return self._original() if self.client else None

    # ------------------------------------------------------------------ app/main.py:1470-1478
    def has_any_data(self) -> bool:
        try:
            st = REGISTRY.get(self.index_name, create=False)
            return st is not None and st.live_count() > 0
        except Exception:
            return False

    # ------------------------------------------------------------------ app/main.py:1527-1560
    def semantic_search(self, query_emb: np.ndarray, k: int = TOP_K, filter_clause: Optional[Dict] = None,
                        patient_id: Optional[str] = None, query: Optional[str] = None, **_ignored
                        ) -> List[Tuple[Dict, float]]:
        if _empty(query_emb):
            return []
        try:
            return self._knn(query_emb, k, filter_clause, patient_id, boost=1.0)
        except Exception as e:  # reference: log and return [] (1558-1560)
            logger.error(f"Semantic search error: {e}")
            return []

    def semantic_search_above(self, query_emb: np.ndarray, min_score: float, limit: int = 256,
                              filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None
                              ) -> Tuple[List[Tuple[Dict, float]], int]:
        """The radial form of the k-NN clause (``min_score`` instead of ``k``): every chunk whose score is at least
        ``min_score`` and how many there are, in one pass over the index (``FlatIndex.search_range``).  ``min_score`` is in
        the units ``semantic_search`` returns (``RASS_SCORE_MODE``) and is converted to a cosine once.  Returns
        ``(hits, total)``: ``[(doc_dict, float(score))]`` best first, at most ``limit`` (<= 4096) of them, and the exact
        number of matching rows, which may exceed ``limit``.  Filters as ``semantic_search``.  An empty embedding or an
        unindexed patient gives ``([], 0)``; errors raise (this method has no counterpart in the reference to mirror)."""
        if _empty(query_emb):
            return [], 0
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return [], 0
        prep = self._prepare(st, query_emb, limit, filter_clause, patient_id, None)
        if prep is None:
            return [], 0
        q, limit_eff, (fval, fmask) = prep
        thr = np.array([_cos_of_score(min_score)], dtype=np.float32)
        if np.isnan(thr[0]):
            raise ValueError("min_score must not be NaN")
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        for _ in range(LAYOUT_ATTEMPTS):    # row ids belong to one layout of the index, as in _knn
            layout = _layout_epoch(st.index)
            scores, ids, totals = st.index.search_range(q, thr, max_hits=limit_eff, **flt)
            hits = self._hits(st, scores[0], ids[0], 1.0, None, layout)
            if hits is not None:
                return hits, int(totals[0])
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_search_collapsed(self, query_emb: np.ndarray, k: int = TOP_K, collapse: str = "patientId",
                                  filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                                  where: Optional[Any] = None) -> Tuple[List[Tuple[Dict, float]], int]:
        """The k-NN clause under ``"collapse": {"field": collapse}``: the best chunk of every distinct value of
        ``collapse`` — ``patientId``, ``doc_type`` or any attribute field of the index (``config.RASS_ATTR_FIELDS``: a
        keyword, int or date column) — the k best of those, in one pass over the index whatever k is
        (``FlatIndex.search_grouped``; for an attribute field ``FlatIndex.search_grouped_by_keys`` over a key column built
        from the field's column on the GPU).  Returns ``(hits, total_groups)``: ``[(doc_dict, float(score))]`` best first in
        ``semantic_search``'s score units, and the exact number of distinct values among the matching chunks (chunks
        without the field count as one value, as OpenSearch collapses missing values together).  An int or date field is
        grouped by value and may span at most 1 048 576 values.  ``where``: an OpenSearch filter as
        ``semantic_search_filtered`` takes it, compiled into a bitmap the scan honours (dim <= 1024; the whole index is
        still streamed).  Filters as ``semantic_search``.  An empty embedding or an unindexed patient gives ``([], 0)``;
        errors raise (this method has no counterpart in the reference to mirror)."""
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        by = _GroupBy("collapse", collapse, st)
        if _empty(query_emb):
            return [], 0
        if st is None:
            return [], 0
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, None)
        if prep is None:
            return [], 0
        q, k_eff, (fval, fmask) = prep
        if not hasattr(st.index, "search_grouped"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no grouped search "
                                      "(IVF-backed and sharded indices cannot collapse; use a flat fp32 index)")
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        if by.tag_mask is None or where is not None:
            self._need_keys(st, where, "grouped search")
        for _ in range(LAYOUT_ATTEMPTS):    # row ids belong to one layout of the index, as in _knn
            layout = _layout_epoch(st.index)
            if by.tag_mask is not None and where is None:       # the tag path, call for call
                # codes run 1 .. len, 0 = none; read per attempt: a concurrent ingest may have added a value
                n_groups = len(st.patients if collapse == "patientId" else st.doc_types) + 1
                scores, ids, _groups, totals = st.index.search_grouped(q, k_eff, by.tag_mask, n_groups, **flt)
            else:
                built = self._keys_and_bitmap(st, by, where, layout)
                if built is None:
                    continue
                keyed, allow = built
                if keyed is None:
                    return [], 0
                scores, ids, _groups, totals = st.index.search_grouped_by_keys(q, k_eff, keyed[0], keyed[1], allow=allow, **flt)
            hits = self._hits(st, scores[0], ids[0], 1.0, None, layout)
            if hits is not None:
                return hits, int(totals[0])
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_search_collapsed_hits(self, query_emb: np.ndarray, k: int = TOP_K, collapse: str = "patientId",
                                       inner_hits: int = 3, filter_clause: Optional[Dict] = None,
                                       patient_id: Optional[str] = None, where: Optional[Any] = None
                                       ) -> Tuple[List[List[Tuple[Dict, float]]], int]:
        """``semantic_search_collapsed`` with ``"inner_hits": {"size": inner_hits}``: the ``inner_hits`` (1 .. 16) best chunks
        of each of the k best values of ``collapse``, in one pass over the index whatever ``inner_hits`` is
        (``FlatIndex.search_group_hits``).  Returns ``(groups, total_groups)``: ``groups[j]`` is a best-first list of
        ``(doc_dict, float(score))`` — ``groups[j][0]`` is what ``semantic_search_collapsed`` returns at position j, a value
        with fewer matching chunks has a shorter list — and the exact number of distinct values among the matching chunks.
        ``collapse``, ``where`` and the filters as in ``semantic_search_collapsed``; every field, ``patientId`` and
        ``doc_type`` included, goes through a key column built on the GPU.  fp32 flat indices with dim <= 1024.  An empty
        embedding or an unindexed patient gives ``([], 0)``; errors raise."""
        def finish(st, out, layout):
            scores, ids, _groups, totals = out[:4]
            groups: List[List[Tuple[Dict, float]]] = []
            for j in range(scores.shape[1]):
                if ids[0, j, 0] < 0:
                    break
                hits = self._hits(st, scores[0, j], ids[0, j], 1.0, None, layout)
                if hits is None:
                    return None
                if hits:
                    groups.append(hits)
            return groups, int(totals[0])
        got = self._group_hits("collapse", query_emb, k, collapse, inner_hits, filter_clause, patient_id, where, False, finish)
        return ([], 0) if got is None else got

    def semantic_search_capped(self, query_emb: np.ndarray, k: int = TOP_K, per: str = "patientId", max_per_group: int = 1,
                               filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                               where: Optional[Any] = None) -> List[Tuple[Dict, float]]:
        """The k best chunks with at most ``max_per_group`` (1 .. 16) of them from any one value of ``per`` — the usual way
        to keep one long document from filling a context window — exactly, in one pass over the index
        (``FlatIndex.search_group_hits`` with ``capped=True``; needs ``k * max_per_group <= 4096``).  ``per``, ``where`` and
        the filters as ``collapse`` in ``semantic_search_collapsed``.  Returns ``[(doc_dict, float(score))]`` best first in
        ``semantic_search``'s score units.  An empty embedding or an unindexed patient gives ``[]``; errors raise."""
        got = self._group_hits("per", query_emb, k, per, max_per_group, filter_clause, patient_id, where, True,
                               lambda st, out, layout: self._hits(st, out[4][0], out[5][0], 1.0, None, layout))
        return [] if got is None else got

    def _group_hits(self, what, query_emb, k, field, group_size, filter_clause, patient_id, where, capped, finish):
        """What the two methods above share: the key column (and bitmap) and ``FlatIndex.search_group_hits`` under one layout
        epoch per attempt, as ``semantic_search_collapsed`` runs its keyed path; ``finish(st, out, layout)`` maps the ids (None:
        a compaction landed, search again).  None: the empty answer."""
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        by = _GroupBy(what, field, st)
        if _empty(query_emb) or st is None:
            return None
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, None)
        if prep is None:
            return None
        q, k_eff, (fval, fmask) = prep
        if not hasattr(st.index, "search_group_hits"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no grouped search with inner hits "
                                      "(IVF-backed and sharded indices cannot collapse; use a flat fp32 index)")
        if int(getattr(st.index, "dim", 0)) > 1024:
            raise NotImplementedError(f"{self.index_name}: the grouped search with inner hits needs dim <= 1024 (no wide-row form)")
        self._need_keys(st, where, "grouped search")
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        for _ in range(LAYOUT_ATTEMPTS):    # row ids belong to one layout of the index, as in _knn
            layout = _layout_epoch(st.index)
            built = self._keys_and_bitmap(st, by, where, layout)
            if built is None:
                continue
            keyed, allow = built
            if keyed is None:
                return None
            out = st.index.search_group_hits(q, k_eff, keyed[0], keyed[1], int(group_size), allow=allow, capped=capped, **flt)
            got = finish(st, out, layout)
            if got is not None:
                return got
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def _need_keys(self, st: IndexState, where: Any, what: str) -> None:
        """The refusals of a key-column call, before anything is built."""
        index = st.index
        if not all(hasattr(index, m) for m in ("search_grouped_by_keys", "search_counts_by_keys", "group_keys_from_attr", "group_keys_from_tag", "attr_minmax")):
            raise NotImplementedError(f"{self.index_name}: {type(index).__name__} has no {what} over a key column "
                                      "(IVF-backed and sharded indices cannot group by an attribute field; use a flat fp32 index)")
        if where is not None:
            if not hasattr(index, "allow_from_attr_clauses"):
                raise NotImplementedError(f"{self.index_name}: {type(index).__name__} has no filtered search "
                                          "(IVF-backed and sharded indices cannot restrict by a bitmap; use a flat fp32 index)")
            if int(getattr(index, "dim", 0)) > 1024:
                raise NotImplementedError(f"{self.index_name}: where= with a {what} needs dim <= 1024 (the bitmap forms of the "
                                          "scan serve narrow rows only)")

    @staticmethod
    def _keys_and_bitmap(st: IndexState, by: "_GroupBy", where: Any, layout: int):
        """The key column and the bitmap of one attempt, built under the state's lock and ONE layout epoch, exactly as
        ``semantic_search_filtered`` builds its bitmap: ``((keys, n_groups, label) or None, allow or None)``; None when a
        compaction landed first (try again)."""
        from .attrfilter import compile_filter, run_plan
        with st.lock:
            if _layout_epoch(st.index) != layout:
                return None
            keyed = by.keys(st)
            allow = None
            if where is not None and keyed is not None:
                allow = run_plan(st.index, compile_filter(where, st.attrs, st.patients, st.doc_types))
        return keyed, allow

    def semantic_search_diverse(self, query_emb: np.ndarray, k: int = TOP_K, fetch_k: Optional[int] = None,
                                lambda_mult: float = 0.5, filter_clause: Optional[Dict] = None,
                                patient_id: Optional[str] = None) -> List[Tuple[Dict, float]]:
        """``semantic_search`` with maximal-marginal-relevance re-ranking (``FlatIndex.search_mmr``): of the exact top
        ``fetch_k`` chunks (default ``min(128, max(4 k, 16))``) the k that a greedy selection picks, each time the chunk
        with the largest ``lambda_mult * cos(query, chunk) - (1 - lambda_mult) * max cos(chunk, picked)``: near-identical
        chunks (a re-issued condition, a note uploaded twice) do not fill the answer while different ones remain among
        the candidates.  ``lambda_mult`` in [0, 1]: 1 is ``semantic_search``, 0 diversity alone.  Returns
        ``[(doc_dict, float(score))]`` in selection order (NOT score order); scores are the chunk's similarity to the
        query in ``semantic_search``'s units (``RASS_SCORE_MODE``).  Filters as ``semantic_search``.  An empty embedding or
        an unindexed patient gives ``[]``; errors raise (this method has no counterpart in the reference to mirror)."""
        if _empty(query_emb):
            return []
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return []
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, None)
        if prep is None:
            return []
        q, k_eff, (fval, fmask) = prep
        if not hasattr(st.index, "search_mmr"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no diversified (MMR) search "
                                      "(IVF-backed and sharded indices cannot re-rank on the device; use a flat fp32 index)")
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        for _ in range(LAYOUT_ATTEMPTS):    # row ids belong to one layout of the index, as in _knn
            layout = _layout_epoch(st.index)
            scores, ids, _ranks = st.index.search_mmr(q, k_eff, fetch_k=fetch_k, lambda_mult=float(lambda_mult), **flt)
            hits = self._hits(st, scores[0], ids[0], 1.0, None, layout)
            if hits is not None:
                return hits
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_aggregate(self, query_emb: np.ndarray, min_score: float, by: str = "patientId", size: int = 5,
                           filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                           interval: Optional[Any] = None, where: Optional[Any] = None, top_hits: int = 1,
                           order: str = "_count") -> Dict[str, Any]:
        """A ``terms`` aggregation on ``by`` (``"patientId"``, ``"doc_type"`` or any attribute field of the index:
        ``conditionCodeText``, ``resourceType``, a date) under the k-NN clause with a ``min_score``:
        how many chunks score at least ``min_score``, of how many distinct values, and the ``size`` values with the most such
        chunks, in one pass over the index (``FlatIndex.search_counts``).  ``min_score`` is in the units ``semantic_search``
        returns (``RASS_SCORE_MODE``) and is converted to a cosine once.  Returns the shape of an OpenSearch ``terms``
        aggregation with two additions::

            {"buckets": [{"key": value (None: chunks without the field), "doc_count": int,
                          "top_hit": (doc_dict, float(score))}, ...],       # doc_count desc, then first-indexed value first
             "sum_other_doc_count": total - the listed doc_counts,
             "cardinality": distinct values among the hits, "total": hits}

        An attribute field goes through a key column built from its column on the GPU (``FlatIndex.search_counts_by_keys``);
        an int or date field is grouped by value (at most 1 048 576 values between its smallest and largest).

        ``interval`` (an int or date field only) makes it OpenSearch's ``histogram`` / ``date_histogram`` instead: an int
        (units, or days on a date field), or ``"day" | "week" | "month" | "year"`` on a date field (UTC calendar, weeks from
        Monday).  Every non-empty bucket (``min_doc_count = 1``) comes back in KEY order — ``size`` is not used —, each
        ``{"key": lower edge (first day), "key_as_string": ISO date (date fields), "doc_count", "top_hit"}``; chunks
        without the field are not counted; more than 4 096 buckets between the smallest and the largest value raise
        ``ValueError``.

        ``top_hits`` (1 .. 16) and ``order`` (``"_count"`` | ``"max_score"``): OpenSearch's ``top_hits {size: n}``
        sub-aggregation and ``"order": {"max_score": "desc"}``.  With ``top_hits > 1`` or ``order="max_score"`` every ``by``,
        ``patientId`` and ``doc_type`` included, goes through a key column built on the GPU and ONE pass keeps the counts and
        each bucket's best chunks together (``FlatIndex.search_counts_hits_by_keys``; fp32 flat indices with dim <= 1024);
        each bucket gains ``"top_hits": [(doc_dict, float(score)), ...]`` best first, at most ``top_hits`` of them, and
        ``"top_hit"`` is the first.  ``"max_score"`` lists the ``size`` buckets with the best chunk instead of those with the
        most; with ``interval`` it raises ``ValueError`` (a histogram stays in key order).

        ``where``: an OpenSearch filter as ``semantic_search_filtered`` takes it (a date range, a ``term``), compiled into
        a bitmap the scan honours (dim <= 1024; the whole index is still streamed).  Filters as ``semantic_search``.  An
        empty embedding or an unindexed patient gives the empty aggregation with zeros; errors raise (this method has no
        counterpart in the reference to mirror: ``aggregate_search`` ignores the query text and stays with the text
        engine)."""
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        grp = _GroupBy("by", by, st, interval)
        if isinstance(top_hits, bool) or not isinstance(top_hits, (int, np.integer)) or not 1 <= int(top_hits) <= 16:
            raise ValueError(f"top_hits must be an int in [1, 16], not {top_hits!r}")
        if order not in ("_count", "max_score"):
            raise ValueError(f"order must be '_count' or 'max_score', not {order!r}")
        if order == "max_score" and interval is not None:
            raise ValueError("order='max_score' cannot go with interval=: a histogram stays in key order")
        with_hits = int(top_hits) > 1 or order == "max_score"
        empty = {"buckets": [], "sum_other_doc_count": 0, "cardinality": 0, "total": 0}
        if _empty(query_emb):
            return empty
        if st is None:
            return empty
        prep = self._prepare(st, query_emb, size, filter_clause, patient_id, None)
        if prep is None:
            return empty
        q, size_eff, (fval, fmask) = prep
        if not hasattr(st.index, "search_counts"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no aggregation "
                                      "(IVF-backed and sharded indices cannot count per group; use a flat fp32 index)")
        thr = np.array([_cos_of_score(min_score)], dtype=np.float32)
        if np.isnan(thr[0]):
            raise ValueError("min_score must not be NaN")
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        if with_hits:
            if not hasattr(st.index, "search_counts_hits_by_keys"):
                raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no aggregation with top hits "
                                          "(IVF-backed and sharded indices cannot count per group; use a flat fp32 index)")
            if int(getattr(st.index, "dim", 0)) > 1024:
                raise NotImplementedError(f"{self.index_name}: the aggregation with top hits needs dim <= 1024 (no wide-row form)")
        if with_hits or grp.tag_mask is None or where is not None:
            self._need_keys(st, where, "aggregation")
        for _ in range(LAYOUT_ATTEMPTS):    # top_hit ids belong to one layout of the index, as in _knn
            layout = _layout_epoch(st.index)
            if grp.tag_mask is not None and where is None and not with_hits:      # the tag path, call for call
                # codes run 1 .. len, 0 = none; read per attempt: a concurrent ingest may have added a value
                names = grp.tag_names(st)
                label = lambda g, names=names: names[g - 1] if g > 0 else None
                groups, counts, scores, ids, n_buckets, totals = st.index.search_counts(q, thr, size_eff, grp.tag_mask,
                                                                                        len(names) + 1, **flt)
            else:
                built = self._keys_and_bitmap(st, grp, where, layout)
                if built is None:
                    continue
                keyed, allow = built
                if keyed is None:
                    return empty
                keys, n_groups, label = keyed
                # a histogram lists every bucket: the select is asked for all of them and the host puts them in key order
                ask = n_groups if interval is not None else size_eff
                if with_hits:       # scores / ids are [1, ask, top_hits]: a bucket's best chunks, best first
                    groups, counts, scores, ids, n_buckets, totals = st.index.search_counts_hits_by_keys(
                        q, thr, ask, keys, n_groups, int(top_hits), order, allow=allow, **flt)
                else:
                    groups, counts, scores, ids, n_buckets, totals = st.index.search_counts_by_keys(q, thr, ask, keys, n_groups,
                                                                                                    allow=allow, **flt)
            listed = [(int(g), int(c), j) for j, (g, c) in enumerate(zip(groups[0], counts[0])) if g >= 0]
            if interval is not None:
                listed.sort()
            buckets = []
            for g, c, j in listed:
                top = self._hits(st, scores[0, j] if with_hits else [scores[0, j]], ids[0, j] if with_hits else [ids[0, j]],
                                 1.0, None, layout)
                if top is None:
                    buckets = None
                    break
                bucket = {"key": label(g), "doc_count": c, "top_hit": top[0] if top else None}
                if with_hits:
                    bucket["top_hits"] = top
                if interval is not None and grp.kind == "date":
                    bucket["key_as_string"] = _day_date(bucket["key"]).isoformat()
                buckets.append(bucket)
            if buckets is not None:
                total = int(totals[0])
                return {"buckets": buckets, "sum_other_doc_count": total - sum(b["doc_count"] for b in buckets),
                        "cardinality": int(n_buckets[0]), "total": total}
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    STATS_ORDERS = ("_count", "value_count", "min", "max", "sum", "avg")

    def semantic_stats(self, query_emb: np.ndarray, min_score: float, field: str, by: Optional[str] = None, size: int = 5,
                       interval: Optional[Any] = None, order: Optional[Dict[str, str]] = None, where: Optional[Any] = None,
                       filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None) -> Dict[str, Any]:
        """``semantic_aggregate`` with OpenSearch's ``stats`` metric sub-aggregation on ``field`` (an int or date attribute
        field; a keyword raises ``ValueError``: codes have no arithmetic): per bucket also the count, min, max, sum and avg
        of ``field`` over the chunks that score at least ``min_score``, in the same single pass over the index
        (``FlatIndex.search_stats_by_keys``).  ``by=None`` gives the global stats (one bucket, ``key`` None); ``by`` and
        ``interval`` as in ``semantic_aggregate`` (``patientId`` / ``doc_type`` go through a key column built from the tag).
        The result has ``semantic_aggregate``'s shape, each bucket gaining::

            "stats": {"count": chunks with a value, "min", "max", "sum", "avg": float(sum) / float(count)}

        with ``min`` / ``max`` / ``avg`` None where ``count`` is 0, and ``min_as_string`` / ``max_as_string`` (ISO dates) on
        a date field, whose values are days since 1970-01-01.

        ``order``: ``{"_count" | "value_count" | "min" | "max" | "sum" | "avg": "asc" | "desc"}``, default ``_count``
        descending (a histogram without ``order`` stays in key order).  Ties go to the first-indexed value, and buckets
        whose chunks all lack the field come last in both directions.  The first four are ordered on the GPU before the
        ``size`` cut; ``sum`` and ``avg`` are ordered here, which needs every bucket listed: a histogram, or a first answer
        with ``cardinality <= size`` — otherwise ``ValueError``.  ``where`` and the filters as ``semantic_aggregate``.
        IVF-backed and sharded indices raise ``NotImplementedError``; errors raise."""
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        found = st.attrs.column(field) if st is not None and isinstance(field, str) and getattr(st, "attrs", None) else None
        if st is not None and found is None:
            raise ValueError(f"field must be an int or date attribute field of the index, not {field!r}")
        if found is not None and found[1] not in ("int", "date"):
            raise ValueError(f"stats need an int or date attribute field, and {field!r} is a {found[1]} (codes have no arithmetic)")
        order = {"_count": "desc"} if order is None and interval is None else order
        if order is not None and (not isinstance(order, dict) or len(order) != 1 or next(iter(order)) not in self.STATS_ORDERS
                                  or next(iter(order.values())) not in ("asc", "desc")):
            raise ValueError(f"order must be {{one of {self.STATS_ORDERS}: 'asc' | 'desc'}}, not {order!r}")
        grp = _GroupBy("by", by, st, interval) if by is not None else None
        if grp is None and interval is not None:
            raise ValueError("interval needs by=")
        empty = {"buckets": [], "sum_other_doc_count": 0, "cardinality": 0, "total": 0}
        if _empty(query_emb) or st is None:
            return empty
        prep = self._prepare(st, query_emb, size, filter_clause, patient_id, None)
        if prep is None:
            return empty
        q, size_eff, (fval, fmask) = prep
        if not hasattr(st.index, "search_stats_by_keys"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no stats aggregation "
                                      "(IVF-backed and sharded indices cannot aggregate per group; use a flat fp32 index)")
        self._need_keys(st, where, "stats aggregation")
        col, kind = found
        thr = np.array([_cos_of_score(min_score)], dtype=np.float32)
        if np.isnan(thr[0]):
            raise ValueError("min_score must not be NaN")
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        by_name, direction = next(iter(order.items())) if order is not None else ("_count", "desc")
        on_host = by_name in ("sum", "avg")
        for _ in range(LAYOUT_ATTEMPTS):    # top_hit ids belong to one layout of the index, as in _knn
            layout = _layout_epoch(st.index)
            if grp is None:
                from .attrfilter import compile_filter, run_plan
                with st.lock:
                    if _layout_epoch(st.index) != layout:
                        continue
                    allow = run_plan(st.index, compile_filter(where, st.attrs, st.patients, st.doc_types)) if where is not None else None
                keyed = (None, 1, lambda g: None)
            else:
                built = self._keys_and_bitmap(st, grp, where, layout)
                if built is None:
                    continue
                keyed, allow = built
                if keyed is None:
                    return empty
            keys, n_groups, label = keyed
            # a histogram lists every bucket; so does a host-side order, which cannot cut before it has sorted
            ask = n_groups if interval is not None else size_eff
            out = st.index.search_stats_by_keys(q, thr, ask, keys, n_groups, col, "_count" if on_host else by_name,
                                                True if on_host else direction == "desc", allow=allow, **flt)
            groups, counts, scores, ids, vcounts, sums, mins, maxs, n_buckets, totals = out
            if on_host and int(n_buckets[0]) > ask:
                raise ValueError(f"order by {by_name!r} is computed on the host and needs every bucket listed: the answer has "
                                 f"{int(n_buckets[0])} buckets and size is {ask} (use a histogram, a larger size, or order by "
                                 "'_count', 'value_count', 'min' or 'max')")
            listed = [(int(g), int(c), s, i, int(vc), int(sm), int(mn), int(mx)) for g, c, s, i, vc, sm, mn, mx in
                      zip(groups[0], counts[0], scores[0], ids[0], vcounts[0], sums[0], mins[0], maxs[0]) if g >= 0]
            if order is None:
                listed.sort()               # a histogram without an order: key order
            elif on_host:                   # metric asc / desc, ties by key, buckets without a value last in both directions
                sign = 1.0 if direction == "asc" else -1.0
                metric = (lambda b: float(b[5])) if by_name == "sum" else (lambda b: float(b[5]) / float(b[4]))
                listed.sort(key=lambda b: (b[4] == 0, sign * metric(b) if b[4] else 0.0, b[0]))
                listed = listed[:size_eff] if interval is None else listed
            as_string = (lambda v: _day_date(v).isoformat()) if kind == "date" else None
            buckets = []
            for g, c, s, i, vc, sm, mn, mx in listed:
                top = self._hits(st, [s], [i], 1.0, None, layout)
                if top is None:
                    buckets = None
                    break
                stats = {"count": vc, "min": mn if vc else None, "max": mx if vc else None, "sum": sm,
                         "avg": float(sm) / float(vc) if vc else None}
                if as_string is not None:
                    stats["min_as_string"] = as_string(mn) if vc else None
                    stats["max_as_string"] = as_string(mx) if vc else None
                bucket = {"key": label(g), "doc_count": c, "top_hit": top[0] if top else None, "stats": stats}
                if interval is not None and grp.kind == "date":
                    bucket["key_as_string"] = _day_date(bucket["key"]).isoformat()
                buckets.append(bucket)
            if buckets is not None:
                total = int(totals[0])
                return {"buckets": buckets, "sum_other_doc_count": total - sum(b["doc_count"] for b in buckets),
                        "cardinality": int(n_buckets[0]), "total": total}
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_search_within(self, query_emb: np.ndarray, k: int = TOP_K, patient_ids: Optional[List[Any]] = None,
                               doc_types: Optional[List[str]] = None, doc_ids: Optional[List[str]] = None,
                               filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None
                               ) -> List[Tuple[Dict, float]]:
        """The k-NN clause under set-valued restrictions: a ``terms`` filter on ``patientId`` (``patient_ids``) and / or
        ``doc_type`` (``doc_types``), an ``ids`` filter (``doc_ids``: the hit set of a text query, an ACL, a date range
        resolved elsewhere), next to the single-valued ``filter_clause`` / ``patient_id`` of ``semantic_search``.  The
        restrictions given are intersected; a value that was never indexed contributes nothing, an overwritten doc is found
        at its current row only, and an empty intersection gives ``[]``.  With none of the three lists it is
        ``semantic_search`` that raises.  The allowed rows go to the GPU as a bitmap (``FlatIndex.allow_from_rows`` /
        ``allow_from_tag_values``) and the scan reads only the 32-row tiles that hold one (``FlatIndex.search_allowed``):
        every allowed chunk gets its exact cosine, however deep it ranks in the whole index.  Returns ``[(doc_dict,
        float(score))]`` best first in ``semantic_search``'s score units.  Errors raise (no counterpart in the reference)."""
        if _empty(query_emb):
            return []
        if patient_ids is None and doc_types is None and doc_ids is None:
            return self._knn(query_emb, k, filter_clause, patient_id, boost=1.0)
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return []
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, None)
        if prep is None:
            return []
        q, k_eff, (fval, fmask) = prep
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        if not hasattr(st.index, "search_allowed"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no allow-list search "
                                      "(IVF-backed and sharded indices cannot restrict by a bitmap; use a flat fp32 index)")
        for _ in range(LAYOUT_ATTEMPTS):    # the bitmap and the ids belong to ONE layout of the index: built, searched and mapped under one epoch
            layout = _layout_epoch(st.index)
            with st.lock:
                if _layout_epoch(st.index) != layout:
                    continue
                # known values only: a value that was never indexed matches no row
                p_codes = None if patient_ids is None else sorted({c for c in (st.patients.lookup(p) for p in patient_ids) if c is not None})
                t_codes = None if doc_types is None else sorted({c for c in (st.doc_types.lookup(t) for t in doc_types) if c is not None})
                rows = None
                if doc_ids is not None:
                    rows = sorted({st.doc_row[d] for d in doc_ids if d in st.doc_row})   # keys as add_documents stores them
                    if p_codes is not None or t_codes is not None:   # intersect on the host: the docs carry both fields
                        def keeps(r: int) -> bool:
                            doc = st.row_doc[r] if r < len(st.row_doc) else None
                            return doc is not None and \
                                (p_codes is None or st.patients.lookup(doc.get("patientId")) in p_codes) and \
                                (t_codes is None or st.doc_types.lookup(doc.get("doc_type")) in t_codes)
                        rows = [r for r in rows if keeps(r)]
            if rows is not None:
                if not rows:
                    return []
                allow = st.index.allow_from_rows(np.asarray(rows, dtype=np.int64))
            else:
                if (p_codes is not None and not p_codes) or (t_codes is not None and not t_codes):
                    return []
                mask = (TAG_PATIENT_MASK if p_codes is not None else 0) | (TAG_DOCTYPE_MASK if t_codes is not None else 0)
                values = [p | (t << TAG_DOCTYPE_SHIFT) for p in (p_codes if p_codes is not None else [0])
                          for t in (t_codes if t_codes is not None else [0])]
                allow = st.index.allow_from_tag_values(np.asarray(values, dtype=np.int32), mask)
            # an ingest may append rows between the build and the search (the epoch does not move on an append): the bitmap
            # speaks for the rows it was built over, and search_allowed lets it allow nothing past them
            scores, ids = st.index.search_allowed(q, k_eff, allow, **flt)
            hits = self._hits(st, scores[0], ids[0], 1.0, None, layout)
            if hits is not None:
                return hits
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_search_filtered(self, query_emb: np.ndarray, k: int = TOP_K, where: Optional[Any] = None,
                                 filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None
                                 ) -> List[Tuple[Dict, float]]:
        """The k-NN clause under an OpenSearch ``filter``: ``where`` is a clause (or a list of them, ANDed) of ``term``,
        ``terms``, ``range`` (``gte`` / ``gt`` / ``lte`` / ``lt``), ``exists`` and ``bool`` (``must`` / ``filter`` = and,
        ``should`` = at least one, ``must_not``), nested freely, over ``patientId``, ``doc_type`` and the attribute fields of
        the index (``config.RASS_ATTR_FIELDS``: keyword, int and date columns stored by ``add_documents``).  On a date field
        the bounds are ``YYYY-MM-DD``, ISO-8601 date-times, epoch milliseconds, ``now`` or ``now-N(d|w|M|y)``, compared as
        UTC days (``gt`` / ``lt``: the next / previous day).  A keyword value that was never indexed matches nothing; a
        ``must_not`` passes the chunks that lack the field.  An unknown field or an unsupported clause (``match``, ...)
        raises ``ValueError`` naming it.  The filter is compiled into a few bitmap-builder calls (``attrfilter``), evaluated
        on the GPU over the columns, and the scan reads only the 32-row tiles with an allowed chunk
        (``FlatIndex.search_allowed``): every allowed chunk gets its exact cosine.  ``filter_clause`` / ``patient_id`` as in
        ``semantic_search``, intersected with ``where``.  ``where=None`` is ``semantic_search`` that raises.  Returns
        ``[(doc_dict, float(score))]`` best first in ``semantic_search``'s score units.  Errors raise (no counterpart in the
        reference)."""
        if _empty(query_emb):
            return []
        if where is None:
            return self._knn(query_emb, k, filter_clause, patient_id, boost=1.0)
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return []
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, None)
        if prep is None:
            return []
        q, k_eff, (fval, fmask) = prep
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        if not hasattr(st.index, "search_allowed") or not hasattr(st.index, "allow_from_attr_clauses"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no filtered search "
                                      "(IVF-backed and sharded indices cannot restrict by a bitmap; use a flat fp32 index)")
        from .attrfilter import compile_filter, run_plan
        for _ in range(LAYOUT_ATTEMPTS):    # the bitmap and the ids belong to ONE layout of the index, as in semantic_search_within
            layout = _layout_epoch(st.index)
            # under the state's lock: the dictionaries are read as one, and no row sits between its append and its column
            # values (add_documents holds the lock across both), where a negated clause would pass it as "missing"
            with st.lock:
                if _layout_epoch(st.index) != layout:
                    continue
                plan = compile_filter(where, st.attrs, st.patients, st.doc_types)
                allow = run_plan(st.index, plan)
            scores, ids = st.index.search_allowed(q, k_eff, allow, **flt)
            hits = self._hits(st, scores[0], ids[0], 1.0, None, layout)
            if hits is not None:
                return hits
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_search_boosted(self, query_emb: np.ndarray, k: int = TOP_K, boost: float = 1.0,
                                text_hits: Optional[List[Tuple[Any, float]]] = None, should: Optional[List[Tuple[Dict, float]]] = None,
                                where: Optional[Any] = None, filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                                doc_type: Optional[str] = None, score_mode: Optional[str] = None) -> List[Tuple[Dict, float]]:
        """A ``bool.should`` around the k-NN clause, answered exactly: the top ``k`` chunks by ``boost * knn_score + the sum of
        what the other clauses are worth for the chunk`` over EVERY chunk of the index (``FlatIndex.search_boosted``), not
        over two ranked lists cut at some depth.  ``text_hits``: ``[(doc | doc_id, score)]`` from a text engine, resolved
        through ``doc_id -> row``; unknown or deleted ids are ignored, repeated ids are summed (fp32, list order).
        ``should``: ``[(leaf filter, weight)]`` with ``term`` / ``terms`` / ``range`` (date math as in a filter) / ``exists``
        leaves over the attribute fields (``attrfilter.compile_should``); weights of any sign.  ``where``: a filter as
        ``semantic_search_filtered`` takes it; the chunks it excludes never rank.  ``filter_clause`` / ``patient_id`` /
        ``doc_type`` as in ``semantic_search``.  ``knn_score`` is in ``score_mode``'s units (default ``RASS_SCORE_MODE``).
        Returns ``[(doc_dict, float(fused))]`` best first; ``[]`` on an empty embedding or on any exception (logged)."""
        if _empty(query_emb):
            return []
        try:
            return self._boosted(query_emb, k, boost, text_hits, should, where, filter_clause, patient_id, doc_type, score_mode)
        except Exception as e:
            logger.error(f"Boosted search error: {e}")
            return []

    def _boosted(self, query_emb, k, boost, text_hits, should, where, filter_clause, patient_id, doc_type, score_mode
                 ) -> List[Tuple[Dict, float]]:
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return []
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, doc_type)
        if prep is None:
            return []
        q, k_eff, (fval, fmask) = prep
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        if not hasattr(st.index, "search_boosted"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no boosted search "
                                      "(sharded indices cannot rank by a bonus column; use a flat fp32 index)")
        boost = float(boost)
        if not np.isfinite(boost):
            raise ValueError(f"boost must be finite, got {boost!r}")
        transform = "raw" if (score_mode or config.RASS_SCORE_MODE) == "cosine" else "opensearch"
        from .attrfilter import MAX_CLAUSES, compile_filter, compile_should, run_plan
        for _ in range(LAYOUT_ATTEMPTS):    # the column and the ids belong to ONE layout of the index, as in semantic_search_within
            layout = _layout_epoch(st.index)
            # under the state's lock from the first cell to the search: no row is appended in between (add_documents takes
            # the lock), so no chunk slips past `where` with the zero bonus of a row the column has not seen
            with st.lock:
                if _layout_epoch(st.index) != layout:
                    continue
                rows, values = self._text_rows(st, text_hits)
                clauses = compile_should(should, st.attrs, st.patients, st.doc_types)
                bonus = st.index.new_bonus()
                if rows:
                    st.index.bonus_scatter(bonus, None, rows, values)
                for i in range(0, len(clauses), MAX_CLAUSES):
                    chunk = clauses[i:i + MAX_CLAUSES]
                    st.index.bonus_from_attr_clauses(bonus, [(0, c, lo, hi, neg) for c, lo, hi, neg, _ in chunk],
                                                     [w for *_, w in chunk], op="add")
                if where is not None:
                    st.index.bonus_mask(bonus, run_plan(st.index, compile_filter(where, st.attrs, st.patients, st.doc_types)))
                scores, ids = st.index.search_boosted(q, k_eff, bonus, boost=boost, transform=transform, **flt)
                out: List[Tuple[Dict, float]] = []
                for s, row in zip(scores[0], ids[0]):
                    if row < 0:
                        break
                    doc = st.row_doc[int(row)] if int(row) < len(st.row_doc) else None
                    if doc is None:
                        continue
                    hit = dict(doc)
                    if config.RASS_RETURN_EMBEDDING:
                        hit["embedding"] = st.index.get_row(int(row)).tolist()  # reference quirk 5
                    out.append((hit, float(s)))
                return out
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    def semantic_search_scored(self, query_emb: np.ndarray, k: int = TOP_K, functions: Optional[List[Dict]] = None,
                               score_mode: str = "multiply", boost_mode: str = "multiply", max_boost: Optional[float] = None,
                               min_score: Optional[float] = None, boost: float = 1.0, where: Optional[Any] = None,
                               filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                               doc_type: Optional[str] = None, knn_score_mode: Optional[str] = None) -> List[Tuple[Dict, float]]:
        """An OpenSearch ``function_score`` around the k-NN clause, answered exactly over EVERY chunk of the index
        (``FlatIndex.search_scored``): the top ``k`` chunks by ``boost_mode(boost * knn_score, functions' value)``.
        ``functions``: ``function_score.functions`` entries (``gauss`` / ``exp`` / ``linear`` decay, ``field_value_factor``,
        ``weight``, each with an optional ``filter`` and ``weight``; ``attrfilter.compile_functions``), folded per chunk by
        ``score_mode`` (multiply / sum / avg / first / max / min) and capped at ``max_boost``; a chunk no function applies to
        is worth 1.0.  ``boost_mode``: multiply / sum / avg / max / min / replace.  ``min_score``: only chunks whose
        ``knn_score`` (before the boost) is at least this rank.  ``where``: a filter as ``semantic_search_filtered`` takes it.
        ``filter_clause`` / ``patient_id`` / ``doc_type`` as in ``semantic_search``.  ``knn_score`` is in
        ``knn_score_mode``'s units (default ``RASS_SCORE_MODE``).  A log modifier over a non-positive value excludes the chunk
        (OpenSearch raises).  Returns ``[(doc_dict, float(fused))]`` best first; ``[]`` on an empty embedding or on any
        exception (logged)."""
        if _empty(query_emb):
            return []
        try:
            return self._scored(query_emb, k, functions, score_mode, boost_mode, max_boost, min_score, boost, where, filter_clause,
                                patient_id, doc_type, knn_score_mode)
        except Exception as e:
            logger.error(f"Function-score search error: {e}")
            return []

    def semantic_search_recent(self, query_emb: np.ndarray, k: int = TOP_K, field: str = "conditionOnsetDateTime",
                               min_score: Optional[float] = None, order: str = "desc", missing: str = "exclude",
                               where: Optional[Any] = None, filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                               doc_type: Optional[str] = None, knn_score_mode: Optional[str] = None) -> List[Tuple[Dict, float]]:
        """The vector counterpart of the reference's ``temporal_search`` sort (app/main.py:1866-1918): the ``k`` chunks with
        ``knn_score >= min_score`` ordered by ``field`` (an int or date attribute field), ``order`` "desc" (latest first) or
        "asc"; ties by row.  ``missing`` "exclude" drops the chunks without the field, "_last" places them after every chunk
        that has it.  Exact over the whole index, however many chunks pass ``min_score``: ``boost_mode`` replace over a
        ``field_value_factor`` (negated for "asc").  Exact only while the field's values are exactly representable in fp32 and
        apart from the stand-in for "no value" (|v| < 2^24; days since 1970 are): checked with ``attr_minmax`` under the same
        lock as the search, else ``ValueError``.  Returns ``[(doc_dict,
        float(sort value))]`` — the field's value (days since 1970 for a date), NaN for a chunk without it; ``[]`` on an
        empty embedding or on any exception (logged)."""
        if _empty(query_emb):
            return []
        try:
            if order not in ("desc", "asc"):
                raise ValueError(f"order must be desc / asc, not {order!r}")
            if missing not in ("exclude", "_last"):
                raise ValueError(f"missing must be exclude / _last, not {missing!r}")
            st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
            if st is None:
                return []
            col = st.attrs.column(field) if st.attrs is not None else None
            if col is None or col[1] == "keyword":
                raise ValueError(f"{field!r} is not an int or date attribute field of {self.index_name}")
            sign = 1.0 if order == "desc" else -1.0
            fvf = {"field": field, "factor": sign}
            if missing == "_last":
                fvf["missing"] = -sign * RECENT_MAX_ABS     # below every stored value after the factor
            hits = self._scored(query_emb, k, [{"field_value_factor": fvf}], "first", "replace", None, min_score, 1.0, where,
                                filter_clause, patient_id, doc_type, knn_score_mode,
                                missing_excludes=missing == "exclude", exact_field=(field, col[0]))
            return [(d, float("nan") if s == -RECENT_MAX_ABS else sign * s) for d, s in hits]
        except Exception as e:
            logger.error(f"Recent search error: {e}")
            return []

    def _scored(self, query_emb, k, functions, score_mode, boost_mode, max_boost, min_score, boost, where, filter_clause, patient_id,
                doc_type, knn_score_mode, missing_excludes: bool = False, exact_field: Optional[Tuple[str, int]] = None
                ) -> List[Tuple[Dict, float]]:
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return []
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, doc_type)
        if prep is None:
            return []
        q, k_eff, (fval, fmask) = prep
        flt = dict(q_filter=np.array([fval], dtype=np.int32), q_filter_mask=np.array([fmask], dtype=np.int32)) if fmask else {}
        if not hasattr(st.index, "search_scored") or not hasattr(st.index, "fn_from_attr"):
            raise NotImplementedError(f"{self.index_name}: {type(st.index).__name__} has no function-score search "
                                      "(sharded indices cannot rank by a function column; use a flat fp32 index)")
        boost = float(boost)
        if not np.isfinite(boost):
            raise ValueError(f"boost must be finite, got {boost!r}")
        gate = None if min_score is None else float(min_score)
        if gate is not None and np.isnan(gate):
            raise ValueError("min_score must not be NaN")
        transform = "raw" if (knn_score_mode or config.RASS_SCORE_MODE) == "cosine" else "opensearch"
        from .attrfilter import compile_filter, compile_functions, run_plan
        for _ in range(LAYOUT_ATTEMPTS):    # the column and the ids belong to ONE layout of the index, as in _boosted
            layout = _layout_epoch(st.index)
            # under the state's lock from the first cell to the search: no row is appended in between (add_documents takes
            # the lock), so the column covers every row the scan sees
            with st.lock:
                if _layout_epoch(st.index) != layout:
                    continue
                if exact_field is not None and hasattr(st.index, "attr_minmax"):     # semantic_search_recent: see its docstring
                    lo, hi, _ = st.index.attr_minmax(exact_field[1])
                    if lo is not None and max(abs(int(lo)), abs(int(hi))) >= RECENT_MAX_ABS:
                        raise ValueError(f"{exact_field[0]!r} holds values of 2^24 or beyond in size: not exactly representable in "
                                         "fp32 (or equal to the stand-in for a missing value), the order would not be exact")
                records, plans = compile_functions(functions, st.attrs, st.patients, st.doc_types)
                bitmaps = [run_plan(st.index, plan) for plan in plans] or None
                column = st.index.new_bonus()
                st.index.fn_from_attr(column, records, score_mode=score_mode, max_boost=max_boost, filters=bitmaps)
                if missing_excludes:    # semantic_search_recent: the one function skipped the rows without the field (1.0 there)
                    exists = {"exists": {"field": functions[0]["field_value_factor"]["field"]}}
                    st.index.bonus_mask(column, run_plan(st.index, compile_filter(exists, st.attrs, st.patients, st.doc_types)))
                if where is not None:
                    st.index.bonus_mask(column, run_plan(st.index, compile_filter(where, st.attrs, st.patients, st.doc_types)))
                scores, ids = st.index.search_scored(q, k_eff, column, boost=boost, transform=transform, combine=boost_mode,
                                                     min_score=gate, **flt)
                out: List[Tuple[Dict, float]] = []
                for s, row in zip(scores[0], ids[0]):
                    if row < 0:
                        break
                    doc = st.row_doc[int(row)] if int(row) < len(st.row_doc) else None
                    if doc is None:
                        continue
                    hit = dict(doc)
                    if config.RASS_RETURN_EMBEDDING:
                        hit["embedding"] = st.index.get_row(int(row)).tolist()  # reference quirk 5
                    out.append((hit, float(s)))
                return out
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    @staticmethod
    def _text_rows(st: IndexState, text_hits) -> Tuple[List[int], List[float]]:
        """``[(doc | doc_id, score)]`` -> (rows, fp32 values) with one entry per row: ids the index does not hold (never
        indexed, deleted) are dropped, repeated ids summed in list order.  The caller holds ``st.lock``."""
        acc: Dict[int, np.float32] = {}
        for doc, s in text_hits or []:
            key = doc.get("doc_id") if isinstance(doc, dict) else doc
            row = st.doc_row.get(key) if key is not None else None
            if row is None or row >= len(st.row_doc) or st.row_doc[row] is None:
                continue
            acc[row] = np.float32(acc[row] + np.float32(s)) if row in acc else np.float32(s)
        return list(acc.keys()), [float(v) for v in acc.values()]

    def knn_scores(self, query_emb: np.ndarray, k: int = TOP_K, boost: float = 1.0,
                   filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None,
                   doc_type: Optional[str] = None) -> List[Tuple[Dict, float]]:
        """The knn ``should`` clause on its own: ``boost * _score`` per hit."""
        if _empty(query_emb):
            return []
        try:
            return self._knn(query_emb, k, filter_clause, patient_id, boost=boost, doc_type=doc_type)
        except Exception as e:
            logger.error(f"kNN score error: {e}")
            return []

    # ------------------------------------------------------------------ app/main.py:1562-1615
    def hybrid_search(self, query: str, query_emb: np.ndarray, k: int = TOP_K, filter_clause: Optional[Dict] = None,
                      patient_id: Optional[str] = None) -> List[Tuple[Dict, float]]:
        if not query or not query.strip() or _empty(query_emb):
            return []  # 1570-1571
        return self._hybrid("hybrid_search", "Hybrid search error", query, query_emb, k, filter_clause, patient_id,
                            BOOST_HYBRID, None)

    # ------------------------------------------------------------------ app/main.py:1710-1775
    def hybrid_structured_search(self, query: str, query_emb: np.ndarray, k: int = TOP_K,
                                 filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None
                                 ) -> List[Tuple[Dict, float]]:
        if not query or not query.strip() or _empty(query_emb):
            return []  # 1712-1713
        # term: doc_type = structured (1765).  The reference stores no embedding on structured docs
        # (1222-1240), so its knn clause matches none of them; here the filter selects the rows whose
        # doc_type byte says "structured" — none with the reference's ingest, all of them for a
        # deployment that embeds its structured docs.
        return self._hybrid("hybrid_structured_search", "Hybrid structured search error", query, query_emb, k,
                            filter_clause, patient_id, BOOST_HYBRID_STRUCTURED, "structured")

    # ------------------------------------------------------------------ app/main.py:1962-2027
    def multi_intent_search(self, query: str, query_emb: np.ndarray, k: int = TOP_K,
                            filter_clause: Optional[Dict] = None, patient_id: Optional[str] = None
                            ) -> List[Tuple[Dict, float]]:
        if not query or not query.strip() or _empty(query_emb):
            return []  # 1970-1971
        return self._hybrid("multi_intent_search", "Multi-intent search error", query, query_emb, k, filter_clause,
                            patient_id, BOOST_MULTI_INTENT, None)

    async def asemantic_search(self, query_emb: np.ndarray, k: int = TOP_K, filter_clause: Optional[Dict] = None,
                               patient_id: Optional[str] = None, query: Optional[str] = None, **_ignored
                               ) -> List[Tuple[Dict, float]]:
        """Awaitable ``semantic_search``: concurrent callers on one event loop share scans
        through the index's ``QueryBatcher`` (up to 32 queries per HBM pass) instead of
        blocking the loop with one scan each (the reference calls the sync client inline,
        app/main.py:1552)."""
        if _empty(query_emb):
            return []
        try:
            st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
            if st is None:
                return []
            prep = self._prepare(st, query_emb, k, filter_clause, patient_id, None)
            if prep is None:
                return []
            q, k_eff, (fval, fmask) = prep
            eng = getattr(st.index, "engine", None)
            for _ in range(LAYOUT_ATTEMPTS):    # the batchers hand back row ids: paired with the layout epoch as in _knn
                layout = _layout_epoch(st.index)
                if eng is not None and hasattr(eng, "search_multi") and k_eff <= 32:
                    # one batcher per ENGINE: concurrent users' per-user indices share scan launches
                    if getattr(eng, "_cross_batcher", None) is None:
                        from .batcher import CrossIndexBatcher
                        eng._cross_batcher = CrossIndexBatcher(eng)
                    scores, ids = await eng._cross_batcher.search(st.index, q[0], k_eff, fval, fmask)
                else:
                    if st.batcher is None:
                        from .batcher import QueryBatcher
                        st.batcher = QueryBatcher(st.index)
                    scores, ids = await st.batcher.search(q[0], k_eff, fval, fmask)
                hits = self._hits(st, scores, ids, 1.0, None, layout)
                if hits is not None:
                    return hits
            raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")
        except Exception as e:
            logger.error(f"Semantic search error: {e}")
            return []

    # ---------------------------------------------------------------------------- internals
    @staticmethod
    def _prepare(st: IndexState, query_emb, k, filter_clause, patient_id, doc_type):
        q = np.asarray(query_emb, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        q = np.ascontiguousarray(q[:1])  # the reference searches row 0 only: (…)[0].tolist(), 1537
        # the reference ANDs its filter list (filter_clause, then term: patientId, then — hybrid_structured_search — term:
        # doc_type, 1543-1550 / 1760-1765): two different values for one field match nothing
        f_pid, f_dtype = _term_from_filter(filter_clause, "patientId"), _term_from_filter(filter_clause, "doc_type")
        if (patient_id and f_pid is not None and str(f_pid) != str(patient_id)) or \
                (doc_type and f_dtype is not None and str(f_dtype) != str(doc_type)):
            return None
        pid = patient_id if patient_id else f_pid
        dtype = doc_type if doc_type else f_dtype
        flt = st.filter_for(pid, dtype)
        if flt is None:
            return None  # term filter on a value that was never indexed
        return q, max(1, int(k)), flt

    def _knn(self, query_emb, k, filter_clause, patient_id, boost, doc_type=None, score_mode=None
             ) -> List[Tuple[Dict, float]]:
        st: Optional[IndexState] = REGISTRY.get(self.index_name, create=False)
        if st is None:
            return []
        prep = self._prepare(st, query_emb, k, filter_clause, patient_id, doc_type)
        if prep is None:
            return []
        q, k_eff, (fval, fmask) = prep
        # Row ids are ordinals of ONE layout of the index (a compaction renumbers them, docstore.IndexState.compact): the
        # layout epoch is read before the search and compared under st.lock before the ids are mapped through row_doc;
        # when a compaction landed in between, the search runs again (a compaction is rare and far slower than a search).
        for _ in range(LAYOUT_ATTEMPTS):
            layout = _layout_epoch(st.index)
            parked = prefetch.take(st, q, k_eff, fval, fmask)
            if parked is not None:      # this request's scan was shared with the other requests in flight
                scores, ids = parked
            elif fmask:
                scores, ids = st.index.search(q, k_eff, q_filter=np.array([fval], dtype=np.int32),
                                              q_filter_mask=np.array([fmask], dtype=np.int32))
                scores, ids = scores[0], ids[0]
            else:
                scores, ids = st.index.search(q, k_eff)
                scores, ids = scores[0], ids[0]
            hits = self._hits(st, scores, ids, boost, score_mode, layout)
            if hits is not None:
                return hits
        raise RuntimeError(f"{self.index_name}: the index was compacted during every one of {LAYOUT_ATTEMPTS} searches")

    @staticmethod
    def _hits(st: IndexState, scores, ids, boost, score_mode, layout: Optional[int] = None
              ) -> Optional[List[Tuple[Dict, float]]]:
        """ids -> docs under the state's lock.  ``layout``: the index's layout epoch read BEFORE the search; None is
        returned (search again) when the index has been compacted since — the ids would name other rows now."""
        out: List[Tuple[Dict, float]] = []
        with st.lock:
            if layout is not None and _layout_epoch(st.index) != layout:
                return None
            for cos, row in zip(scores, ids):
                if row < 0:
                    break
                doc = st.row_doc[int(row)] if int(row) < len(st.row_doc) else None
                if doc is None:
                    continue
                hit = dict(doc)
                if config.RASS_RETURN_EMBEDDING:
                    hit["embedding"] = st.index.get_row(int(row)).tolist()  # reference quirk 5
                out.append((hit, boost * _score_out(cos, score_mode)))
        return out

    def _hybrid(self, method: str, err_label: str, query, query_emb, k, filter_clause, patient_id, boost, doc_type
                ) -> List[Tuple[Dict, float]]:
        """``bool.should`` of the reference's hybrid builders: score = sum of the matching clauses.
        The knn clause comes from the HBM index; the text clauses from the kept text engine (when there
        is one), whose own knn clause matches nothing because no vector is stored there any more.  The
        two ranked lists are read FUSION_OVERFETCH x k deep and summed by ``doc_id``."""
        try:
            k = max(1, int(k))
            text = self._text_engine()
            depth = k * FUSION_OVERFETCH if text is not None else k
            if config.RASS_HYBRID_EXACT and text is not None:
                # the text list at today's depth becomes a bonus column: every row gets boost * knn score + its text score
                try:
                    bm25 = getattr(text, method)(query, query_emb, k=depth, filter_clause=filter_clause, patient_id=patient_id)
                except Exception as e:
                    logger.error(f"{err_label} (text clauses): {e}")
                    bm25 = []
                return self._boosted(query_emb, k, boost, bm25, None, None, filter_clause, patient_id, doc_type, None)
            knn = self._knn(query_emb, depth, filter_clause, patient_id, boost=boost, doc_type=doc_type)
            if text is None:
                return knn[:k]
            try:
                bm25 = getattr(text, method)(query, query_emb, k=depth, filter_clause=filter_clause,
                                             patient_id=patient_id)
            except Exception as e:  # e.g. the reference's own KeyError in hybrid_structured_search (quirk 3)
                logger.error(f"{err_label} (text clauses): {e}")
                bm25 = []
            fused: Dict[Any, List] = {}
            for doc, s in knn:
                fused[doc.get("doc_id", id(doc))] = [doc, float(s)]
            for doc, s in bm25 or []:
                key = doc.get("doc_id", id(doc))
                if key in fused:
                    fused[key][1] += float(s)
                else:
                    fused[key] = [doc, float(s)]
            ranked = sorted(fused.values(), key=lambda e: -e[1])
            return [(d, s) for d, s in ranked[:k]]
        except Exception as e:
            logger.error(f"{err_label}: {e}")
            return []


# --------------------------------------------------------------------------------- write side
_ORIGINALS: Dict[int, Dict[str, Any]] = {}   # id(module) -> the names install() replaced


def _originals_for(fn_globals_name: Optional[str] = None) -> Dict[str, Any]:
    for rec in _ORIGINALS.values():
        if fn_globals_name is None or rec.get("__name__") == fn_globals_name:
            return rec
    return {}


async def ensure_index_exists(client: Any, index_name: str) -> None:
    """app/main.py:350-579: create the per-user cosine index when absent; errors are printed
    and swallowed (578-579).  When a text engine is kept (``client`` given and the module's original
    function was recorded by ``install``) its index — the ~90 text fields — is ensured as well."""
    st = None
    try:
        st = REGISTRY.get(index_name, create=True)
    except Exception as e:
        print(f"[Error] OpenSearch Index could not be created: {e}")
    orig = _originals_for().get("ensure_index_exists")
    if client and orig is not None:
        try:
            await orig(client, index_name)
        except Exception as e:
            print(f"[Error] OpenSearch Index could not be created: {e}")
    # ask() awaits this right after embed_query and right before its synchronous search (app/main.py:2800-2802):
    # the one place where the k-NN scans of concurrent requests can share a launch (prefetch.py)
    await prefetch.run(st)


def add_documents(index_name: str, docs: List[Dict], embeddings: Optional[np.ndarray],
                  texts: Optional[List[str]] = None) -> List[int]:
    """Append ``docs`` with their (un-normalised) ``embeddings`` [n, dim]; the GPU normalises
    (app/main.py:1249-1251).  ``_id = doc_id`` overwrite semantics (1260): the new rows are appended
    FIRST and the rows they supersede are tombstoned only after the append succeeded, so a failed add
    (OOM on slab growth, HIP error) loses nothing.  Returns the row ids.  With ``texts`` instead of
    ``embeddings`` (a multi-GPU index whose ranks have encoders, ``index.can_encode``) the texts are embedded
    where their rows will live: data-parallel over the ranks, no vector leaves its GPU."""
    st = REGISTRY.get(index_name, create=True)
    if texts is not None:
        if len(texts) != len(docs):
            raise ValueError(f"{len(texts)} texts do not match {len(docs)} docs")
        emb = None
    else:
        emb = np.ascontiguousarray(embeddings, dtype=np.float32)
        if emb.ndim != 2 or emb.shape[0] != len(docs):
            raise ValueError(f"embeddings {emb.shape} do not match {len(docs)} docs")
    with st.lock:
        tags = np.array([st.tag_of(d) for d in docs], dtype=np.int32)
        # the attribute columns of the new rows; encoded before the append, so a value that does not fit changes nothing
        cols = st.attrs.encode_docs(docs) if st.attrs and hasattr(st.index, "set_attr") else None
        # duplicates inside one batch: the last one wins, as with sequential bulk index ops
        last = {}
        for i, d in enumerate(docs):
            last[d.get("doc_id")] = i
        if emb is None:
            first = st.index.add_texts(list(texts), tags=tags, normalize=True)
        else:
            first = st.index.add(emb, tags=tags, normalize=True)      # raises -> nothing was changed
        rows = list(range(first, first + len(docs)))
        if cols is not None and len(docs):      # right after the append, before the rows they supersede are tombstoned
            for c in range(cols.shape[0]):
                st.index.set_attr(c, first, cols[c])
        for d in docs:
            old = st.doc_row.pop(d.get("doc_id"), None)
            if old is not None:
                st.index.delete(old)
                st.row_doc[old] = None
                st.note_deleted(old)
        for i, (d, r) in enumerate(zip(docs, rows)):
            if len(st.row_doc) <= r:
                st.row_doc.extend([None] * (r + 1 - len(st.row_doc)))
            if last[d.get("doc_id")] == i:
                st.row_doc[r] = d
                st.doc_row[d.get("doc_id")] = r
            else:
                st.index.delete(r)  # superseded inside the same batch
        _maybe_compact(st)
        return rows


def _maybe_compact(st: IndexState) -> None:
    """The compaction policy (``RASS_COMPACT_FRACTION`` / ``RASS_COMPACT_MIN_ROWS``, off by default): once the tombstones
    of an index exceed the fraction of its rows, they are squeezed out on the GPU.  An index that cannot compact (a
    sharded front) is skipped.  The caller holds ``st.lock``.  (The row ids ``add_documents`` returns are those of the
    append, as before: after a compaction they have been renumbered like every other row.)"""
    fraction = config.RASS_COMPACT_FRACTION
    if fraction <= 0 or not callable(getattr(st.index, "compact", None)):
        return
    rows = int(st.index.rows)
    dead = rows - int(st.index.count)
    if rows < config.RASS_COMPACT_MIN_ROWS or dead <= fraction * rows:
        return
    try:
        st.compact()
    except NotImplementedError:     # an index whose compaction is out of scope (serving.ShardedIndex)
        pass


async def _call_embed(embed_fn, texts: List[str]) -> np.ndarray:
    """main.py's embed_texts_in_batches takes batch_size (240-242), embedding_gen.py's does not (173)."""
    try:
        params = inspect.signature(embed_fn).parameters
    except (TypeError, ValueError):
        params = {}
    if "batch_size" in params:
        return await embed_fn(texts, batch_size=config.BATCH_SIZE)
    return await embed_fn(texts)


async def store_fhir_docs_in_opensearch(structured_docs: List[Dict], unstructured_docs: List[Dict], client: Any,
                                        index_name: str, embed_fn=None) -> None:
    """app/main.py:1211-1282 (embedding_gen.py:1061-1132) with the vector hops removed: the
    unstructured docs are embedded (``embed_texts_in_batches``), normalised and indexed in HBM.
    Structured docs carry no embedding (k-NN never returns them — same as the reference); they are
    kept by doc_id and, when a text engine is kept (``client`` given, ``install`` recorded the module's
    ``bulk``), bulk-indexed there like the reference does — as are the unstructured docs' TEXT (without
    the 1024-float ``embedding`` field), so the BM25 builders keep seeing every document."""
    await ensure_index_exists(client, index_name)
    st = REGISTRY.get(index_name, create=True)
    bulk = _originals_for().get("bulk") if client else None

    def _bulk(docs: List[Dict], label: str) -> None:
        if bulk is None or not docs:
            return
        actions = [{"_op_type": "index", "_index": index_name, "_id": d["doc_id"], "_source": d,
                    "_routing": d.get("patientId")} for d in docs]
        step = max(1, config.BATCH_SIZE)
        for a in range(0, len(actions), step):
            try:
                ok, errors = bulk(client, actions[a:a + step])
                logger.info(f"Indexed {ok} {label} docs, errors: {errors}")
            except Exception as e:
                logger.error(f"{label.capitalize()} docs indexing error: {e}")

    if structured_docs:
        try:
            with st.lock:
                for doc in structured_docs:
                    st.structured[doc["doc_id"]] = doc
                    st.note_structured(doc["doc_id"])
            if bulk is None:
                logger.info(f"Indexed {len(structured_docs)} structured docs, errors: []")
        except Exception as e:
            logger.error(f"Structured docs indexing error: {e}")
        _bulk(structured_docs, "structured")
    if not unstructured_docs:
        return
    un_texts = [d["unstructuredText"] for d in unstructured_docs]
    # a multi-GPU index whose ranks hold encoders embeds the texts where their rows will live
    data_parallel = embed_fn is None and getattr(st.index, "can_encode", False)
    if embed_fn is None:
        from .embedding import embed_texts_in_batches as embed_fn
    if not data_parallel:
        embeddings = await _call_embed(embed_fn, un_texts)     # an embedding error propagates, as in the reference
    try:
        if data_parallel:
            await asyncio.to_thread(add_documents, index_name, unstructured_docs, None, un_texts)
        else:
            add_documents(index_name, unstructured_docs, embeddings)
        if bulk is None:
            logger.info(f"Indexed {len(unstructured_docs)} unstructured docs, errors: []")
    except Exception as e:
        logger.error(f"Unstructured docs indexing error: {e}")
        return
    _bulk(unstructured_docs, "unstructured")   # text only: the vectors live in HBM


# --------------------------------------------------------------------------------- install
def make_indexer_class(original_cls: Optional[type]) -> type:
    """A ``HipIndexer`` subclass that delegates the BM25 builders to ``original_cls``."""
    if original_cls is not None and isinstance(original_cls, type) and issubclass(original_cls, HipIndexer):
        return original_cls  # already installed
    if original_cls is None or original_cls is object or not callable(original_cls):
        return HipIndexer
    return type("HipIndexer", (HipIndexer,), {"_original_cls": original_cls, "__doc__": HipIndexer.__doc__})


def install(module) -> None:
    """Rebind the reference's hot-path names on an imported ``main`` / ``embedding_gen`` module
    (SURVEY §8b): routes, chunk_text, Prisma and LLM code stay untouched.

    * ``OpenSearchIndexer`` -> a ``HipIndexer`` subclass that KEEPS the module's own class for the eight
      BM25 / aggregate builders (``ask()`` builds a table of all eleven search methods before it
      dispatches, app/main.py:2855-2867, and calls ``document_fetch_search`` at 2805);
    * ``embed_*``: the flavour of the module being patched — ``app/main.py:225-274`` raises on errors and
      returns ``np.array([])`` for an empty list; ``app/embedding_gen.py:152-192`` takes no ``batch_size``,
      returns ``zeros((0, EMBED_DIM))`` and turns errors into zero vectors;
    * ``ensure_index_exists`` / ``store_fhir_docs_in_opensearch``: vectors to HBM; the module's originals and
      its ``bulk`` are remembered so a kept text engine still receives the text.
    Idempotent."""
    from . import embedding
    rec = _ORIGINALS.get(id(module))
    if rec is None:
        rec = {"__name__": getattr(module, "__name__", None)}
        for name in ("OpenSearchIndexer", "ensure_index_exists", "store_fhir_docs_in_opensearch", "bulk",
                     "ollama_embed_text", "embed_texts_in_batches", "embed_query"):
            if hasattr(module, name):
                rec[name] = getattr(module, name)
        _ORIGINALS[id(module)] = rec
    orig_embed = rec.get("embed_texts_in_batches")
    gen_flavour = False
    if callable(orig_embed):
        try:
            gen_flavour = "batch_size" not in inspect.signature(orig_embed).parameters
        except (TypeError, ValueError):
            gen_flavour = False
    elif str(rec.get("__name__") or "").endswith("embedding_gen"):
        gen_flavour = True
    emb = embedding.GEN_FLAVOUR if gen_flavour else embedding.MAIN_FLAVOUR
    bindings = (("OpenSearchIndexer", make_indexer_class(rec.get("OpenSearchIndexer"))),
                ("ensure_index_exists", ensure_index_exists),
                ("store_fhir_docs_in_opensearch", store_fhir_docs_in_opensearch),
                ("ollama_embed_text", emb["ollama_embed_text"]),
                ("embed_texts_in_batches", emb["embed_texts_in_batches"]),
                ("embed_query", emb["embed_query"]))
    for name, obj in bindings:
        if hasattr(module, name):
            setattr(module, name, obj)


def uninstall(module) -> None:
    """Put the module's own names back (tests)."""
    rec = _ORIGINALS.pop(id(module), None)
    if rec:
        for name, obj in rec.items():
            if name != "__name__" and name != "bulk":
                setattr(module, name, obj)
