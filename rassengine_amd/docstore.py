"""Host-side metadata that OpenSearch kept next to the vectors: ``row -> doc dict``,
``doc_id -> row`` (overwrite semantics of ``_id=doc_id``, app/main.py:1260), the patientId
dictionary behind the integer row tags (the reference's ``_routing`` / ``term: patientId``
filter, app/main.py:1263, 1549) and the ``doc_type`` dictionary (``term: doc_type`` of
hybrid_structured_search, app/main.py:1765).  Pure Python; the vectors live in HBM.

Row tag (int32, on the device): ``patient code | doc_type code << 24`` — bits 0..23 the patientId
code (0 = none), bits 24..30 the doc_type code (0 = none); -1 = tombstone.  A masked compare in
the scan kernel serves either filter or both (include/rass_engine.h, RASS_TAG_*).

One ``IndexState`` per index name; a process-global registry makes
``HipIndexer(client, index_name)`` O(1) (the reference builds it per request, 2802).
"""
from __future__ import annotations

import datetime as _dt
import json
import logging
import os
import re
import threading
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

logger = logging.getLogger("rassengine_amd")

PATIENT_NONE = 0  # tag of rows without a patientId
TAG_PATIENT_MASK = 0x00FFFFFF
TAG_DOCTYPE_SHIFT = 24
TAG_DOCTYPE_MASK = 0x7F000000


class PatientDictionary:
    """Dictionary-encodes strings to int32 codes >= 1 (0 = none).  Used for patientId
    (24 bits) and doc_type (7 bits)."""

    def __init__(self, max_code: int = TAG_PATIENT_MASK):
        self._code: Dict[str, int] = {}
        self._name: List[Optional[str]] = [None]
        self._max = max_code

    def encode(self, patient_id: Optional[Any]) -> int:
        if patient_id is None or patient_id == "":
            return PATIENT_NONE
        key = str(patient_id)
        code = self._code.get(key)
        if code is None:
            code = len(self._name)
            if code > self._max:
                raise OverflowError(f"dictionary full ({self._max} distinct values)")
            self._code[key] = code
            self._name.append(key)
        return code

    def lookup(self, patient_id: Optional[Any]) -> Optional[int]:
        """Code of a known value, None when it was never indexed (filter matches nothing)."""
        if patient_id is None or patient_id == "":
            return None
        return self._code.get(str(patient_id))

    def names(self) -> List[str]:
        return list(self._name[1:])

    def __len__(self) -> int:
        return len(self._name) - 1


ATTR_MISSING = -(1 << 31)     # RASS_ATTR_MISSING: the row has no value in the column
ATTR_MIN, ATTR_MAX = ATTR_MISSING + 1, (1 << 31) - 1
MAX_ATTRS = 8                 # RASS_MAX_ATTRS
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)
_DATE_ONLY = re.compile(r"^\d{4}-\d{2}-\d{2}$")
_DATE_MATH = re.compile(r"^now(?:([+-])(\d+)([dwMy]))?$")


def utc_now() -> _dt.datetime:
    """The clock behind ``now`` in a date range (``AttrSchema.clock`` defaults to it; tests inject their own)."""
    return _dt.datetime.now(_dt.timezone.utc)


def date_days(value: Any) -> Optional[int]:
    """A date as days since 1970-01-01 UTC: ``YYYY-MM-DD``, an ISO-8601 date-time with or without an offset (none = UTC;
    floored to its UTC day) or integer epoch milliseconds.  None when the value is none of these."""
    if isinstance(value, bool) or value is None:
        return None
    if isinstance(value, (int, np.integer)):
        days = int(value) // 86_400_000
        return days if ATTR_MIN <= days <= ATTR_MAX else None
    if not isinstance(value, str):
        return None
    text = value.strip()
    try:
        if _DATE_ONLY.match(text):
            return _dt.date.fromisoformat(text).toordinal() - _EPOCH.toordinal()
        if text[-1:] in ("Z", "z"):
            text = text[:-1] + "+00:00"
        when = _dt.datetime.fromisoformat(text)
    except ValueError:
        return None
    if when.tzinfo is None:
        when = when.replace(tzinfo=_dt.timezone.utc)
    return (when - _EPOCH) // _dt.timedelta(days=1)


def date_bound_days(value: Any, now: _dt.datetime) -> Optional[int]:
    """A bound of a ``range`` on a date field: what ``date_days`` takes, plus ``now`` and ``now±N(d|w|M|y)`` against the
    given clock (months and years on the calendar, the day clamped to the month's length)."""
    if isinstance(value, str):
        m = _DATE_MATH.match(value.strip())
        if m:
            when = now.astimezone(_dt.timezone.utc)
            if m.group(1):
                n = int(m.group(2)) * (1 if m.group(1) == "+" else -1)
                unit = m.group(3)
                if unit in "dw":
                    when = when + _dt.timedelta(days=n * (7 if unit == "w" else 1))
                else:
                    months = when.year * 12 + (when.month - 1) + n * (12 if unit == "y" else 1)
                    year, month = divmod(months, 12)
                    nxt = _dt.date(year + (month == 11), (month + 1) % 12 + 1, 1)
                    last = (nxt - _dt.timedelta(days=1)).day
                    when = when.replace(year=year, month=month + 1, day=min(when.day, last))
            return (when - _EPOCH) // _dt.timedelta(days=1)
    return date_days(value)


class AttrSchema:
    """The typed per-row fields an index keeps as int32 attribute columns: an ordered list of up to 8 ``(field, kind)``
    pairs, column c = pair c.  ``keyword``: the value's dictionary code (>= 1; the dictionary grows as values arrive, like
    ``PatientDictionary``); ``int``: the value itself, which must fit int32; ``date``: days since 1970-01-01 UTC
    (``date_days``).  An absent, None or (keyword) empty value, and a date that cannot be parsed (logged once per field), is
    missing.  An empty schema is falsy: no column is ever set."""

    KINDS = ("keyword", "int", "date")

    def __init__(self, fields=()):
        self.fields: List[Tuple[str, str]] = [(str(f), str(k)) for f, k in fields]
        if len(self.fields) > MAX_ATTRS:
            raise ValueError(f"at most {MAX_ATTRS} attribute fields, got {len(self.fields)}")
        names = [f for f, _ in self.fields]
        if len(set(names)) != len(names) or any(not f for f in names):
            raise ValueError(f"attribute field names must be distinct and non-empty: {names}")
        for f, k in self.fields:
            if k not in self.KINDS:
                raise ValueError(f"attribute field {f!r}: kind must be one of {self.KINDS}, not {k!r}")
            if f in ("patientId", "doc_type"):
                raise ValueError(f"{f!r} lives in the row tag, not in an attribute column")
        self.dicts: Dict[str, PatientDictionary] = {f: PatientDictionary(max_code=ATTR_MAX) for f, k in self.fields if k == "keyword"}
        self.clock: Callable[[], _dt.datetime] = utc_now
        self._warned: set = set()

    @classmethod
    def parse(cls, spec: Optional[str]) -> "AttrSchema":
        """``"resourceType:keyword,file_type:keyword,chunkDate:date"`` (``config.RASS_ATTR_FIELDS``); empty = no schema."""
        pairs = []
        for item in (spec or "").split(","):
            if item.strip():
                field, sep, kind = item.strip().partition(":")
                if not sep:
                    raise ValueError(f"attribute field {item!r}: expected field:kind")
                pairs.append((field.strip(), kind.strip().lower()))
        return cls(pairs)

    def __bool__(self) -> bool:
        return bool(self.fields)

    def __len__(self) -> int:
        return len(self.fields)

    def __eq__(self, other) -> bool:
        return isinstance(other, AttrSchema) and self.fields == other.fields

    def column(self, field: str) -> Optional[Tuple[int, str]]:
        """(column, kind) of a schema field, None for a field the schema does not hold."""
        for c, (f, k) in enumerate(self.fields):
            if f == field:
                return c, k
        return None

    def encode_value(self, col: int, value: Any) -> int:
        """The int32 stored for ``value`` in column ``col`` (a new keyword value gets a code)."""
        field, kind = self.fields[col]
        if value is None:
            return ATTR_MISSING
        if kind == "keyword":
            code = self.dicts[field].encode(value)
            return code if code != PATIENT_NONE else ATTR_MISSING
        if kind == "int":
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError(f"attribute field {field!r} is an int column, got {value!r}")
            if not ATTR_MIN <= int(value) <= ATTR_MAX:
                raise OverflowError(f"attribute field {field!r}: {value} does not fit an int32 column")
            return int(value)
        days = date_days(value)
        if days is None or not ATTR_MIN <= days <= ATTR_MAX:
            if field not in self._warned:
                self._warned.add(field)
                logger.warning(f"attribute field {field!r}: {value!r} is not a date (YYYY-MM-DD, ISO-8601 or epoch "
                               "milliseconds); stored as missing (logged once per field)")
            return ATTR_MISSING
        return days

    def encode_docs(self, docs: List[dict]) -> np.ndarray:
        """int32 [len(fields), len(docs)]: row c is column c of the docs."""
        out = np.full((len(self.fields), len(docs)), ATTR_MISSING, dtype=np.int32)
        for c, (field, _) in enumerate(self.fields):
            for i, d in enumerate(docs):
                if d is not None:
                    out[c, i] = self.encode_value(c, d.get(field))
        return out

    def to_meta(self) -> dict:
        return {"fields": [[f, k] for f, k in self.fields], "keywords": {f: d.names() for f, d in self.dicts.items()}}

    @classmethod
    def from_meta(cls, meta: Optional[dict]) -> "AttrSchema":
        if not meta:
            return cls()
        schema = cls([(f, k) for f, k in meta.get("fields", [])])
        schema.absorb(meta)
        return schema

    def absorb(self, meta: Optional[dict]) -> None:
        """The keyword dictionaries of a manifest or a delta segment, in their stored order (codes are positions)."""
        for field, names in ((meta or {}).get("keywords") or {}).items():
            if field in self.dicts:
                for name in names:
                    self.dicts[field].encode(name)


def compose_tag(patient_code: int, doctype_code: int) -> int:
    return (int(patient_code) & TAG_PATIENT_MASK) | (int(doctype_code) << TAG_DOCTYPE_SHIFT)


class IndexState:
    """Everything the shim keeps per index name besides the HBM slab."""

    def __init__(self, name: str, index):
        self.name = name
        self.index = index                      # FlatIndex-like: add / delete / search / count
        self.lock = threading.RLock()
        self.row_doc: List[Optional[dict]] = []  # row id -> stored doc (None = tombstoned)
        self.doc_row: Dict[str, int] = {}        # doc_id -> live row
        self.structured: Dict[str, dict] = {}    # structured docs carry no embedding (app/main.py:1222-1240)
        self.patients = PatientDictionary()
        self.doc_types = PatientDictionary(max_code=0x7F)
        from . import config
        self.attrs = AttrSchema.parse(config.RASS_ATTR_FIELDS)   # empty (falsy) = no attribute columns
        self.batcher = None                      # QueryBatcher, created on first async search
        self.generation = 0                      # bumped by every save()
        # incremental persistence (save_delta): what changed since the last save() / save_delta()
        self._ckpt_rows = 0                      # rows of the index that are on disk
        self._dead_since: List[int] = []         # rows < _ckpt_rows tombstoned since
        self._structured_dirty: set = set()      # structured doc_ids (re)written since
        self._delta_seq = 0                      # delta segments written on top of the current snapshot
        self._delta_broken = False               # a compaction renumbered the rows: the log is unusable until the next save()

    def live_count(self) -> int:
        return len(self.doc_row) + len(self.structured)

    # ---- the write path reports what it changes (indexer.add_documents / store_fhir_docs_in_opensearch)
    def note_deleted(self, row: int) -> None:
        if row < self._ckpt_rows:
            self._dead_since.append(int(row))

    def note_structured(self, doc_id: str) -> None:
        self._structured_dirty.add(doc_id)

    # ---- compaction: tombstoned rows leave the index (FlatIndex.compact) and every ordinal kept here follows
    def compact(self) -> Tuple[int, int]:
        """Remove the tombstoned rows from the index and renumber ``row_doc`` / ``doc_row`` through the old -> new map it
        returns, all under the state's lock: a reader that maps ids under the lock sees the old layout or the new one
        (``indexer.HipIndexer._hits`` compares the index's ``layout_epoch``).  The delta log speaks old ordinals:
        ``save_delta`` answers False ("take a snapshot") until the next ``save``.  Returns (rows before, rows after)."""
        with self.lock:
            new_row = np.asarray(self.index.compact(), dtype=np.int64)
            before, after = int(new_row.shape[0]), int(self.index.rows)
            if after == before:             # no tombstone: nothing moved
                return before, after
            row_doc: List[Optional[dict]] = [None] * after
            for old, new in enumerate(new_row.tolist()):
                if new >= 0 and old < len(self.row_doc):
                    row_doc[new] = self.row_doc[old]
            self.row_doc = row_doc
            self.doc_row = {doc_id: int(new_row[old]) for doc_id, old in self.doc_row.items() if new_row[old] >= 0}
            self._delta_broken = True
            self._dead_since = []
            return before, after

    def tag_of(self, doc: dict) -> int:
        return compose_tag(self.patients.encode(doc.get("patientId")), self.doc_types.encode(doc.get("doc_type")))

    def filter_for(self, patient_id: Optional[Any], doc_type: Optional[str]) -> Optional[Tuple[int, int]]:
        """(value, mask) of the masked tag compare for the given term filters; (-1, 0) = no filter;
        None = a filter on a value that was never indexed (matches nothing)."""
        value = mask = 0
        if patient_id not in (None, ""):
            code = self.patients.lookup(patient_id)
            if code is None:
                return None
            value |= code
            mask |= TAG_PATIENT_MASK
        if doc_type not in (None, ""):
            code = self.doc_types.lookup(doc_type)
            if code is None:
                return None
            value |= code << TAG_DOCTYPE_SHIFT
            mask |= TAG_DOCTYPE_MASK
        return (value, mask) if mask else (-1, 0)

    # ---- persistence: the vectors go to `<prefix>.g<generation>.rass` (rass_index_save),
    # the host-side metadata OpenSearch used to hold (docs, doc_id map, dictionaries) to `<prefix>.meta.json`,
    # which NAMES the vector file of its generation.  Replaces OpenSearch's durability for this path.
    #
    # Crash safety: both files are written under temporary names and fsynced; the vector file is renamed to
    # its (new, unique) generation name first, the manifest is renamed LAST (os.replace is atomic), and only
    # then is the previous generation's vector file removed.  At every instant `<prefix>.meta.json` is either
    # the old manifest (whose vector file still exists) or the new one (whose vector file is complete).
    def save(self, prefix: str) -> None:
        with self.lock:
            # never reuse a file name the live manifest references: a state built WITHOUT load() starts at generation 0
            # and would otherwise overwrite `<prefix>.g000001.rass` in place before the new manifest is committed
            gen = max(self.generation, self._manifest_generation(prefix)) + 1
            prev = self._manifest_vectors(prefix)
            vec_name = f"{os.path.basename(prefix)}.g{gen:06d}.rass"
            vec_path = os.path.join(os.path.dirname(prefix) or ".", vec_name)
            tmp_vec = vec_path + ".tmp"
            self.index.save(tmp_vec)            # rass_index_save fsyncs before closing
            os.replace(tmp_vec, vec_path)
            meta = {"version": 2, "name": self.name, "generation": gen, "vectors": vec_name,
                    "rows": int(self.index.rows), "live": int(self.index.count),
                    "row_doc": self.row_doc, "structured": self.structured,
                    "patients": self.patients.names(), "doc_types": self.doc_types.names()}
            if self.attrs:          # the schema and its keyword dictionaries; the values are columns of the vector file
                meta["attrs"] = self.attrs.to_meta()
            tmp_meta = prefix + ".meta.json.tmp"
            with open(tmp_meta, "w", encoding="utf-8") as f:
                json.dump(meta, f)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp_meta, prefix + ".meta.json")
            _fsync_dir(os.path.dirname(prefix) or ".")
            self.generation = gen
            # the snapshot covers everything: the delta log of the previous generation goes with it
            self._ckpt_rows, self._dead_since, self._structured_dirty, self._delta_seq = int(self.index.rows), [], set(), 0
            self._delta_broken = False
            self._remove_deltas(prefix, keep_generation=None)
            if prev and prev != vec_path and os.path.exists(prev):
                # a sharded index's vector "file" is a manifest naming one shard file per rank
                for f in (self.index.saved_files(prev) if hasattr(self.index, "saved_files") else []):
                    if os.path.exists(f):
                        os.remove(f)
                os.remove(prev)

    # ---- incremental persistence (the reference's durability is incremental: one bulk per 64 docs,
    # app/main.py:1253-1282).  save() writes a SNAPSHOT (every vector, every doc: O(corpus)); save_delta() appends ONE segment
    # holding only what changed since the last save() / save_delta(): the rows appended since (read back from the index:
    # the stored, normalised bits), their docs, the rows tombstoned since, the structured docs rewritten since — O(delta).
    # `<prefix>.deltas.json` (tiny, replaced atomically, LAST) lists the segments of the manifest's generation; load() replays
    # them in order on top of the snapshot.  A segment or list left behind by a crash before that replace is ignored.
    def save_delta(self, prefix: str) -> bool:
        """Returns False (nothing written) when there is no snapshot of THIS state under ``prefix`` to append to, or the index
        cannot hand its rows out (``get_rows``): the caller then takes a snapshot (``save``)."""
        with self.lock:
            get_rows = getattr(self.index, "get_rows", None)
            if get_rows is None or self.generation == 0 or self._manifest_generation_only(prefix) != self.generation:
                return False
            if self._delta_broken:          # a compaction since the snapshot: _ckpt_rows / the log's "dead" are old ordinals
                return False
            rows_now = int(self.index.rows)
            n_new = rows_now - self._ckpt_rows
            if n_new == 0 and not self._dead_since and not self._structured_dirty:
                return True
            vecs = np.ascontiguousarray(get_rows(self._ckpt_rows, n_new), dtype=np.float32) if n_new else np.zeros((0, 0), np.float32)
            head = {"version": 1, "generation": self.generation, "seq": self._delta_seq + 1, "first_row": self._ckpt_rows,
                    "n": n_new, "dim": int(vecs.shape[1]) if n_new else 0,
                    "row_doc": self.row_doc[self._ckpt_rows:rows_now] + [None] * max(0, rows_now - len(self.row_doc)),
                    "dead": sorted(set(self._dead_since)),
                    "structured": {k: self.structured[k] for k in sorted(self._structured_dirty) if k in self.structured},
                    "patients": self.patients.names(), "doc_types": self.doc_types.names(),
                    "rows_after": rows_now, "live_after": int(self.index.count)}
            if self.attrs and hasattr(self.index, "get_attr"):   # the appended rows' column values, read back like the rows
                head["attrs"] = dict(self.attrs.to_meta(), values=[
                    self.index.get_attr(c, self._ckpt_rows, n_new).tolist() for c in range(len(self.attrs))])
            d, base = os.path.dirname(prefix) or ".", os.path.basename(prefix)
            seg = f"{base}.g{self.generation:06d}.d{self._delta_seq + 1:06d}.delta"
            tmp = os.path.join(d, seg + ".tmp")
            with open(tmp, "wb") as f:
                f.write(json.dumps(head).encode("utf-8") + b"\n")
                f.write(vecs.tobytes())
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, os.path.join(d, seg))
            listing = self._read_delta_list(prefix)
            segs = listing["segments"] if listing and listing.get("generation") == self.generation else []
            tmp_l = prefix + ".deltas.json.tmp"
            with open(tmp_l, "w", encoding="utf-8") as f:
                json.dump({"generation": self.generation, "segments": segs + [seg]}, f)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp_l, prefix + ".deltas.json")
            _fsync_dir(d)
            self._ckpt_rows, self._dead_since, self._structured_dirty = rows_now, [], set()
            self._delta_seq += 1
            return True

    @staticmethod
    def _read_delta_list(prefix: str) -> Optional[dict]:
        try:
            with open(prefix + ".deltas.json", encoding="utf-8") as f:
                return json.load(f)
        except (OSError, ValueError):
            return None

    @classmethod
    def _remove_deltas(cls, prefix: str, keep_generation: Optional[int]) -> None:
        d, base = os.path.dirname(prefix) or ".", os.path.basename(prefix)
        try:
            for fn in os.listdir(d):
                if fn.startswith(base + ".g") and (fn.endswith(".delta") or fn.endswith(".delta.tmp")):
                    if keep_generation is None or not fn.startswith(f"{base}.g{keep_generation:06d}."):
                        os.remove(os.path.join(d, fn))
            if keep_generation is None and os.path.exists(prefix + ".deltas.json"):
                os.remove(prefix + ".deltas.json")
        except OSError:
            pass

    @staticmethod
    def _manifest_generation_only(prefix: str) -> int:
        try:
            with open(prefix + ".meta.json", encoding="utf-8") as f:
                return int(json.load(f).get("generation", 0))
        except (OSError, ValueError, TypeError):
            return 0

    def _replay_deltas(self, prefix: str) -> None:
        """load(): the segments `<prefix>.deltas.json` lists for this generation, in order, on top of the snapshot."""
        listing = self._read_delta_list(prefix)
        if not listing or int(listing.get("generation", -1)) != self.generation:
            return
        d = os.path.dirname(prefix) or "."
        for k, seg in enumerate(listing.get("segments", [])):
            with open(os.path.join(d, seg), "rb") as f:
                head = json.loads(f.readline().decode("utf-8"))
                n, dim = int(head["n"]), int(head["dim"])
                raw = f.read(n * dim * 4)
            if int(head.get("generation", -1)) != self.generation or int(head.get("seq", -1)) != k + 1 or \
                    int(head["first_row"]) != int(self.index.rows) or len(raw) != n * dim * 4 or len(head["row_doc"]) != n:
                raise ValueError(f"{seg}: delta segment does not continue the index (generation / order / rows / length)")
            for pname in head["patients"]:
                self.patients.encode(pname)
            for t in head.get("doc_types", []):
                self.doc_types.encode(t)
            if n:
                vecs = np.frombuffer(raw, dtype=np.float32).reshape(n, dim).copy()
                tags = np.array([self.tag_of(doc) if doc is not None else 0 for doc in head["row_doc"]], dtype=np.int32)
                first = self.index.add(vecs, tags=tags, normalize=False)     # the stored bits, not re-normalised
                if int(first) != int(head["first_row"]):
                    raise ValueError(f"{seg}: rows landed at {first}, expected {head['first_row']}")
            seg_attrs = head.get("attrs")
            if seg_attrs and self.attrs:
                if [list(p) for p in self.attrs.fields] != [list(p) for p in seg_attrs.get("fields", [])]:
                    raise ValueError(f"{seg}: the segment's attribute schema is not the snapshot's")
                self.attrs.absorb(seg_attrs)
                for c, vals in enumerate(seg_attrs.get("values", [])):
                    if n:
                        self.index.set_attr(c, int(head["first_row"]), np.asarray(vals, dtype=np.int32))
            for r in head["dead"]:
                self.index.delete(int(r))
                doc = self.row_doc[int(r)]
                if doc is not None and self.doc_row.get(doc.get("doc_id")) == int(r):
                    del self.doc_row[doc.get("doc_id")]
                self.row_doc[int(r)] = None
            for i, doc in enumerate(head["row_doc"]):
                r = int(head["first_row"]) + i
                self.row_doc.append(doc)
                if doc is None:
                    self.index.delete(r)
                else:
                    self.doc_row[doc["doc_id"]] = r
            self.structured.update(head["structured"])
            if int(self.index.rows) != int(head["rows_after"]) or int(self.index.count) != int(head["live_after"]):
                raise ValueError(f"{seg}: after the replay the index holds {self.index.rows} rows / {self.index.count} live, "
                                 f"the segment recorded {head['rows_after']} / {head['live_after']}")
            self._delta_seq = k + 1
        self._ckpt_rows = int(self.index.rows)

    @staticmethod
    def _manifest_generation(prefix: str) -> int:
        """Generation of the manifest on disk (0 when there is none / it is unreadable); a vector file of a later
        generation left behind by a crash between the two renames counts too."""
        gen = 0
        try:
            with open(prefix + ".meta.json", encoding="utf-8") as f:
                gen = int(json.load(f).get("generation", 0))
        except (OSError, ValueError, TypeError):
            pass
        d, base = os.path.dirname(prefix) or ".", os.path.basename(prefix)
        try:
            for fn in os.listdir(d):
                if fn.startswith(base + ".g") and fn.endswith(".rass"):
                    digits = fn[len(base) + 2:-5]
                    if digits.isdigit():
                        gen = max(gen, int(digits))
        except OSError:
            pass
        return gen

    @staticmethod
    def _manifest_vectors(prefix: str) -> Optional[str]:
        try:
            with open(prefix + ".meta.json", encoding="utf-8") as f:
                meta = json.load(f)
            return os.path.join(os.path.dirname(prefix) or ".", meta["vectors"]) if "vectors" in meta else None
        except (OSError, ValueError, KeyError):
            return None

    @classmethod
    def load(cls, name: str, prefix: str, index_loader) -> "IndexState":
        """``index_loader(name, path) -> FlatIndex-like`` (e.g. ``Engine.load_index``).  The pair is
        rejected when the manifest and the vector file disagree (rows, tombstones)."""
        with open(prefix + ".meta.json", encoding="utf-8") as f:
            meta = json.load(f)
        vec = os.path.join(os.path.dirname(prefix) or ".", meta["vectors"]) if "vectors" in meta else prefix + ".rass"
        index = index_loader(name, vec)
        try:    # a restored index takes the configured candidate mode like a new one (the default factory below)
            from . import config
            if config.RASS_PREFILTER != "off" and hasattr(index, "set_prefilter") and not getattr(index, "prefilter", False):
                index.set_prefilter(config.RASS_PREFILTER)
        except Exception:   # e.g. a bf16 corpus: no prefilter mode — the exact scan serves
            pass
        row_doc = meta["row_doc"]
        rows, live = int(index.rows), int(index.count)
        dead = sum(1 for d in row_doc if d is None)
        if len(row_doc) != rows or rows - live != dead or meta.get("rows", rows) != rows or meta.get("live", live) != live:
            raise ValueError(f"{prefix}: manifest and vector file disagree (manifest rows {len(row_doc)} / tombstones "
                             f"{dead}, vector file rows {rows} / tombstones {rows - live}): refusing to load")
        st = cls(name, index)
        st.row_doc = row_doc
        st.structured = meta["structured"]
        st.generation = int(meta.get("generation", 0))
        for p in meta["patients"]:
            st.patients.encode(p)
        for t in meta.get("doc_types", []):
            st.doc_types.encode(t)
        st.doc_row = {d["doc_id"]: r for r, d in enumerate(st.row_doc) if d is not None}
        loaded = AttrSchema.from_meta(meta.get("attrs"))     # a manifest without the key: no schema
        if loaded != st.attrs:
            logger.warning(f"{prefix}: the saved attribute schema {loaded.fields} differs from the configured one "
                           f"{st.attrs.fields}; keeping the saved one (it describes the columns of the file)")
        st.attrs = loaded
        st._ckpt_rows = rows
        st._replay_deltas(prefix)
        return st


def _fsync_dir(path: str) -> None:
    try:
        fd = os.open(path, os.O_RDONLY)
        try:
            os.fsync(fd)
        finally:
            os.close(fd)
    except OSError:
        pass


class Registry:
    """index name -> IndexState; the engine behind it is created lazily on first use."""

    def __init__(self):
        self._lock = threading.Lock()
        self._states: Dict[str, IndexState] = {}
        self._factory = None

    def set_index_factory(self, factory) -> None:
        """``factory(index_name) -> FlatIndex-like``.  Default: the process-global HIP engine."""
        with self._lock:
            self._factory = factory

    def _default_factory(self, name: str):
        from . import config
        from .engine import Engine
        eng = Engine.get(config.RASS_DEVICE, config.EMBED_DIM)
        if config.RASS_IVF_NLIST > 0:       # approximate index + flat delta for later inserts (ivf.IvfBackedIndex)
            from .ivf import open_backed_index
            idx = open_backed_index(eng, name)
        else:
            idx = eng.open_index(name)
        if config.RASS_PREFILTER != "off":  # searches of k <= 16: bf16 / int8 candidate scan + exact fp32 re-rank (engine.set_prefilter)
            idx.set_prefilter(config.RASS_PREFILTER)
        return idx

    def get(self, name: str, create: bool = True) -> Optional[IndexState]:
        with self._lock:
            st = self._states.get(name)
            if st is None and create:
                factory = self._factory or self._default_factory
                st = self._states[name] = IndexState(name, factory(name))
            return st

    def put(self, st: IndexState) -> None:
        with self._lock:
            self._states[st.name] = st

    def exists(self, name: str) -> bool:
        with self._lock:
            return name in self._states

    def drop(self, name: str) -> None:
        with self._lock:
            self._states.pop(name, None)

    def clear(self) -> None:
        with self._lock:
            self._states.clear()


REGISTRY = Registry()
