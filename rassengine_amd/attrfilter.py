"""The filter compiler behind ``HipIndexer.semantic_search_filtered``: an OpenSearch filter (``term``, ``terms``, ``range``,
``exists``, ``bool`` with ``must`` / ``filter`` / ``should`` / ``must_not``, nested freely) over the fields an index holds —
the attribute columns of its ``docstore.AttrSchema`` and the two tag fields ``patientId`` / ``doc_type`` — becomes a small
PLAN of bitmap-builder calls, and ``run_plan`` issues them on a ``FlatIndex``.

Negations are pushed down to the leaves (a clause carries a ``negate`` flag, under which a missing value passes: OpenSearch's
``must_not`` over an absent field).  A plan node is one of

* ``("all", [clause, ...])`` / ``("any", [clause, ...])``: ONE ``allow_from_attr_clauses`` call (ALL / ANY; a longer list in
  chunks of 64), clause = ``(col, lo, hi, negate)``.  A ``must`` of leaves folds into one ``all``, a ``should`` of leaves or
  a ``terms`` into one ``any``; ``("all", [])`` is every live row, ``("any", [])`` none;
* ``("tags", values, mask, negate)``: ``allow_from_tag_values`` (``patientId`` / ``doc_type``);
* ``("and", [node, ...])`` / ``("or", [node, ...])``: the children one after the other into the same bitmap through the
  builder's ``combine``, a nested child through a second bitmap and ``allow_combine``.

``should`` means "at least one" wherever it stands (``minimum_should_match`` other than 1 is refused).  Pure Python + numpy:
no GPU is touched before ``run_plan``.
"""
from __future__ import annotations

import datetime as _dt
from typing import Any, List, Optional, Tuple

import numpy as np

from .docstore import (ATTR_MAX, ATTR_MIN, TAG_DOCTYPE_MASK, TAG_DOCTYPE_SHIFT, TAG_PATIENT_MASK, AttrSchema, PatientDictionary,
                       date_bound_days)

MAX_CLAUSES = 64        # RASS_MAX_ATTR_CLAUSES: clauses per query per builder call
NOTHING = (1, 0)        # lo > hi: holds for no row
EXISTS = (ATTR_MIN, ATTR_MAX)


def _as_list(x: Any, what: str) -> List[Any]:
    if isinstance(x, dict):
        return [x]
    if isinstance(x, (list, tuple)):
        return list(x)
    raise ValueError(f"{what}: expected a clause or a list of clauses, got {type(x).__name__}")


def _one_field(body: Any, what: str) -> Tuple[str, Any]:
    if not isinstance(body, dict) or len(body) != 1:
        raise ValueError(f"{what}: expected exactly one field, got {body!r}")
    return next(iter(body.items()))


class Compiler:
    def __init__(self, schema: Optional[AttrSchema], patients: PatientDictionary, doc_types: PatientDictionary,
                 now: Optional[_dt.datetime] = None):
        self.schema = schema if schema is not None else AttrSchema()
        self.patients, self.doc_types = patients, doc_types
        self.now = now if now is not None else self.schema.clock()

    # ---- leaves
    def _tag_codes(self, field: str, values: List[Any]) -> Tuple[List[int], int]:
        if field == "patientId":
            codes = {self.patients.lookup(v) for v in values}
            return sorted(c for c in codes if c is not None), TAG_PATIENT_MASK
        codes = {self.doc_types.lookup(v) for v in values}
        return sorted(c << TAG_DOCTYPE_SHIFT for c in codes if c is not None), TAG_DOCTYPE_MASK

    def _equals(self, field: str, col: int, kind: str, value: Any) -> Tuple[int, int]:
        """(lo, hi) of `field == value`; a value that cannot be stored in the column matches nothing."""
        if isinstance(value, dict) and "value" in value:      # {"term": {"f": {"value": v}}}
            value = value["value"]
        if value is None:
            return NOTHING
        if kind == "keyword":
            code = self.schema.dicts[field].lookup(value)     # never indexed: matches nothing
            return (code, code) if code is not None else NOTHING
        if kind == "int":
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError(f"term on the int field {field!r} needs an integer, got {value!r}")
            return (int(value), int(value)) if ATTR_MIN <= int(value) <= ATTR_MAX else NOTHING
        days = date_bound_days(value, self.now)
        if days is None:
            raise ValueError(f"term on the date field {field!r}: {value!r} is not a date")
        return (days, days) if ATTR_MIN <= days <= ATTR_MAX else NOTHING

    def _terms(self, field: str, values: List[Any], negate: bool):
        if field in ("patientId", "doc_type"):
            codes, mask = self._tag_codes(field, values)
            return ("tags", codes, mask, negate)
        where = self.schema.column(field)
        if where is None:
            raise ValueError(f"unknown filter field {field!r}: not patientId, doc_type or one of the attribute fields "
                             f"{[f for f, _ in self.schema.fields]}")
        col, kind = where
        bounds = sorted({self._equals(field, col, kind, v) for v in values} - {NOTHING})
        if not bounds:
            return ("all", []) if negate else ("any", [])
        # not (a or b) = (not a) and (not b)
        return ("all" if negate else "any", [(col, lo, hi, 1 if negate else 0) for lo, hi in bounds])

    def _range(self, field: str, body: Any, negate: bool):
        if field in ("patientId", "doc_type"):
            raise ValueError(f"unsupported clause: range on the tag field {field!r}")
        where = self.schema.column(field)
        if where is None:
            raise ValueError(f"unknown filter field {field!r}: not one of the attribute fields {[f for f, _ in self.schema.fields]}")
        col, kind = where
        if kind == "keyword":
            raise ValueError(f"unsupported clause: range on the keyword field {field!r}")
        if not isinstance(body, dict):
            raise ValueError(f"range on {field!r}: expected bounds, got {body!r}")
        lo, hi = ATTR_MIN, ATTR_MAX
        for op, raw in body.items():
            if op in ("format", "time_zone", "boost", "relation"):
                if op == "time_zone":
                    raise ValueError("unsupported range option: time_zone (bounds are UTC days)")
                continue
            if op not in ("gte", "gt", "lte", "lt"):
                raise ValueError(f"unsupported range bound {op!r} on {field!r}")
            if raw is None:
                continue
            if kind == "int":
                if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)):
                    raise ValueError(f"range on the int field {field!r} needs integer bounds, got {raw!r}")
                v = int(raw)
            else:
                v = date_bound_days(raw, self.now)
                if v is None:
                    raise ValueError(f"range on the date field {field!r}: {raw!r} is not a date or now±N(d|w|M|y)")
            if op == "gt":
                v += 1          # whole values: > v is >= v + 1 (a date: the next day)
            if op == "lt":
                v -= 1
            if op in ("gte", "gt"):
                lo = max(lo, v)
            else:
                hi = min(hi, v)
        lo, hi = (max(lo, ATTR_MIN), min(hi, ATTR_MAX))
        if lo > hi:
            lo, hi = NOTHING
        return ("all", [(col, lo, hi, 1 if negate else 0)])

    def _exists(self, body: Any, negate: bool):
        if not isinstance(body, dict) or "field" not in body:
            raise ValueError(f"exists: expected {{'field': name}}, got {body!r}")
        field = body["field"]
        if field in ("patientId", "doc_type"):
            d = self.patients if field == "patientId" else self.doc_types
            return self._terms(field, d.names(), negate)
        where = self.schema.column(field)
        if where is None:
            raise ValueError(f"unknown filter field {field!r}")
        return ("all", [(where[0], EXISTS[0], EXISTS[1], 1 if negate else 0)])

    # ---- the tree
    def compile(self, where: Any, negate: bool = False):
        """The plan of one clause (or of a list of clauses: their conjunction)."""
        if isinstance(where, (list, tuple)):
            return self._junction([self.compile(c, negate) for c in where], "or" if negate else "and")
        if not isinstance(where, dict) or len(where) != 1:
            raise ValueError(f"a filter clause is a dict with one key (term, terms, range, exists, bool), got {where!r}")
        kind, body = next(iter(where.items()))
        if kind == "term":
            field, value = _one_field(body, "term")
            return self._terms(field, [value], negate)
        if kind == "terms":
            body = {f: v for f, v in body.items() if f != "boost"} if isinstance(body, dict) else body
            field, values = _one_field(body, "terms")
            if not isinstance(values, (list, tuple)):
                raise ValueError(f"terms on {field!r}: expected a list of values")
            return self._terms(field, list(values), negate)
        if kind == "range":
            field, bounds = _one_field(body, "range")
            return self._range(field, bounds, negate)
        if kind == "exists":
            return self._exists(body, negate)
        if kind == "bool":
            return self._bool(body, negate)
        raise ValueError(f"unsupported filter clause {kind!r} (supported: term, terms, range, exists, bool)")

    def _bool(self, body: Any, negate: bool):
        if not isinstance(body, dict):
            raise ValueError(f"bool: expected a dict, got {body!r}")
        parts = []      # the conjunction, un-negated
        for key, sub in body.items():
            if key in ("must", "filter"):
                parts += [("pos", c) for c in _as_list(sub, key)]
            elif key == "must_not":
                parts += [("neg", c) for c in _as_list(sub, key)]
            elif key == "should":
                if _as_list(sub, key):
                    parts.append(("should", _as_list(sub, key)))
            elif key == "minimum_should_match":
                if sub not in (1, "1"):
                    raise ValueError("unsupported: minimum_should_match other than 1 (should means at least one)")
            elif key == "boost":
                continue
            else:
                raise ValueError(f"unsupported bool key {key!r}")
        nodes = []
        for how, c in parts:
            if how == "should":     # not (a or b) = not a and not b
                nodes.append(self._junction([self.compile(s, negate) for s in c], "and" if negate else "or"))
            else:
                nodes.append(self.compile(c, negate != (how == "neg")))
        return self._junction(nodes, "or" if negate else "and")

    @staticmethod
    def _junction(nodes: List[tuple], op: str):
        """``and`` / ``or`` of plan nodes with the leaves folded: an ``and`` takes the clauses of its ``all`` children (and of
        one-clause ``any`` children) into one ``all``, an ``or`` likewise into one ``any``; nested junctions of the same kind
        are flattened."""
        leaf = "all" if op == "and" else "any"
        clauses: List[tuple] = []
        rest: List[tuple] = []
        for n in nodes:
            if n[0] == op:
                for m in n[1]:
                    (clauses.extend(m[1]) if m[0] == leaf else rest.append(m))
            elif n[0] == leaf or (n[0] in ("all", "any") and len(n[1]) == 1):
                clauses.extend(n[1])
            else:
                rest.append(n)
        # an empty leaf of the OTHER kind decides the junction: and(..., nothing) = nothing, or(..., everything) = everything
        absorbing = ("any", []) if op == "and" else ("all", [])
        if any(n[0] == absorbing[0] and not n[1] for n in rest):
            return absorbing
        if not rest:
            return (leaf, clauses)
        folded = ([(leaf, clauses)] if clauses else []) + rest
        return folded[0] if len(folded) == 1 else (op, folded)


def compile_filter(where: Any, schema: Optional[AttrSchema], patients: PatientDictionary, doc_types: PatientDictionary,
                   now: Optional[_dt.datetime] = None):
    """``where`` (an OpenSearch filter clause, or a list of them) as a plan; ``ValueError`` names an unknown field or an
    unsupported clause."""
    return Compiler(schema, patients, doc_types, now).compile(where)


def compile_should(should: Any, schema: Optional[AttrSchema], patients: PatientDictionary, doc_types: PatientDictionary,
                   now: Optional[_dt.datetime] = None) -> List[Tuple[int, int, int, int, float]]:
    """The weighted should-clauses of ``HipIndexer.semantic_search_boosted`` as ``(col, lo, hi, negate, weight)`` rows for
    ``FlatIndex.bonus_from_attr_clauses``, in list order.  ``should`` is ``[(leaf, weight), ...]``; a leaf is ``term``,
    ``terms``, ``range`` (date math as in a filter) or ``exists`` over an attribute field, with a filter's encodings.  A
    ``terms`` leaf becomes one clause per distinct value (a row holds one value, so it earns the weight once); a value that
    was never indexed contributes no clause.  ``patientId`` / ``doc_type`` leaves (tag fields: no column), ``bool`` and every
    other node raise ``ValueError``, as does a weight that is not a finite number."""
    comp = Compiler(schema, patients, doc_types, now)
    out: List[Tuple[int, int, int, int, float]] = []
    for item in should or []:
        if not isinstance(item, (list, tuple)) or len(item) != 2:
            raise ValueError(f"a should entry is (leaf filter, weight), got {item!r}")
        leaf, weight = item
        if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not np.isfinite(weight):
            raise ValueError(f"a should weight must be a finite number, got {weight!r}")
        if not isinstance(leaf, dict) or len(leaf) != 1:
            raise ValueError(f"a should leaf is a dict with one key (term, terms, range, exists), got {leaf!r}")
        kind, body = next(iter(leaf.items()))
        if kind not in ("term", "terms", "range", "exists"):
            raise ValueError(f"unsupported should clause {kind!r} (supported leaves: term, terms, range, exists)")
        if kind == "exists":
            field = body.get("field") if isinstance(body, dict) else None
        else:
            fields = [f for f in body if f != "boost"] if isinstance(body, dict) else []
            field = fields[0] if len(fields) == 1 else None
        if field in ("patientId", "doc_type"):
            raise ValueError(f"unsupported should clause: {kind} on the tag field {field!r} (use filter_clause / patient_id / where)")
        node = comp.compile(leaf)
        if node[0] not in ("all", "any"):
            raise ValueError(f"unsupported should clause {leaf!r}")
        out += [(c, lo, hi, neg, float(weight)) for c, lo, hi, neg in node[1]]
    return out


DECAY_KINDS = ("gauss", "exp", "linear")
FN_MODIFIERS = ("none", "log", "log1p", "log2p", "ln", "ln1p", "ln2p", "square", "sqrt", "reciprocal")
_DAY_SPAN = {"d": 1, "w": 7}


def _number(x: Any, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
        raise ValueError(f"{what} must be a finite number, got {x!r}")
    return float(x)


def _day_span(x: Any, what: str) -> float:
    """A decay ``scale`` / ``offset`` on a date field, in days: ``"30d"`` / ``"2w"``, or a number of days.  The column holds
    whole UTC days, so a span in hours, minutes, seconds or milliseconds is refused."""
    if isinstance(x, str):
        s = x.strip()
        if len(s) >= 2 and s[:-1].isdigit() and s[-1] in _DAY_SPAN:
            return float(int(s[:-1]) * _DAY_SPAN[s[-1]])
        if s[:-1].isdigit() or s[:-2].isdigit():
            raise ValueError(f"{what}: {x!r} is finer than a day (or not a d / w span): the date columns hold whole UTC days")
        raise ValueError(f"{what}: {x!r} is not a span like '30d' or '2w'")
    return _number(x, what)


def compile_functions(functions: Any, schema: Optional[AttrSchema], patients: PatientDictionary, doc_types: PatientDictionary,
                      now: Optional[_dt.datetime] = None) -> Tuple[List[dict], List[Any]]:
    """OpenSearch ``function_score.functions`` entries as (records, filter plans) for ``FlatIndex.fn_from_attr``.  An entry is
    ``{"gauss" | "exp" | "linear": {field: {"origin", "scale", "offset", "decay"}}}``, ``{"field_value_factor": {"field",
    "factor", "modifier", "missing"}}`` or ``{"weight": w}`` alone; each may carry a ``"filter"`` (a clause as
    ``compile_filter`` takes it) and a ``"weight"``.  Fields are the int and date attribute fields of the schema (a keyword
    field has no numeric value).  On a date field ``origin`` is a date as a ``range`` bound takes it (``YYYY-MM-DD``, ISO
    date-times, ``now``, ``now-30d``, with an optional ``/d`` rounding; default ``now``) and ``scale`` / ``offset`` are day
    spans (``"30d"``, ``"2w"``, or a number of days); a span finer than a day is a ``ValueError``.  ``decay`` defaults to 0.5,
    ``offset`` to 0.  A record is a dict ``{kind, col, weight, filter, ...}`` whose ``filter`` is None or an index into the
    returned list of filter PLANS (each entry's ``filter`` compiled once, as ``compile_filter`` compiles it): resolve each with
    ``run_plan`` and hand the bitmaps to ``fn_from_attr``.  A bare number as ``scale`` / ``offset`` on a date field is DAYS
    here (OpenSearch reads a bare number on a date as milliseconds).  Every malformed entry raises ``ValueError`` naming it.  Pure Python: no GPU is touched."""
    comp = Compiler(schema, patients, doc_types, now)
    records: List[dict] = []
    filters: List[Any] = []
    for entry in functions or []:
        if not isinstance(entry, dict):
            raise ValueError(f"a function entry is a dict, got {entry!r}")
        keys = [k for k in entry if k not in ("filter", "weight")]
        if len(keys) > 1:
            raise ValueError(f"a function entry holds one function, got {sorted(keys)}")
        rec: dict = {"weight": 1.0, "filter": None}
        if "weight" in entry:
            rec["weight"] = _number(entry["weight"], "a function's weight")
        if not keys:
            if "weight" not in entry:
                raise ValueError(f"a function entry without a function needs a weight, got {entry!r}")
            rec.update(kind="weight", col=0)
        elif keys[0] in DECAY_KINDS:
            field, body = _one_field(entry[keys[0]], keys[0])
            where = comp.schema.column(field)
            if where is None or where[1] == "keyword":
                raise ValueError(f"{keys[0]} decay needs an int or date attribute field, not {field!r}")
            if not isinstance(body, dict) or "scale" not in body:
                raise ValueError(f"{keys[0]} on {field!r}: expected {{origin, scale, offset, decay}}, got {body!r}")
            unknown = set(body) - {"origin", "scale", "offset", "decay"}
            if unknown:
                raise ValueError(f"{keys[0]} on {field!r}: unsupported option(s) {sorted(unknown)}")
            col, kind = where
            what = f"{keys[0]} on {field!r}"
            if kind == "date":
                raw = body.get("origin", "now")
                if isinstance(raw, str) and raw.strip().endswith("/d"):     # rounding down to the day: what the column holds
                    raw = raw.strip()[:-2]
                origin = date_bound_days(raw, comp.now)
                if origin is None:
                    raise ValueError(f"{what}: origin {body.get('origin')!r} is not a date or now±N(d|w|M|y)")
                scale, offset = _day_span(body["scale"], f"{what}: scale"), _day_span(body.get("offset", 0), f"{what}: offset")
            else:
                if "origin" not in body:
                    raise ValueError(f"{what}: an int field needs an origin")
                origin = _number(body["origin"], f"{what}: origin")
                scale, offset = _number(body["scale"], f"{what}: scale"), _number(body.get("offset", 0), f"{what}: offset")
            decay = _number(body.get("decay", 0.5), f"{what}: decay")
            if not scale > 0:
                raise ValueError(f"{what}: scale must be > 0, got {body['scale']!r}")
            if offset < 0:
                raise ValueError(f"{what}: offset must be >= 0, got {body.get('offset')!r}")
            if not 0 < decay < 1:
                raise ValueError(f"{what}: decay must be in (0, 1), got {decay!r}")
            rec.update(kind=keys[0], col=col, origin=float(origin), scale=scale, offset=offset, decay=decay)
        elif keys[0] == "field_value_factor":
            body = entry[keys[0]]
            if not isinstance(body, dict) or "field" not in body:
                raise ValueError(f"field_value_factor: expected {{field, factor, modifier, missing}}, got {body!r}")
            unknown = set(body) - {"field", "factor", "modifier", "missing"}
            if unknown:
                raise ValueError(f"field_value_factor: unsupported option(s) {sorted(unknown)}")
            where = comp.schema.column(body["field"])
            if where is None or where[1] == "keyword":
                raise ValueError(f"field_value_factor needs an int or date attribute field, not {body['field']!r}")
            mod = body.get("modifier") or "none"
            if mod not in FN_MODIFIERS:
                raise ValueError(f"field_value_factor: modifier must be one of {FN_MODIFIERS}, not {mod!r}")
            rec.update(kind="field_value_factor", col=where[0], factor=_number(body.get("factor", 1.0), "field_value_factor: factor"),
                       modifier=mod, missing=None if body.get("missing") is None else _number(body["missing"], "field_value_factor: missing"))
        else:
            raise ValueError(f"unsupported function {keys[0]!r} (supported: gauss, exp, linear, field_value_factor, weight)")
        if entry.get("filter") is not None:
            rec["filter"] = len(filters)
            filters.append(comp.compile(entry["filter"]))     # malformed filters raise here, before any GPU work
        records.append(rec)
    return records, filters


def plan_calls(plan) -> int:
    """Builder calls a plan costs (for documentation and tests): one per 64 clauses of a leaf, one per tag set."""
    if plan[0] in ("all", "any"):
        return max(1, -(-len(plan[1]) // MAX_CLAUSES))
    if plan[0] == "tags":
        return 1
    return sum(plan_calls(n) for n in plan[1])


def run_plan(index, plan):
    """Evaluate a plan on a ``FlatIndex``: the device bitmap (one, shared by every query) of the rows it allows.  Every
    bitmap of the evaluation has the length of the first; the engine has finished with all of them on return."""
    import torch
    words: List[int] = []       # the length of the first bitmap, once there is one
    keep: List[Any] = []        # every bitmap stays allocated until the engine's stream has drained

    def new_bitmap():
        t = torch.empty((words[0],), dtype=torch.int32, device=f"cuda:{index.engine.device}")
        keep.append(t)
        return t

    def clauses_call(mode: str, clauses, combine: str, target):
        arr = np.array([(0, c, lo, hi, neg) for c, lo, hi, neg in clauses], dtype=np.int64).reshape(-1, 5)
        if target is None and not words:
            target = index.allow_from_attr_clauses(arr, nq=1, shared=True, mode=mode)
            words.append(int(target.shape[-1]))
            keep.append(target)
            return target
        if target is None:
            target, combine = new_bitmap(), "replace"
        return index.allow_from_attr_clauses(arr, nq=1, shared=True, mode=mode, combine=combine, allow=target)

    def merge(target, node, combine: str):
        return index.allow_combine(target, emit(node, None, "replace"), combine)

    def emit(node, target, combine: str):
        """A new bitmap holding the node (``target`` None), or ``target`` and / or the node, in place."""
        assert target is None or combine in ("and", "or")
        kind = node[0]
        if kind in ("all", "any"):
            chunks = [node[1][i:i + MAX_CLAUSES] for i in range(0, len(node[1]), MAX_CLAUSES)] or [[]]
            follow = "and" if kind == "all" else "or"
            if target is not None and len(chunks) > 1 and combine != follow:
                return merge(target, node, combine)     # (c1 and c2) or target: through a bitmap of its own
            for chunk in chunks:
                target = clauses_call(kind, chunk, combine, target)
                combine = follow
            return target
        if kind == "tags":
            _, values, mask, negate = node
            tags = index.allow_from_tag_values(np.asarray(values, dtype=np.int32), mask, words=words[0] if words else None)
            keep.append(tags)
            if not words:
                words.append(int(tags.shape[-1]))
            if negate:      # not x = the live rows and-not x
                tags = index.allow_combine(clauses_call("all", [], "replace", None), tags, "andnot")
            return tags if target is None else index.allow_combine(target, tags, combine)
        if target is not None and combine != kind:      # an `or` under an `and` (or the reverse): a bitmap of its own
            return merge(target, node, combine)
        for child in sorted(node[1], key=lambda n: n[0] in ("all", "any")):     # nested children first, leaves refine
            target = emit(child, target, kind)
        return target

    out = emit(plan, None, "replace")
    index.engine.synchronize()
    return out
