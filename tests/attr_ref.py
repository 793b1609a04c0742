"""numpy / plain-Python restatement of the attribute filter, for the tests: what ``rass_index_allow_from_attr_clauses`` must
write word for word (``build``), what a compiled plan allows (``eval_plan``) and what an OpenSearch filter means for a doc
dict (``doc_matches``).  Nothing here imports the engine's own path."""
import calendar
import datetime as dt

import numpy as np

MISSING = -(1 << 31)
INT_MIN, INT_MAX = MISSING + 1, (1 << 31) - 1
ALL, ANY = 0, 1
REPLACE, AND, OR = 0, 1, 2


def pack(bits, words):
    """bool [nb, n] -> uint32 [nb, words]: bit r & 31 of word r >> 5 = row r; n <= 32 words."""
    bits = np.asarray(bits, dtype=bool)
    padded = np.zeros((bits.shape[0], words * 32), dtype=bool)
    padded[:, :bits.shape[1]] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32)


def unpack(words, n):
    w = np.ascontiguousarray(np.asarray(words).astype("<u4"))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def holds(values, lo, hi, negate):
    """One clause over one column (None = never set = all missing)."""
    v = np.asarray(values, dtype=np.int64)
    return ((v != MISSING) & (lo <= v) & (v <= hi)) != bool(negate)


def allowed(cols, tags, clauses, nq, mode):
    """bool [nq, n]: the rows each query allows.  ``cols``: {col: int32 [n]} (a column not in it was never set)."""
    n = len(tags)
    out = np.ones((nq, n), dtype=bool) if mode == ALL else np.zeros((nq, n), dtype=bool)
    for q, col, lo, hi, neg in np.asarray(clauses, dtype=np.int64).reshape(-1, 5):
        h = holds(cols[col] if col in cols else np.full(n, MISSING), lo, hi, neg)
        out[q] = (out[q] & h) if mode == ALL else (out[q] | h)
    return out & (np.asarray(tags) != -1)[None, :]


def build(cols, tags, clauses, nq, n_bitmaps, mode, combine, prior, bits=None):
    """The words the builder must leave: ``prior`` is uint32 [n_bitmaps, words] (what the bitmap held).  ``bits``: the
    result of ``allowed`` for these clauses, when the caller already has it."""
    new = pack(allowed(cols, tags, clauses, n_bitmaps, mode) if bits is None else bits, prior.shape[1])
    if combine == REPLACE:
        return new
    if combine == AND:
        return prior & new            # tail bits and surplus words of `new` are 0: they come out 0
    return prior | new                # ... and stay as they were


# ------------------------------------------------------------------------------------------------ compiled plans
def eval_plan(plan, cols, tags):
    """bool [n]: the live rows a plan of ``attrfilter.compile_filter`` allows."""
    tags = np.asarray(tags)
    live = tags != -1
    kind = plan[0]
    if kind in ("all", "any"):
        cl = [(0, c, lo, hi, neg) for c, lo, hi, neg in plan[1]]
        return allowed(cols, tags, cl, 1, ALL if kind == "all" else ANY)[0]
    if kind == "tags":
        _, values, mask, negate = plan
        hit = np.isin(tags & mask, np.asarray(values, dtype=np.int64)) & live
        return (live & ~hit) if negate else hit
    parts = [eval_plan(p, cols, tags) for p in plan[1]]
    out = parts[0]
    for p in parts[1:]:
        out = (out & p) if kind == "and" else (out | p)
    return out


# ------------------------------------------------------------------------------------------------ docs
def day_of(value):
    """days since 1970-01-01 UTC of a stored date value, None when it is none (plain datetime arithmetic)."""
    if isinstance(value, bool) or value is None:
        return None
    if isinstance(value, int):
        return value // 86_400_000
    try:
        if len(value) == 10:
            return (dt.date.fromisoformat(value) - dt.date(1970, 1, 1)).days
        when = dt.datetime.fromisoformat(value.replace("Z", "+00:00"))
    except (ValueError, AttributeError, TypeError):
        return None
    if when.tzinfo is None:
        when = when.replace(tzinfo=dt.timezone.utc)
    return (when.astimezone(dt.timezone.utc).date() - dt.date(1970, 1, 1)).days


def bound_day(value, now):
    if isinstance(value, str) and value.startswith("now"):
        rest = value[3:]
        if not rest:
            return (now.date() - dt.date(1970, 1, 1)).days
        n, unit = int(rest[:-1]), rest[-1]
        d = now.date()
        if unit == "d":
            d = d + dt.timedelta(days=n)
        elif unit == "w":
            d = d + dt.timedelta(days=7 * n)
        else:
            m = d.year * 12 + d.month - 1 + (12 * n if unit == "y" else n)
            y, mo = divmod(m, 12)
            d = dt.date(y, mo + 1, min(d.day, calendar.monthrange(y, mo + 1)[1]))
        return (d - dt.date(1970, 1, 1)).days
    return day_of(value)


def field_value(doc, field, kinds):
    """The comparable value of a doc's field: str (keyword, patientId, doc_type), int, day number; None = missing."""
    v = doc.get(field)
    kind = kinds.get(field, "keyword")
    if v is None or (kind == "keyword" and v == ""):
        return None
    if kind == "keyword":
        return str(v)
    if kind == "int":
        return int(v)
    return day_of(v)


def doc_matches(where, doc, kinds, now):
    """OpenSearch filter semantics over one doc dict.  ``kinds``: {field: keyword | int | date}; patientId and doc_type are
    keywords.  ``should`` = at least one; a missing field fails every positive clause and passes under must_not."""
    if isinstance(where, (list, tuple)):
        return all(doc_matches(w, doc, kinds, now) for w in where)
    (kind, body), = where.items()
    if kind == "bool":
        def lst(x):
            return [x] if isinstance(x, dict) else list(x)
        ok = all(doc_matches(c, doc, kinds, now) for key in ("must", "filter") for c in lst(body.get(key, [])))
        ok = ok and not any(doc_matches(c, doc, kinds, now) for c in lst(body.get("must_not", [])))
        sh = lst(body.get("should", []))
        return ok and (not sh or any(doc_matches(c, doc, kinds, now) for c in sh))
    if kind == "exists":
        return field_value(doc, body["field"], kinds) is not None
    (field, arg), = body.items()
    have = field_value(doc, field, kinds)
    fkind = kinds.get(field, "keyword")

    def want(x):
        return str(x) if fkind == "keyword" else int(x) if fkind == "int" else bound_day(x, now)
    if kind == "term":
        return have is not None and have == want(arg)
    if kind == "terms":
        return have is not None and any(have == want(a) for a in arg)
    if kind == "range":
        if have is None:
            return False
        for op, raw in arg.items():
            b = want(raw)
            if (op == "gte" and not have >= b) or (op == "gt" and not have > b) or (op == "lte" and not have <= b) or \
                    (op == "lt" and not have < b):
                return False
        return True
    raise AssertionError(kind)
