"""The host-side layers of the allow-list search, without a GPU: the bitmap pack / unpack helpers,
``HipIndexer.semantic_search_within`` over a stand-in index that answers ``allow_from_rows`` / ``allow_from_tag_values`` /
``search_allowed`` in numpy, the argument validation of ``FlatIndex.search_allowed`` (which refuses before any native call is
made), and the new entry points' presence in the header, the binding table and the built library."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from rassengine_amd import _native, config, indexer
from rassengine_amd.docstore import REGISTRY, TAG_DOCTYPE_MASK, TAG_DOCTYPE_SHIFT, TAG_PATIENT_MASK, IndexState
from rassengine_amd.engine import FlatIndex, pack_allow, unpack_allow

DIM = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("rass_index_search_allowed", "rass_index_search_allowed_device", "rass_index_allow_from_rows",
                    "rass_index_allow_from_tag_values", "rass_index_allow_plan")


# ---------------------------------------------------------------------------------------------- pack / unpack
@pytest.mark.parametrize("shape", [(0,), (1,), (31,), (32,), (33,), (64,), (1000,), (3, 100), (1, 32), (5, 0)])
def test_pack_unpack_round_trip(shape):
    rng = np.random.default_rng(sum(shape))
    m = rng.random(shape) < 0.4
    w = pack_allow(m)
    assert w.dtype == np.uint32 and w.shape == shape[:-1] + ((shape[-1] + 31) // 32,)
    assert np.array_equal(unpack_allow(w, shape[-1]), m)
    nb = int(np.prod(shape[:-1]))                            # 1 for a single mask
    flat_m, flat_w = m.reshape(nb, shape[-1]), w.reshape(nb, w.shape[-1])
    for b in range(flat_m.shape[0]):                         # bit r & 31 of word r >> 5, and nothing else
        for r in range(shape[-1]):
            assert bool((int(flat_w[b, r >> 5]) >> (r & 31)) & 1) == bool(flat_m[b, r])
        assert sum(bin(int(x)).count("1") for x in flat_w[b]) == int(flat_m[b].sum())


def test_pack_unpack_refuse_bad_shapes():
    with pytest.raises(ValueError):
        pack_allow(np.zeros((2, 2, 2), dtype=bool))
    with pytest.raises(ValueError):
        unpack_allow(np.zeros(2, dtype=np.uint32), 65)
    assert unpack_allow(np.array([0xFFFFFFFF, 1], dtype=np.uint32), 40).tolist() == [True] * 33 + [False] * 7


# ---------------------------------------------------------------------------------------------- the stand-in index
class StandInIndex:
    """``FlatIndex``'s write path, compaction and allow-list methods in numpy: a bitmap is ``pack_allow`` words."""

    def __init__(self):
        self.x = np.zeros((0, DIM), dtype=np.float32)
        self.tags = np.zeros(0, dtype=np.int32)
        self.layout_epoch = 0
        self.calls = []
        self.compact_during_next = 0     # that many coming searches see the index compacted under them
        self.compact_for_real_before_next_search = None   # an IndexState to compact between bitmap and search
        self.before_next_search = None   # called once at the start of the next search: an ingest landing after the build

    rows = property(lambda self: self.x.shape[0])
    count = property(lambda self: int(np.count_nonzero(self.tags != -1)))

    def add(self, vecs, tags=None, normalize=True):
        v = np.asarray(vecs, dtype=np.float32)
        v = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
        first = self.rows
        self.x = np.concatenate([self.x, v.astype(np.float32)])
        self.tags = np.concatenate([self.tags, np.asarray(tags, dtype=np.int32)])
        return first

    def delete(self, row):
        self.tags[row] = -1

    def compact(self):
        live = self.tags != -1
        new_row = np.where(live, np.cumsum(live) - 1, -1).astype(np.int64)
        self.x, self.tags = self.x[live], self.tags[live]
        self.layout_epoch += 1
        return new_row

    def allow_from_rows(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        m = np.zeros(self.rows, dtype=bool)
        m[rows[(rows >= 0) & (rows < self.rows)]] = True
        self.calls.append(dict(fn="rows", rows=rows.tolist()))
        return pack_allow(m)

    def allow_from_tag_values(self, values, mask):
        values = np.asarray(values, dtype=np.int32)
        self.calls.append(dict(fn="tags", values=sorted(values.tolist()), mask=int(mask)))
        return pack_allow(np.isin(self.tags & mask, values) & (self.tags != -1))

    def search_allowed(self, queries, k, allow, q_filter=None, q_filter_mask=None):
        self.calls.append(dict(fn="search", k=k, q_filter=q_filter, q_filter_mask=q_filter_mask, words=int(np.asarray(allow).shape[-1])))
        if self.before_next_search is not None:
            hook, self.before_next_search = self.before_next_search, None
            hook()
        if self.compact_for_real_before_next_search is not None:
            st, self.compact_for_real_before_next_search = self.compact_for_real_before_next_search, None
            st.compact()
        if self.compact_during_next > 0:
            self.compact_during_next -= 1
            self.layout_epoch += 1
        bits = unpack_allow(allow, min(self.rows, allow.shape[-1] * 32))
        bits = np.concatenate([bits, np.zeros(self.rows - len(bits), dtype=bool)])
        q = np.asarray(queries, dtype=np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-9)
        out_s = np.full((q.shape[0], k), -np.inf, dtype=np.float32)
        out_i = np.full((q.shape[0], k), -1, dtype=np.int64)
        for j in range(q.shape[0]):
            s = (self.x @ q[j]).astype(np.float32)
            ok = (self.tags != -1) & bits
            if q_filter is not None and q_filter[j] >= 0:
                ok &= ((self.tags & q_filter_mask[j]) if q_filter_mask is not None else self.tags) == q_filter[j]
            rows = np.flatnonzero(ok)
            rows = rows[np.lexsort((rows, -s[rows]))][:k]
            out_s[j, :len(rows)], out_i[j, :len(rows)] = s[rows], rows
        return out_s, out_i

    def search(self, queries, k, q_filter=None, q_filter_mask=None):
        return self.search_allowed(queries, k, pack_allow(np.ones(self.rows, dtype=bool)), q_filter, q_filter_mask)


def _fill(name, idx):
    """40 chunks of four patients (p0..p3 by n % 4) and two doc types (every fifth chunk a 'note') whose cosine to the
    query e0 is known by construction and falls with n."""
    REGISTRY.put(IndexState(name, idx))
    cos = np.linspace(0.99, 0.02, 40)
    emb = np.zeros((40, DIM), dtype=np.float32)
    emb[:, 0] = cos
    emb[:, 1] = np.sqrt(1.0 - cos ** 2)
    docs = [{"doc_id": f"d{i}", "patientId": f"p{i % 4}", "doc_type": "note" if i % 5 == 0 else "unstructured", "n": i}
            for i in range(40)]
    indexer.add_documents(name, docs, emb * 5.0)
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 3.0
    return q, cos


@pytest.fixture
def world():
    name = "allow-cpu"
    idx = StandInIndex()
    q, cos = _fill(name, idx)
    yield indexer.HipIndexer(None, name), idx, q, cos
    REGISTRY.drop(name)


def ns(hits):
    return [d["n"] for d, _ in hits]


def test_terms_on_patients_and_doc_types_intersect(world):
    hip, idx, q, cos = world
    assert ns(hip.semantic_search_within(q, k=5, patient_ids=["p1", "p3"])) == [1, 3, 5, 7, 9]
    call = [c for c in idx.calls if c["fn"] == "tags"][-1]
    assert call["mask"] == TAG_PATIENT_MASK and len(call["values"]) == 2
    assert ns(hip.semantic_search_within(q, k=4, doc_types=["note"])) == [0, 5, 10, 15]
    assert [c for c in idx.calls if c["fn"] == "tags"][-1]["mask"] == TAG_DOCTYPE_MASK
    # both: patient in {p0, p1} AND doc type note -> n % 4 in {0, 1} and n % 5 == 0
    assert ns(hip.semantic_search_within(q, k=10, patient_ids=["p0", "p1"], doc_types=["note"])) == [0, 5, 20, 25]
    call = [c for c in idx.calls if c["fn"] == "tags"][-1]
    assert call["mask"] == TAG_PATIENT_MASK | TAG_DOCTYPE_MASK and len(call["values"]) == 2
    assert all(v >> TAG_DOCTYPE_SHIFT for v in call["values"])
    # ... AND the single-valued filters of semantic_search, as a tag filter next to the bitmap
    assert ns(hip.semantic_search_within(q, k=10, patient_ids=["p0", "p1"], doc_types=["note"], patient_id="p1")) == [5, 25]
    call = idx.calls[-1]
    assert call["fn"] == "search" and int(call["q_filter_mask"][0]) == TAG_PATIENT_MASK
    assert ns(hip.semantic_search_within(q, k=10, patient_ids=["p0", "p1"], filter_clause={"term": {"doc_type": "note"}})) == [0, 5, 20, 25]
    # k larger than the set: all of it
    assert ns(hip.semantic_search_within(q, k=100, patient_ids=["p2"])) == list(range(2, 40, 4))


def test_doc_ids_and_their_intersection_with_terms(world):
    hip, idx, q, cos = world
    assert ns(hip.semantic_search_within(q, k=10, doc_ids=["d30", "d7", "d12", "d7"])) == [7, 12, 30]
    assert [c for c in idx.calls if c["fn"] == "rows"][-1]["rows"] == [7, 12, 30]
    assert ns(hip.semantic_search_within(q, k=2, doc_ids=["d30", "d7", "d12"])) == [7, 12]
    assert ns(hip.semantic_search_within(q, k=10, doc_ids=["d30", "d7", "d12", "d8"], patient_ids=["p0", "p3"])) == [7, 8, 12]
    assert ns(hip.semantic_search_within(q, k=10, doc_ids=["d30", "d7", "d10"], doc_types=["note"])) == [10, 30]
    assert ns(hip.semantic_search_within(q, k=10, doc_ids=["d30", "d7", "d10"], patient_id="p3")) == [7]


def test_unknown_values_contribute_nothing_and_empty_intersections_are_empty(world):
    hip, idx, q, cos = world
    assert ns(hip.semantic_search_within(q, k=3, patient_ids=["p1", "nobody"])) == [1, 5, 9]
    assert ns(hip.semantic_search_within(q, k=3, doc_ids=["d4", "no-such-doc"])) == [4]
    n_search = sum(c["fn"] == "search" for c in idx.calls)
    assert hip.semantic_search_within(q, patient_ids=["nobody"]) == []
    assert hip.semantic_search_within(q, patient_ids=[]) == []
    assert hip.semantic_search_within(q, doc_types=["x-ray"]) == []
    assert hip.semantic_search_within(q, doc_ids=[]) == []
    assert hip.semantic_search_within(q, doc_ids=["no-such-doc"]) == []
    assert hip.semantic_search_within(q, doc_ids=["d1"], patient_ids=["p2"]) == []            # d1 is p1's
    assert hip.semantic_search_within(q, patient_ids=["p1"], patient_id="nobody") == []        # the term filter of _prepare
    assert hip.semantic_search_within(q, patient_ids=["p1"], patient_id="p1", filter_clause={"term": {"patientId": "p2"}}) == []
    assert hip.semantic_search_within(np.zeros(0), patient_ids=["p1"]) == []
    assert hip.semantic_search_within(None, patient_ids=["p1"]) == []
    assert indexer.HipIndexer(None, "no-such-index").semantic_search_within(q, patient_ids=["p1"]) == []
    assert sum(c["fn"] == "search" for c in idx.calls) == n_search                            # none of them searched
    # patient p1 and doc type note exist, but never together among d1 / d9: the search runs and finds nothing
    assert hip.semantic_search_within(q, patient_ids=["p2"], doc_types=["note"], patient_id="p1") == []
    # no list at all: the plain k-NN answer
    assert ns(hip.semantic_search_within(q, k=3)) == ns(hip.semantic_search(q, k=3)) == [0, 1, 2]


def test_an_overwritten_docs_old_row_is_never_allowed(world):
    hip, idx, q, cos = world
    rows_before = idx.rows
    indexer.add_documents(hip.index_name, [{"doc_id": "d0", "patientId": "p0", "doc_type": "unstructured", "n": 100}],
                          np.eye(1, DIM, 1, dtype=np.float32))       # orthogonal to the query: d0 now scores ~0
    hits = hip.semantic_search_within(q, k=5, doc_ids=["d0", "d4"])
    assert ns(hits) == [4, 100]
    assert [c for c in idx.calls if c["fn"] == "rows"][-1]["rows"] == [4, rows_before]      # the new row, not row 0
    assert 0 not in ns(hip.semantic_search_within(q, k=50, patient_ids=["p0"]))               # the tombstone never matches


@pytest.mark.parametrize("mode", ["opensearch", "cosine"])
def test_scores_are_in_the_units_semantic_search_returns(world, monkeypatch, mode):
    hip, idx, q, cos = world
    monkeypatch.setattr(config, "RASS_SCORE_MODE", mode)
    hits = hip.semantic_search_within(q, k=3, doc_ids=["d2", "d6", "d11"])
    assert ns(hits) == [2, 6, 11]
    for (_, score), c in zip(hits, (cos[2], cos[6], cos[11])):
        assert isinstance(score, float) and score == pytest.approx(indexer._score_out(float(np.float32(c))), abs=1e-6)
    assert [s for _, s in hits] == sorted((s for _, s in hits), reverse=True)


def test_layout_epoch_retry(world):
    hip, idx, q, cos = world
    searches = lambda: sum(c["fn"] == "search" for c in idx.calls)
    builds = lambda: sum(c["fn"] in ("rows", "tags") for c in idx.calls)
    idx.compact_during_next = 2                     # two searches see a compaction land under them, the third is clean
    s0, b0 = searches(), builds()
    assert ns(hip.semantic_search_within(q, k=3, patient_ids=["p1"])) == [1, 5, 9]
    assert searches() - s0 == 3 and builds() - b0 == 3          # the bitmap is rebuilt with every attempt
    idx.compact_during_next = 10 ** 6
    with pytest.raises(RuntimeError, match="compacted during every one"):
        hip.semantic_search_within(q, k=3, doc_ids=["d1"])
    assert searches() - s0 == 3 + indexer.LAYOUT_ATTEMPTS
    idx.compact_during_next = 0
    # a REAL compaction between building the bitmap and the search: rows renumber, the stale bitmap's answer is discarded
    # and the second attempt maps d9 / d30 through the new doc_id -> row table
    st = REGISTRY.get(hip.index_name, create=False)
    indexer.add_documents(hip.index_name, [{"doc_id": "d3", "patientId": "p3", "doc_type": "unstructured", "n": 300}],
                          np.eye(1, DIM, 1, dtype=np.float32))       # tombstones row 3
    idx.compact_for_real_before_next_search = st
    s0 = searches()
    assert ns(hip.semantic_search_within(q, k=5, doc_ids=["d9", "d30", "d3"])) == [9, 30, 300]
    assert searches() - s0 == 2 and idx.rows == 40 and idx.layout_epoch > 0
    assert [c for c in idx.calls if c["fn"] == "rows"][-1]["rows"] == [8, 29, 39]          # the rows after the compaction


def test_rows_appended_between_build_and_search(world):
    """An ingest lands after the bitmap was built and before the search (the layout epoch does not move on an append): 40
    chunks, across a 32-row boundary, all scoring above everything indexed.  The bitmap speaks for the rows it was built
    over: the call succeeds, without a retry, and none of the new rows is in the answer."""
    hip, idx, q, cos = world
    best = np.zeros((40, DIM), dtype=np.float32)
    best[:, 0] = 1.0
    late = [{"doc_id": f"late{i}", "patientId": "p1", "doc_type": "note", "n": 1000 + i} for i in range(40)]
    ingest = lambda: indexer.add_documents(hip.index_name, late, best)
    for kw, want in ((dict(patient_ids=["p1"]), [1, 5, 9]), (dict(doc_ids=["d9", "d30", "late3"]), [9, 30]),
                     (dict(patient_ids=["p1"], doc_types=["note"]), [5, 25])):
        REGISTRY.drop(hip.index_name)
        idx = StandInIndex()
        _fill(hip.index_name, idx)
        idx.before_next_search = ingest
        assert ns(hip.semantic_search_within(q, k=3, **kw)) == want
        assert idx.rows == 80 and sum(c["fn"] == "search" for c in idx.calls) == 1
        assert [c for c in idx.calls if c["fn"] == "search"][-1]["words"] == 2       # built over 40 rows, searched over 80
        # the next call sees them
        assert ns(hip.semantic_search_within(q, k=3, **kw))[0] >= 1000


class GrowingLib:
    """A native layer whose index has ``rows_seen_by_python`` rows when Python asks and ``rows_at_the_call`` when the search
    entry point checks ``words_per_bitmap``, as an append in between makes it."""

    def __init__(self, rows_seen_by_python, rows_at_the_call):
        self.py_rows, self.call_rows, self.calls = list(rows_seen_by_python), list(rows_at_the_call), []

    def rass_index_dim(self, h):
        return DIM

    def rass_index_rows(self, h):
        return self.py_rows.pop(0) if len(self.py_rows) > 1 else self.py_rows[0]

    def rass_index_search_allowed(self, h, q, nq, k, allow, n_bitmaps, words, f, m, out_s, out_i):
        rows = self.call_rows.pop(0) if len(self.call_rows) > 1 else self.call_rows[0]
        self.calls.append((n_bitmaps, words, rows))
        return 0 if words >= (rows + 31) // 32 else -1


def test_flat_index_extends_a_bitmap_the_index_has_outgrown():
    q = np.zeros((3, DIM), dtype=np.float32)
    slack = FlatIndex.ALLOW_SLACK_WORDS
    # built over 40 rows (2 words), searched over 100: extended with zero words to what 100 rows need, plus slack
    lib = GrowingLib([100], [100])
    FlatIndex(types.SimpleNamespace(_L=lib), "v", None).search_allowed(q, 5, np.ones(2, dtype=np.uint32))
    assert lib.calls == [(1, 4 + slack, 100)]
    lib = GrowingLib([100], [100])
    FlatIndex(types.SimpleNamespace(_L=lib), "v", None).search_allowed(q, 5, np.ones((3, 2), dtype=np.uint32))
    assert lib.calls == [(3, 4 + slack, 100)]
    # long enough: passed as it is
    lib = GrowingLib([64], [64])
    FlatIndex(types.SimpleNamespace(_L=lib), "v", None).search_allowed(q, 5, np.ones(2, dtype=np.uint32))
    assert lib.calls == [(1, 2, 64)]
    # rows land between Python's look and the native check, within the slack: one call
    lib = GrowingLib([100], [100 + 32 * slack])
    FlatIndex(types.SimpleNamespace(_L=lib), "v", None).search_allowed(q, 5, np.ones(2, dtype=np.uint32))
    assert len(lib.calls) == 1
    # ... beyond the slack: the refused call is repeated with a longer bitmap
    big = 100 + 32 * slack + 40
    lib = GrowingLib([100, big], [big])
    FlatIndex(types.SimpleNamespace(_L=lib), "v", None).search_allowed(q, 5, np.ones(2, dtype=np.uint32))
    assert [c[1] for c in lib.calls] == [4 + slack, (big + 31) // 32 + slack]


def test_an_index_without_the_method_says_so():
    class PlainIndex(StandInIndex):
        search_allowed = property()          # hasattr() is False

    name = "allow-cpu-plain"
    q, _ = _fill(name, PlainIndex())
    try:
        with pytest.raises(NotImplementedError, match="allow-list search"):
            indexer.HipIndexer(None, name).semantic_search_within(q, patient_ids=["p1"])
    finally:
        REGISTRY.drop(name)


def test_flat_index_search_allowed_validates_before_the_native_call():
    class Lib:
        def rass_index_dim(self, h):
            return DIM

        def rass_index_rows(self, h):
            return 128                          # 4 words

        def rass_index_search_allowed(self, *a):
            raise AssertionError("the native entry point was reached")

    idx = FlatIndex(types.SimpleNamespace(_L=Lib()), "v", None)
    q = np.zeros((3, DIM), dtype=np.float32)
    good = dict(queries=q, k=5, allow=np.zeros(4, dtype=np.uint32))
    bad = [dict(queries=np.zeros(DIM)), dict(queries=np.zeros((3, DIM + 1))), dict(k=0), dict(k=4097), dict(k=-3),
           dict(allow=np.zeros((2, 4), dtype=np.uint32)), dict(allow=np.zeros((3, 2, 2), dtype=np.uint32)),
           dict(queries=np.zeros((4097, DIM), dtype=np.float32)),
           dict(q_filter=np.zeros(2, dtype=np.int32)), dict(q_filter_mask=np.zeros(3, dtype=np.int32)),
           dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(4, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_allowed(**dict(good, **kw))
    for kw in (dict(), dict(k=1), dict(k=4096), dict(allow=np.zeros((3, 4), dtype=np.uint32)), dict(allow=np.zeros((1, 4), dtype=np.uint32)),
               dict(q_filter=np.zeros(3, dtype=np.int32), q_filter_mask=np.zeros(3, dtype=np.int32))):
        with pytest.raises(AssertionError, match="native entry point"):
            idx.search_allowed(**dict(good, **kw))
    s, i = idx.search_allowed(np.zeros((0, DIM), dtype=np.float32), 5, np.zeros(4, dtype=np.uint32))      # no query, no call
    assert s.shape == (0, 5) and i.shape == (0, 5)


# ---------------------------------------------------------------------------------------------- header / table / library
def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in _native.SIGNATURES, f"{name} is not in the binding table"
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), f"{name}: header and binding table disagree"
    assert os.path.exists(_native.LIB_PATH), "librass_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [name for name in NEW_ENTRY_POINTS if name not in exported]
    assert not missing, f"not exported by the built library: {missing}"
