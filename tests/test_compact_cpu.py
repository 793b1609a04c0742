"""Compaction above the kernel, without a GPU: the ABI surface, ``IndexState.compact`` and the readers that hold row
ordinals (``HipIndexer``, the k-NN prefetch), the ``RASS_COMPACT_*`` policy.  The index is the oracle-backed test double
with the two members a compacting index adds (``compact`` / ``layout_epoch``)."""
import asyncio
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import OracleIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rass_index_compact", "rass_index_layout_epoch", "rass_compact_plan", "rass_compact_plan_workspace_bytes",
               "rass_compact_rows_f32")
DIM = 64


class CompactingOracleIndex(OracleIndex):
    """``OracleIndex`` + what ``engine.FlatIndex`` offers for compaction.  ``before_search_returns``: a hook called with the
    index after a search computed its answer and before it returns it (a compaction landing between a search and the
    caller's use of its ids)."""

    def __init__(self, dim=DIM):
        super().__init__(dim)
        self.layout_epoch = 0
        self.compactions = 0
        self.searches = 0
        self.before_search_returns = None

    def compact(self):
        live = self._tags != -1
        new_row = np.where(live, np.cumsum(live) - live, -1).astype(np.int64)
        self.compactions += 1
        if live.all():
            return new_row
        self._rows, self._tags = self._rows[live], self._tags[live]
        self.layout_epoch += 1
        return new_row

    def search(self, queries, k, q_filter=None, q_filter_mask=None):
        self.searches += 1
        out = super().search(queries, k, q_filter, q_filter_mask)
        hook, self.before_search_returns = self.before_search_returns, None
        if hook is not None:
            hook(self)
        return out

    def save(self, path):
        np.savez(path + ".npz", rows=self._rows, tags=self._tags)
        os.replace(path + ".npz", path)

    @classmethod
    def load(cls, name, path):
        z = np.load(path)
        idx = cls(int(z["rows"].shape[1]))
        idx._rows, idx._tags = z["rows"], z["tags"]
        return idx


# ------------------------------------------------------------------------------------------------ the ABI surface
def test_header_library_and_binding_carry_the_new_entry_points():
    from rassengine_amd import _native as N
    header = open(os.path.join(ROOT, "include", "rass_engine.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(rass_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    exported = set(re.findall(r" T (rass_[a-z0-9_]+)", subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], check=True,
                                                                      capture_output=True, text=True).stdout))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in N.SIGNATURES, name
    assert callable(getattr(N.lib(), "rass_index_compact"))


def test_null_index_is_refused_with_a_message():
    from rassengine_amd import _native as N
    L = N.lib()
    before, after = ctypes.c_int64(-5), ctypes.c_int64(-5)
    assert L.rass_index_compact(None, None, 0, ctypes.byref(before), ctypes.byref(after)) == -1      # RASS_ERR_INVALID
    assert b"NULL" in L.rass_last_error()
    assert L.rass_index_layout_epoch(None) == 0
    assert L.rass_compact_plan(None, 10, None, None, None, None, 0, None) == -1 and L.rass_last_error()
    assert L.rass_compact_rows_f32(None, None, 100, None, 1, 1, None) == -1 and L.rass_last_error()
    assert L.rass_compact_plan_workspace_bytes(0) > 0
    assert L.rass_compact_plan_workspace_bytes(70_000_000) >= 70_000_000 // 2048 * 8


def test_engine_surface():
    from rassengine_amd.engine import FlatIndex
    from rassengine_amd.ivf import IvfBackedIndex
    from rassengine_amd.serving import ShardedIndex
    assert callable(FlatIndex.compact) and isinstance(FlatIndex.layout_epoch, property) and isinstance(FlatIndex.epoch, property)
    assert IvfBackedIndex.compact is not FlatIndex.compact
    with pytest.raises(NotImplementedError, match="collective remap"):
        ShardedIndex.compact(object.__new__(ShardedIndex))


# ------------------------------------------------------------------------------------------------ the shim
@pytest.fixture
def world(monkeypatch):
    from rassengine_amd import config
    from rassengine_amd.docstore import REGISTRY
    monkeypatch.setattr(config, "RASS_KNN_PREFETCH", 0)
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "cosine")
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: CompactingOracleIndex(DIM))
    yield REGISTRY
    REGISTRY.set_index_factory(None)
    REGISTRY.clear()


def _docs(lo, hi, version=0):
    return [{"doc_id": f"d{i}", "patientId": f"p{i % 3}", "doc_type": "note" if i % 2 else "lab", "v": version, "i": i}
            for i in range(lo, hi)]


def _ingest(name, rng):
    """Adds, same-doc_id overwrites and in-batch duplicates; returns the vector every doc_id ends up with."""
    from rassengine_amd.indexer import add_documents
    vec = {}

    def put(docs):
        emb = rng.standard_normal((len(docs), DIM)).astype(np.float32)
        add_documents(name, docs, emb)
        for d, e in zip(docs, emb):
            vec[d["doc_id"]] = e
    put(_docs(0, 40))
    put(_docs(10, 25, version=1))                               # overwrites
    put(_docs(38, 44, version=2) + _docs(40, 42, version=3))    # overwrites + duplicates inside the batch (the last wins)
    put(_docs(0, 5, version=4))
    return vec


def _answers(name, queries, k=7):
    from rassengine_amd.indexer import HipIndexer
    ix = HipIndexer(None, name)
    out = []
    for q in queries:
        out.append([(d["doc_id"], d["v"], s) for d, s in ix.semantic_search(q, k=k)])
        out.append([(d["doc_id"], d["v"], s) for d, s in ix.semantic_search(q, k=k, patient_id="p1")])
        out.append([(d["doc_id"], d["v"], s) for d, s in ix.hybrid_search("text", q, k=k)])
        out.append([(d["doc_id"], d["v"], s) for d, s in ix.multi_intent_search("text", q, k=40)])
        out.append([(d["doc_id"], d["v"], s) for d, s in ix.knn_scores(q, k=k, doc_type="note")])
    return out


def test_index_state_compact_keeps_every_answer(world, tmp_path):
    from rassengine_amd.docstore import IndexState
    rng = np.random.default_rng(0)
    vec = _ingest("u", rng)
    st = world.get("u")
    queries = rng.standard_normal((4, DIM)).astype(np.float32)
    before = _answers("u", queries)
    assert any(before) and st.index.rows > st.index.count and None in st.row_doc
    prefix = str(tmp_path / "u")
    st.save(prefix)
    assert st.save_delta(prefix) is True

    rows_before, live = st.index.rows, st.index.count
    assert st.compact() == (rows_before, live)
    assert st.index.rows == st.index.count == live == len(st.row_doc) == len(vec)
    assert None not in st.row_doc
    assert sorted(st.doc_row) == sorted(vec)
    for doc_id, row in st.doc_row.items():
        assert st.row_doc[row]["doc_id"] == doc_id
        want = vec[doc_id] / (np.linalg.norm(vec[doc_id]) + 1e-9)
        assert np.allclose(st.index.get_row(row), want, atol=1e-6), doc_id
    assert _answers("u", queries) == before                      # the same docs with the same scores
    assert st.compact() == (live, live) and st.index.layout_epoch == 1   # nothing left to remove

    # the delta log speaks old ordinals: "take a snapshot" until the next save()
    assert st.save_delta(prefix) is False
    from rassengine_amd.indexer import add_documents
    add_documents("u", _docs(100, 103), rng.standard_normal((3, DIM)).astype(np.float32))
    assert st.save_delta(prefix) is False
    st.save(prefix)
    assert st.save_delta(prefix) is True
    back = IndexState.load("u", prefix, CompactingOracleIndex.load)
    assert back.row_doc == st.row_doc and back.doc_row == st.doc_row
    assert back.index.rows == st.index.rows == back.index.count
    assert np.array_equal(back.index._rows, st.index._rows)


def test_a_compaction_between_search_and_hits_makes_knn_search_again(world):
    from rassengine_amd.indexer import HipIndexer
    rng = np.random.default_rng(1)
    _ingest("u", rng)
    st = world.get("u")
    q = rng.standard_normal(DIM).astype(np.float32)
    ix = HipIndexer(None, "u")
    want = [(d["doc_id"], s) for d, s in ix.semantic_search(q, k=5)]
    stale_docs = [st.row_doc[r] for r in st.index.search(q[None], 5)[1][0]]
    st.index.before_search_returns = lambda index: st.compact()   # lands after the scan, before _hits maps the ids
    searches = st.index.searches
    got = [(d["doc_id"], s) for d, s in ix.semantic_search(q, k=5)]
    assert st.index.layout_epoch == 1 and st.index.searches == searches + 2      # searched again
    assert got == want
    # (without the epoch check the stale ordinals would have named other rows of the new layout)
    assert [d and d["doc_id"] for d in stale_docs] == [w[0] for w in want]
    assert [st.row_doc[r]["doc_id"] for r in st.index.search(q[None], 5)[1][0]] == [w[0] for w in want]


def test_async_search_pairs_the_batchers_ids_with_the_layout_epoch(world):
    from rassengine_amd.indexer import HipIndexer
    rng = np.random.default_rng(2)
    _ingest("u", rng)
    st = world.get("u")
    q = rng.standard_normal(DIM).astype(np.float32)
    ix = HipIndexer(None, "u")

    async def main():
        want = [(d["doc_id"], s) for d, s in await ix.asemantic_search(q, k=5)]
        st.index.before_search_returns = lambda index: st.compact()
        got = [(d["doc_id"], s) for d, s in await ix.asemantic_search(q, k=5)]
        await st.batcher.close()
        return want, got
    want, got = asyncio.run(main())
    assert want and got == want and st.index.layout_epoch == 1


# ------------------------------------------------------------------------------------------------ the policy
def _overwrite_rounds(name, rng, rounds):
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.indexer import add_documents
    seen = []
    for v in range(rounds):
        add_documents(name, _docs(0, 20, version=v), rng.standard_normal((20, DIM)).astype(np.float32))
        st = REGISTRY.get(name)
        seen.append((st.index.rows, st.index.count))
    return seen


def test_policy_is_off_by_default(world):
    from rassengine_amd import config
    assert config.RASS_COMPACT_FRACTION == 0 and config.RASS_COMPACT_MIN_ROWS == 65536
    seen = _overwrite_rounds("u", np.random.default_rng(3), 5)
    assert seen == [(20 * (v + 1), 20) for v in range(5)]        # rows only grow, as before
    assert world.get("u").index.compactions == 0


def test_policy_compacts_once_the_threshold_is_crossed(world, monkeypatch):
    from rassengine_amd import config
    monkeypatch.setattr(config, "RASS_COMPACT_FRACTION", 0.25)
    monkeypatch.setattr(config, "RASS_COMPACT_MIN_ROWS", 30)
    seen = _overwrite_rounds("u", np.random.default_rng(4), 4)
    # round 0: 20 rows, nothing dead.  round 1: 40 rows, 20 dead > 0.25 * 40 and 40 >= 30 rows: compacted back to 20 ...
    assert seen == [(20, 20)] * 4
    st = world.get("u")
    assert st.index.layout_epoch == 3 and None not in st.row_doc and len(st.row_doc) == 20
    assert all(st.row_doc[r]["v"] == 3 for r in st.doc_row.values())
    # below the minimum row count the policy leaves the index alone
    monkeypatch.setattr(config, "RASS_COMPACT_MIN_ROWS", 1000)
    assert _overwrite_rounds("w", np.random.default_rng(5), 3) == [(20, 20), (40, 20), (60, 20)]


def test_policy_skips_an_index_that_cannot_compact(world, monkeypatch):
    from rassengine_amd import config
    from rassengine_amd.serving import ShardedIndex
    monkeypatch.setattr(config, "RASS_COMPACT_FRACTION", 0.25)
    monkeypatch.setattr(config, "RASS_COMPACT_MIN_ROWS", 1)
    world.set_index_factory(lambda name: OracleIndex(DIM))        # no compact() at all
    assert _overwrite_rounds("plain", np.random.default_rng(6), 3) == [(20, 20), (40, 20), (60, 20)]

    class Refusing(OracleIndex):                                  # a compact() that is out of scope (the sharded front's)
        compact = ShardedIndex.compact
    world.set_index_factory(lambda name: Refusing(DIM))
    assert _overwrite_rounds("sharded", np.random.default_rng(7), 3) == [(20, 20), (40, 20), (60, 20)]
    assert None in world.get("sharded").row_doc


# ------------------------------------------------------------------------------------------------ the prefetch
def test_append_overwrite_compact_changes_the_index_epoch_and_a_parked_list_is_dropped(world, monkeypatch):
    """Rows and tombstones come back to the same two numbers through a compaction, with other rows behind the ordinals:
    only the layout epoch tells the two states apart."""
    from rassengine_amd import config, prefetch
    from rassengine_amd.indexer import HipIndexer, add_documents
    monkeypatch.setattr(config, "RASS_KNN_PREFETCH", 2)
    rng = np.random.default_rng(8)
    q = rng.standard_normal(DIM).astype(np.float32)

    def put(lo, hi, version=0):
        add_documents("u", _docs(lo, hi, version), rng.standard_normal((hi - lo, DIM)).astype(np.float32))

    async def main():
        prefetch.reset_stats()
        put(0, 30)
        st = world.get("u")
        put(30, 40)                 # append 10
        put(30, 40, version=1)      # overwrite 10
        assert (st.index.rows, st.index.count) == (50, 40)
        prefetch.remember(q)
        await prefetch.run(st)
        assert prefetch.stats["prefetched"] == 1
        before = prefetch.index_epoch(st.index)
        parked = prefetch.take(st, q[None], 5, -1, 0)
        assert parked is not None and prefetch.stats["answered"] == 1     # control: the unchanged index answers from it
        st.compact()                # 40 rows, none dead
        put(0, 10, version=2)       # overwrite 10 again: 10 rows appended, 10 tombstoned
        after = prefetch.index_epoch(st.index)
        assert (st.index.rows, st.index.count) == (50, 40) and before[:2] == after[:2] == (50, 10)
        assert before != after
        assert prefetch.take(st, q[None], 5, -1, 0) is None and prefetch.stats["stale"] == 1      # the parked list is not used
        got = [(d["doc_id"], d["v"]) for d, _ in HipIndexer(None, "u").semantic_search(q, k=5)]
        ids = st.index.search(q[None], 5)[1][0]
        assert got == [(st.row_doc[r]["doc_id"], st.row_doc[r]["v"]) for r in ids]
        if st.batcher is not None:
            await st.batcher.close()

    asyncio.run(main())
