"""Attribute columns and the predicate builder on the GPU, against numpy (``attr_ref``) and the CPU oracle.

* the builder ``rass_index_allow_from_attr_clauses`` word for word: both modes, 0 / 1 / 8 / 64 clauses per query, negation,
  the three combines over random prior words (one prior from ``allow_from_tag_values``), tails and surplus words pre-filled
  with ones, nq = 1, 5, 32, 33 (a second launch group of one) and the shared form;
* ``search_allowed`` behind a predicate bitmap against the oracle's ``KIND_F32_MFMA`` scores ranked by numpy over the matching
  rows (ids and scores EQUAL, as in test_gpu_allow_search.py);
* the columns through growth, compaction, save / load (and a truncated file), and an index without columns saving the bytes it
  always saved;
* the shim: ``add_documents`` with ``RASS_ATTR_FIELDS``, an overwrite, ``save_delta`` / load, and ``semantic_search_filtered``
  against ``semantic_search(k=300)`` filtered on the host by a plain Python evaluator.

Rows of dim 128 with n = 20 (less than a word), 1 000 (the last word has 8 bits) and 4 128 (129 tiles, grown past the first
capacity after columns were set), and n = 1 000 at dim 1024.  Columns 0, 3 and 7 are set with ~10 % missing, column 5 never;
values include INT32_MIN + 1 and INT32_MAX.  One world per shape, built once.  Integer and bit-exact throughout."""
import datetime as dt

import numpy as np
import pytest

import attr_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(20, 128), (1000, 128), (4128, 128), (1000, 1024)]
SET_COLS = (0, 3, 7)
NEVER_SET = 5
NQ = 33
SURPLUS = 3
NEG_INF = np.float32(-np.inf)
PATIENT_MASK = 0x00FFFFFF


class World:
    def __init__(self, torch, oracle, n, dim):
        from rassengine_amd import ops
        from rassengine_amd.engine import Engine
        rng = np.random.default_rng(9000 + n + dim)
        self.torch, self.oracle, self.n, self.dim, self.rng = torch, oracle, n, dim, rng
        self.xn = oracle.normalize_ref(rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
        self.q_raw = rng.standard_normal((NQ, dim), dtype=np.float32) * 3.0
        self.qn_gpu = ops.normalize_rows(torch.from_numpy(self.q_raw).cuda()).cpu().numpy()
        self.scores = oracle.scores(self.xn, self.qn_gpu, kind=oracle.KIND_F32_MFMA).astype(np.float32)
        self.tags = rng.integers(0, 6, size=n).astype(np.int32)
        self.cols = {}
        for c in SET_COLS:
            v = rng.integers(0, 40, size=n).astype(np.int64)
            v[rng.random(n) < 0.1] = R.MISSING
            v[rng.integers(0, n, size=2)] = R.INT_MIN
            v[rng.integers(0, n, size=2)] = R.INT_MAX
            self.cols[c] = v.astype(np.int32)
        self.eng = Engine(0, dim)
        self.idx = self.eng.open_index("attr")
        assert self.idx.attr_mask == 0
        first = min(n, 1000)                 # the first append sizes the index for 1 024 rows; the second outgrows that
        self.idx.add(self.xn[:first], tags=self.tags[:first], normalize=False)
        assert np.array_equal(self.idx.get_attr(0, 0, first), np.full(first, R.MISSING))      # never set: all missing
        for c in SET_COLS:
            self.idx.set_attr(c, 0, self.cols[c][:first])
        if n > first:
            self.idx.add(self.xn[first:], tags=self.tags[first:], normalize=False)
            for c in SET_COLS:            # appended rows read missing until they are set
                assert np.array_equal(self.idx.get_attr(c, first, n - first), np.full(n - first, R.MISSING))
                self.idx.set_attr(c, first, self.cols[c][first:])
        self.dead = sorted({3, n - 1} if n < 100 else set(rng.choice(n, size=n // 25, replace=False).tolist()) | {31, 32, n - 1})
        for r in self.dead:
            self.idx.delete(int(r))
        self.tags[self.dead] = -1
        self.words = (n + 31) // 32 + SURPLUS

    def random_clauses(self, nq, per_query, seed, negate_share=0.25):
        rng = np.random.default_rng(seed)
        out = []
        for q in range(nq):
            for _ in range(per_query):
                col = int(rng.choice((0, 3, 7, 7, NEVER_SET)))
                lo, hi = sorted(int(x) for x in rng.choice((R.INT_MIN, 0, 5, 12, 20, 33, 39, R.INT_MAX), size=2))
                if rng.random() < 0.15:
                    lo, hi = hi + 1 if hi < R.INT_MAX else hi, lo            # mostly lo > hi: holds for nothing
                if rng.random() < 0.2:
                    hi = lo                                                   # equality
                out.append((q, col, lo, hi, int(rng.random() < negate_share)))
        rng.shuffle(out)                                                      # any order: the host sorts by column
        return np.array(out, dtype=np.int64).reshape(-1, 5)

    def build(self, clauses, nq, shared, mode, combine, prior):
        """The builder over a copy of ``prior`` (uint32 [n_bitmaps, words]) -> the words it left."""
        torch = self.torch
        t = torch.from_numpy(prior.view(np.int32).copy()).cuda()
        t = t[0].contiguous() if shared else t
        got = self.idx.allow_from_attr_clauses(clauses, nq=nq, shared=shared, mode=mode, combine=combine, allow=t)
        assert got is t
        self.eng.synchronize()
        return t.cpu().numpy().view(np.uint32).reshape(prior.shape)

    def check_build(self, clauses, nq, shared, mode, combine, prior, what, bits=None):
        nb = 1 if shared else nq
        got = self.build(clauses, nq, shared, mode, combine, prior)
        want = R.build(self.cols, self.tags, clauses, nq, nb, {"all": R.ALL, "any": R.ANY}[mode],
                       {"replace": R.REPLACE, "and": R.AND, "or": R.OR}[combine], prior, bits=bits)
        assert np.array_equal(got, want), (what, self.n, self.dim, nq, shared, mode, combine, np.argwhere(got != want)[:5])
        return got

    def priors(self, nb, seed):
        rng = np.random.default_rng(seed)
        return {"ones": np.full((nb, self.words), 0xFFFFFFFF, dtype=np.uint32),            # tails and surplus words pre-filled
                "random": rng.integers(0, 2 ** 32, size=(nb, self.words), dtype=np.uint64).astype(np.uint32)}


@pytest.fixture(scope="module")
def worlds(gpu, oracle):
    made = {}

    def get(n, dim):
        if (n, dim) not in made:
            made[(n, dim)] = World(gpu, oracle, n, dim)
        return made[(n, dim)]

    yield get
    for w in made.values():
        w.eng.close()


# ------------------------------------------------------------------------------------------------ builder == numpy
@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("mode", ["all", "any"])
def test_builder_equals_numpy_word_for_word(worlds, n, dim, mode):
    w = worlds(n, dim)
    for nq, shared in ((1, False), (5, False), (32, False), (33, False), (33, True)):
        nb = 1 if shared else nq
        for per_query in (0, 1, 8, 64):
            clauses = w.random_clauses(nb, per_query, seed=nq * 100 + per_query)
            bits = R.allowed(w.cols, w.tags, clauses, nb, {"all": R.ALL, "any": R.ANY}[mode])     # numpy, once per clause set
            for combine in ("replace", "and", "or"):
                for name, prior in w.priors(nb, seed=per_query + nq).items():
                    got = w.check_build(clauses, nq, shared, mode, combine, prior, f"{per_query} clauses, prior {name}", bits)
                    if combine != "or":     # bits at or past the row count and the surplus words come out 0
                        assert not R.unpack(got, w.words * 32)[:, n:].any()
                    elif name == "ones":    # ... and stay as they were under OR
                        assert R.unpack(got, w.words * 32)[:, n:].all()


@pytest.mark.parametrize("n,dim", SHAPES)
def test_builder_refines_a_tag_value_bitmap_and_composes(worlds, n, dim):
    w = worlds(n, dim)
    values = np.array([1, 4], dtype=np.int32)
    d_tags = w.idx.allow_from_tag_values(values, PATIENT_MASK)
    prior = d_tags.cpu().numpy().view(np.uint32)[None, :w.words].copy()
    assert np.array_equal(R.unpack(prior, n)[0], np.isin(w.tags, values))                    # tombstones are -1: excluded
    a = np.array([(0, 0, 5, 30, 0), (0, 3, 0, 20, 1)], dtype=np.int64)
    b = np.array([(0, 7, 12, 12, 0), (0, NEVER_SET, R.INT_MIN, R.INT_MAX, 0)], dtype=np.int64)
    both = w.check_build(a, 1, True, "all", "and", prior, "tag values, then AND")
    final = w.check_build(b, 1, True, "any", "or", both, "then OR")
    want = (np.isin(w.tags, values) & R.allowed(w.cols, w.tags, a, 1, R.ALL)[0]) | R.allowed(w.cols, w.tags, b, 1, R.ANY)[0]
    assert np.array_equal(R.unpack(final, n)[0], want)
    # the word-wise merge of two bitmaps
    torch = w.torch
    x = w.priors(2, seed=n)["random"]
    for op, fn in (("and", lambda p, q: p & q), ("or", lambda p, q: p | q), ("andnot", lambda p, q: p & ~q)):
        d0, d1 = torch.from_numpy(x[0].view(np.int32).copy()).cuda(), torch.from_numpy(x[1].view(np.int32).copy()).cuda()
        assert w.idx.allow_combine(d0, d1, op) is d0
        w.eng.synchronize()
        assert np.array_equal(d0.cpu().numpy().view(np.uint32), fn(x[0], x[1])) and np.array_equal(d1.cpu().numpy().view(np.uint32), x[1])


def test_builder_refuses_what_is_out_of_bounds(worlds):
    from rassengine_amd import _native as N
    w = worlds(1000, 128)
    torch = w.torch
    t = torch.zeros((2, w.words), dtype=torch.int32, device="cuda")

    def refused(clauses, nq=2, shared=False, allow=t, **kw):
        with pytest.raises(N.RassError) as e:
            w.idx.allow_from_attr_clauses(np.array(clauses, dtype=np.int64).reshape(-1, 5), nq=nq, shared=shared, allow=allow, **kw)
        assert e.value.code == -1 and str(e.value)                  # RASS_ERR_INVALID with a reason
    ok = [(1, 0, 0, 5, 0)] * 64
    w.idx.allow_from_attr_clauses(np.array(ok, dtype=np.int64), nq=2, allow=t)
    refused(ok + [(1, 3, 0, 5, 0)])                                 # a 65th clause for query 1
    refused([(2, 0, 0, 5, 0)])                                      # a query outside [0, nq)
    refused([(-1, 0, 0, 5, 0)])
    refused([(0, 8, 0, 5, 0)])                                      # a column outside 0 .. 7
    refused([(0, -1, 0, 5, 0)])
    refused([(1, 0, 0, 5, 0)], nq=2, shared=True, allow=t[0].contiguous())     # a shared bitmap's clauses name query 0
    refused([(0, 0, 0, 5, 0)], nq=1, allow=torch.zeros((1, (1000 + 31) // 32 - 1), dtype=torch.int32, device="cuda"))   # too few words
    refused([], nq=4097, shared=True, allow=t[0].contiguous())
    for col, first, vals in ((8, 0, [1]), (-1, 0, [1]), (0, 999, [1, 2]), (0, -1, [1]), (0, 1001, [])):
        with pytest.raises(N.RassError) as e:
            w.idx.set_attr(col, first, np.array(vals, dtype=np.int32))
        assert e.value.code == -1
    with pytest.raises(N.RassError):
        w.idx.get_attr(0, 990, 11)
    with pytest.raises(OverflowError):
        w.idx.set_attr(0, 0, np.array([2 ** 31], dtype=np.int64))
    assert np.array_equal(w.idx.get_attr(0, 0, 1000), w.cols[0])    # nothing of that was stored


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("k", [10, 100])
def test_search_behind_a_predicate_equals_the_oracle(worlds, n, dim, k):
    w = worlds(n, dim)
    nq = NQ
    # query q: column 0 within [0, q / 4 - 1] and column 7 present — from no match (q < 4: lo > hi) over a few (fewer than k:
    # padding) to a fifth of the rows
    clauses = np.array([(q, 0, 0, q // 4 - 1, 0) for q in range(nq)] + [(q, 7, R.INT_MIN, R.INT_MAX, 0) for q in range(nq)], dtype=np.int64)
    allow = w.idx.allow_from_attr_clauses(clauses, nq=nq)
    assert tuple(allow.shape) == (nq, w.idx.allow_words + w.idx.ALLOW_SLACK_WORDS)
    bits = R.allowed(w.cols, w.tags, clauses, nq, R.ALL)
    assert np.array_equal(R.unpack(allow.cpu().numpy().view(np.uint32), n), bits)
    counts = bits.sum(axis=1)
    if n >= 1000:
        assert counts.min() < 10 <= k and counts.max() > 100            # both sides of k
    es = np.full((nq, k), NEG_INF, dtype=np.float32)
    ei = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        rows = np.flatnonzero(bits[q])
        order = np.lexsort((rows, -w.scores[q, rows]))[:k]
        es[q, :len(order)], ei[q, :len(order)] = w.scores[q, rows[order]], rows[order]
    s, i = w.idx.search_allowed(w.q_raw, k, allow)
    assert np.array_equal(i, ei) and np.array_equal(s, es), (n, dim, k, np.argwhere(i != ei)[:5])
    # one shared predicate for every query
    shared = w.idx.allow_from_attr_clauses(np.array([(0, 3, 10, 39, 1)], dtype=np.int64), nq=nq, shared=True)
    assert shared.dim() == 1
    sb = R.allowed(w.cols, w.tags, [(0, 3, 10, 39, 1)], 1, R.ALL)[0]
    s, i = w.idx.search_allowed(w.q_raw, k, shared)
    for q in range(nq):
        rows = np.flatnonzero(sb)
        order = np.lexsort((rows, -w.scores[q, rows]))[:k]
        assert np.array_equal(i[q, :len(order)], rows[order]) and np.array_equal(s[q, :len(order)], w.scores[q, rows[order]])
        assert np.all(i[q, len(order):] == -1)


# ------------------------------------------------------------------------------------------------ row movement
def test_columns_survive_growth_and_read_back(worlds):
    w = worlds(4128, 128)
    assert w.idx.attr_mask == (1 << 0) | (1 << 3) | (1 << 7)
    for c in SET_COLS:
        assert np.array_equal(w.idx.get_attr(c, 0, w.n), w.cols[c]), c       # set before and after the growth
        assert w.idx.device_attr_ptr(c) != 0
    assert np.array_equal(w.idx.get_attr(NEVER_SET, 0, w.n), np.full(w.n, R.MISSING)) and w.idx.device_attr_ptr(NEVER_SET) == 0
    assert np.array_equal(w.idx.get_attr(3, 31, 2), w.cols[3][31:33])        # delete leaves the values alone


def _small_index(eng, name, n=300, dim=128, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    idx = eng.open_index(name)
    idx.add(x, tags=rng.integers(0, 4, size=n).astype(np.int32))
    return idx, rng


def test_compaction_carries_the_columns(gpu):
    from rassengine_amd.engine import Engine
    eng = Engine(0, 128)
    try:
        idx, rng = _small_index(eng, "attr-compact")
        n = idx.rows
        cols = {c: rng.integers(-50, 50, size=n).astype(np.int32) for c in (1, 6)}
        cols[6][rng.random(n) < 0.2] = R.MISSING
        for c, v in cols.items():
            idx.set_attr(c, 0, v)
        dead = sorted(set(rng.choice(n, size=60, replace=False).tolist()) | {0, 31, 32, n - 1})
        for r in dead:
            idx.delete(r)
        clauses = np.array([(0, 1, -10, 30, 0), (0, 6, 0, 49, 1)], dtype=np.int64)
        before = R.unpack(idx.allow_from_attr_clauses(clauses, shared=True).cpu().numpy().view(np.uint32)[None], n)[0]
        new_row = idx.compact()
        live = np.flatnonzero(new_row >= 0)
        assert idx.rows == len(live) == n - len(dead) and idx.attr_mask == (1 << 1) | (1 << 6)
        for c, v in cols.items():
            assert np.array_equal(idx.get_attr(c, 0, idx.rows), v[live]), c            # the columns follow new_row
        after = R.unpack(idx.allow_from_attr_clauses(clauses, shared=True).cpu().numpy().view(np.uint32)[None], idx.rows)[0]
        assert np.array_equal(after, before[live]) and before[dead].sum() == 0          # the same docs as before
        first = idx.add(rng.standard_normal((5, 128), dtype=np.float32))                # rows appended afterwards read missing
        assert np.array_equal(idx.get_attr(1, first, 5), np.full(5, R.MISSING))
    finally:
        eng.close()


def test_save_load_round_trip_and_file_format(gpu, tmp_path):
    from rassengine_amd import _native as N
    from rassengine_amd.engine import Engine
    eng = Engine(0, 128)
    try:
        idx, rng = _small_index(eng, "attr-save")
        n = idx.rows
        plain = str(tmp_path / "plain.rass")
        idx.save(plain)                                             # no column: today's bytes
        plain_bytes = open(plain, "rb").read()
        assert len(plain_bytes) == 40 + n * (128 * 4 + 4) and plain_bytes[20:24] == b"\x00\x00\x00\x00"   # header.reserved
        cols = {c: rng.integers(R.INT_MIN, R.INT_MAX, size=n, dtype=np.int64).astype(np.int32) for c in (0, 2, 7)}
        cols[2][::3] = R.MISSING
        for c, v in cols.items():
            idx.set_attr(c, 0, v)
        idx.delete(17)
        typed = str(tmp_path / "typed.rass")
        idx.save(typed)
        raw = open(typed, "rb").read()
        assert raw[20:24] == b"\x02\x00\x00\x00" and len(raw) == len(plain_bytes) + 4 + 3 * (4 + 4 * n)
        tail = np.frombuffer(raw[len(plain_bytes):], dtype=np.int32)
        assert tail[0] == 3 and [int(tail[1 + j * (n + 1)]) for j in range(3)] == [0, 2, 7]
        assert np.array_equal(tail[2:2 + n], cols[0])
        back = eng.load_index("attr-save-back", typed)
        assert back.rows == n and back.count == n - 1 and back.attr_mask == 0b10000101
        for c in range(8):                                          # every column, the never-set ones included
            assert np.array_equal(back.get_attr(c, 0, n), cols.get(c, np.full(n, R.MISSING))), c
        assert np.array_equal(back.get_rows(0, n), idx.get_rows(0, n))
        old = eng.load_index("attr-save-plain", plain)              # a file without the section still loads
        assert old.rows == n and old.attr_mask == 0
        again = str(tmp_path / "again.rass")
        old.save(again)
        assert open(again, "rb").read() == plain_bytes              # ... and saves the same bytes
        # a truncated attribute section: RASS_ERR_IO, and the name is free again
        for cut in (len(raw) - 4, len(plain_bytes) + 2, len(plain_bytes) + 4 + 4 * n):
            short = str(tmp_path / "short.rass")
            open(short, "wb").write(raw[:cut])
            with pytest.raises(N.RassError) as e:
                eng.load_index("attr-short", short)
            assert e.value.code == -6
        ok = eng.load_index("attr-short", typed)
        assert ok.rows == n
    finally:
        eng.close()


def test_bf16_and_synthetic_rows_take_columns(gpu):
    from rassengine_amd.engine import Engine
    eng = Engine(0, 256)
    try:
        idx = eng.open_index("attr-bf16", dtype="bf16")
        idx.fill_synthetic(100, seed=1)
        idx.set_attr(4, 10, np.arange(50, dtype=np.int32))
        idx.fill_synthetic(2000, seed=2)                            # grows; the filled rows read missing
        want = np.full(2100, R.MISSING, dtype=np.int32)
        want[10:60] = np.arange(50)
        assert np.array_equal(idx.get_attr(4, 0, 2100), want)
        t = idx.allow_from_attr_clauses(np.array([(0, 4, 0, 9, 0)], dtype=np.int64), shared=True)
        assert np.array_equal(np.flatnonzero(R.unpack(t.cpu().numpy().view(np.uint32)[None], 2100)[0]), np.arange(10, 20))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the shim
NOW = dt.datetime(2024, 2, 29, 15, 30, tzinfo=dt.timezone.utc)
KINDS = {"resourceType": "keyword", "chunkDate": "date", "pages": "int", "patientId": "keyword", "doc_type": "keyword"}
WHERES = [
    {"term": {"resourceType": "Observation"}},
    {"bool": {"must": [{"range": {"chunkDate": {"gte": "now-1y", "lt": "now"}}}, {"terms": {"resourceType": ["Condition", "Encounter", "Nope"]}}],
              "must_not": {"range": {"pages": {"gt": 20}}}}},
    {"bool": {"should": [{"term": {"patientId": "p2"}}, {"bool": {"must": [{"exists": {"field": "pages"}}, {"term": {"doc_type": "note"}}]}}],
              "must_not": [{"term": {"resourceType": "Procedure"}}]}},
    {"bool": {"must_not": [{"exists": {"field": "chunkDate"}}, {"term": {"patientId": "p0"}}]}},
    {"bool": {"filter": [{"bool": {"should": [{"range": {"pages": {"lte": 3}}}, {"range": {"pages": {"gte": 30}}}]}},
                         {"bool": {"should": [{"term": {"resourceType": "Observation"}}, {"range": {"chunkDate": {"lte": "2022-12-31"}}}]}}]}},
    {"term": {"resourceType": "NeverIndexed"}},
]


def _corpus(rng, n=300):
    types = ["Observation", "Condition", "Encounter", "Procedure"]
    docs = []
    for i in range(n):
        d = {"doc_id": f"d{i}", "doc_type": "note" if i % 5 == 0 else "unstructured", "patientId": f"p{i % 4}"}
        if rng.random() < 0.9:
            d["resourceType"] = types[int(rng.integers(4))]
        if rng.random() < 0.85:
            stamp = dt.datetime(2022, 6, 1, tzinfo=dt.timezone.utc) + dt.timedelta(hours=int(rng.integers(0, 24 * 700)))
            d["chunkDate"] = [stamp.date().isoformat(), int(stamp.timestamp() * 1000), stamp.isoformat()][int(rng.integers(3))]
        if rng.random() < 0.9:
            d["pages"] = int(rng.integers(0, 40))
        docs.append(d)
    return docs


def test_shim_filtered_search_equals_host_filtering(gpu, tmp_path, monkeypatch):
    from rassengine_amd import config, indexer
    from rassengine_amd.docstore import REGISTRY, IndexState
    from rassengine_amd.engine import Engine
    monkeypatch.setattr(config, "RASS_ATTR_FIELDS", "resourceType:keyword,chunkDate:date,pages:int")
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "cosine")
    eng = Engine(0, 128)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: eng.open_index(name))
    try:
        rng = np.random.default_rng(17)
        name, prefix = "rass-idx-attr", str(tmp_path / "attr")
        docs = _corpus(rng)
        emb = rng.standard_normal((300, 128), dtype=np.float32)
        indexer.add_documents(name, docs[:200], emb[:200])
        st = REGISTRY.get(name)
        st.attrs.clock = lambda: NOW
        st.save(prefix)
        # the rest, and 20 docs overwritten with other field values
        over = [dict(docs[i], resourceType="Encounter", pages=int(i % 40), chunkDate="2023-09-09") for i in range(40, 60)]
        for d in over:
            docs[int(d["doc_id"][1:])] = d
        indexer.add_documents(name, docs[200:] + over, np.concatenate([emb[200:], emb[40:60]]))
        assert st.index.rows == 320 and st.index.count == 300 and st.index.attr_mask == 0b111
        assert st.save_delta(prefix)
        st2 = IndexState.load("rass-idx-attr-restored", prefix, eng.load_index)
        st2.attrs.clock = lambda: NOW
        REGISTRY.put(st2)
        assert st2.attrs == st.attrs and st2.attrs.to_meta() == st.attrs.to_meta() and st2.index.attr_mask == 0b111
        for c in range(3):
            assert np.array_equal(st2.index.get_attr(c, 0, 320), st.index.get_attr(c, 0, 320)), c
        want_cols = st.attrs.encode_docs([st.row_doc[r] for r in range(320)])
        live = np.array([d is not None for d in st.row_doc])
        assert np.array_equal(np.stack([st.index.get_attr(c, 0, 320) for c in range(3)])[:, live], want_cols[:, live])
        q = rng.standard_normal(128).astype(np.float32)
        for index_name in (name, "rass-idx-attr-restored"):
            hip = indexer.HipIndexer(None, index_name)
            everything = hip.semantic_search(q, k=300)
            assert len(everything) == 300
            for where in WHERES:
                want = [(d["doc_id"], s) for d, s in everything if R.doc_matches(where, d, KINDS, NOW)]
                for k in (10, 300):
                    got = [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=k, where=where)]
                    assert got == want[:k], (index_name, where, k)
            assert WHERES[-1] and hip.semantic_search_filtered(q, k=5, where=WHERES[-1]) == []
            # with a patient filter next to it, and where=None
            got = [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=300, where=WHERES[0], patient_id="p1")]
            assert got == [(d["doc_id"], s) for d, s in everything if d["patientId"] == "p1" and d.get("resourceType") == "Observation"]
            assert hip.semantic_search_filtered(q, k=7) == hip.semantic_search(q, k=7)
            assert hip.semantic_search_filtered(np.zeros(0, dtype=np.float32), where=WHERES[0]) == []
            for bad in ({"term": {"color": "red"}}, {"match": {"resourceType": "Observation"}}, {"range": {"resourceType": {"gte": "a"}}}):
                with pytest.raises(ValueError):
                    hip.semantic_search_filtered(q, k=5, where=bad)

        class NoAllow:
            rows = count = 0
        REGISTRY.put(IndexState("rass-idx-attr-ivf", NoAllow()))
        with pytest.raises(NotImplementedError):
            indexer.HipIndexer(None, "rass-idx-attr-ivf").semantic_search_filtered(q, k=5, where=WHERES[0])
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()
