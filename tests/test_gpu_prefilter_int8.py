"""Prefilter mode 2 (SURVEY §8f-4 "bf16 (or int8)"): int8 candidate scan + exact fp32 re-rank.

The candidate scan is integer work: its lists (scores AND rows) must equal the oracle's numpy restatement BIT FOR BIT.
The final result must be bit-identical to the flat fp32 path for every returned row; on these corpora the id lists
are identical too (recall 1.0 — the true top-k sits inside the int8 top-32)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def engine(gpu):
    from rassengine_amd.engine import Engine
    eng = Engine(device=0, dim=1024)
    yield eng
    eng.close()


def _cand(idx, q, qf=None):
    import torch
    s, r = idx.candidates_device(torch.from_numpy(np.ascontiguousarray(q)).cuda(), qf)
    return s.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("dim", [1024, 384, 512, 768, 1100, 1536, 2048])
def test_int8_candidates_equal_the_oracle_bit_for_bit(gpu, oracle, dim):
    from rassengine_amd.engine import Engine
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(100 + dim)
        n = 5000 + 37                                   # a ragged last tile and a ragged last 16-row block
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x[11] = 0.0                                     # a zero row (a blank chunk's embedding): scale 0, score 0
        x[12, 5] = 40.0                                 # an outlier component: a coarse scale for that row
        tags = rng.integers(0, 3, size=n).astype(np.int32)
        idx = eng.open_index("i8")
        idx.set_prefilter("int8")                       # before any row exists
        assert idx.prefilter_mode == "int8"
        idx.add(x[:3000], tags=tags[:3000])
        idx.add(x[3000:], tags=tags[3000:])             # growth + an append that re-quantises a partly filled block
        idx.delete(17)
        idx.delete(4999)
        tags[[17, 4999]] = -1
        xn = idx.get_rows(0, n)                         # the stored (normalised) rows: what the quantiser saw
        for nq in (1, 16, 17, 32):
            q = rng.standard_normal((nq, dim)).astype(np.float32)
            qn = oracle.normalize_c(q)
            qf = rng.integers(-1, 3, size=nq).astype(np.int32)
            for f in (None, qf):
                s_g, r_g = _cand(idx, q, f)
                s_o, r_o = oracle.candidates_i8(xn, qn, 32, tags=tags, qfilter=f)
                assert np.array_equal(r_g, r_o), (dim, nq, f is not None)
                assert np.array_equal(s_g.view(np.uint32), s_o.view(np.uint32)), (dim, nq)
    finally:
        eng.close()


def test_int8_prefilter_matches_flat_path(engine, oracle):
    rng = np.random.default_rng(8)
    idx = engine.open_index("pf8")
    idx.set_prefilter("int8")
    n = 0
    tags_all = []
    for c in (1, 40, 3000, 17, 9000):            # odd batch sizes: int8 slab + scales kept in sync on add + growth
        x = rng.standard_normal((c, 1024), dtype=np.float32)
        t = rng.integers(1, 4, size=c).astype(np.int32)
        idx.add(x, tags=t)
        tags_all.append(t)
        n += c
    tags = np.concatenate(tags_all)
    idx.delete(7)
    idx.delete(4000)
    q = rng.standard_normal((45, 1024), dtype=np.float32)
    qf = rng.integers(-1, 4, size=45).astype(np.int32)
    for k in (1, 5, 10, 16, 32):                 # k > 16 silently takes the exact flat scan
        s_p, i_p = idx.search(q, k, q_filter=qf)
        idx.set_prefilter(False)
        s_f, i_f = idx.search(q, k, q_filter=qf)
        idx.set_prefilter("int8")                # re-enabled on a populated index: quantises the existing rows
        assert np.array_equal(i_p, i_f), k
        assert np.array_equal(s_p, s_f), k       # exact re-rank = the flat kernel's fmaf order
    live = i_p[i_p >= 0]
    assert 7 not in live and 4000 not in live
    for r in range(45):
        if qf[r] >= 0:
            assert np.all(tags[i_p[r][i_p[r] >= 0]] == qf[r])
    # the two candidate copies are exclusive; switching rebuilds from the fp32 rows
    idx.set_prefilter("bf16")
    assert idx.prefilter_mode == "bf16"
    s_b, i_b = idx.search(q, 10, q_filter=qf)
    idx.set_prefilter("int8")
    s_8, i_8 = idx.search(q, 10, q_filter=qf)
    assert np.array_equal(i_b, i_8) and np.array_equal(s_b, s_8)


def test_int8_prefilter_small_and_padding(engine):
    rng = np.random.default_rng(9)
    idx = engine.open_index("pf8-small")
    x = rng.standard_normal((5, 1024), dtype=np.float32)
    idx.add(x)
    idx.set_prefilter("int8")
    s, i = idx.search(x[:2], 10)
    idx.set_prefilter(False)
    s2, i2 = idx.search(x[:2], 10)
    assert np.array_equal(i, i2) and np.array_equal(s, s2)
    assert np.all(i[:, 5:] == -1) and np.all(np.isneginf(s[:, 5:]))
    assert i[0, 0] == 0 and i[1, 0] == 1


def test_int8_near_duplicates_are_reranked_exactly(engine):
    """Rows closer together than the int8 resolution: the candidate scan cannot order them, the fp32 re-rank must."""
    rng = np.random.default_rng(10)
    base = rng.standard_normal((1, 1024)).astype(np.float32)
    x = np.repeat(base, 20, axis=0) + 1e-4 * rng.standard_normal((20, 1024)).astype(np.float32)
    x[11] = x[3]                                  # exact duplicate
    filler = rng.standard_normal((2000, 1024)).astype(np.float32)
    idx = engine.open_index("pf8-dup")
    idx.add(np.concatenate([filler, x]))
    q = base * 3.0
    for k in (12, 16):
        idx.set_prefilter("int8")
        s_p, i_p = idx.search(q, k)
        idx.set_prefilter(False)
        s_f, i_f = idx.search(q, k)
        assert np.array_equal(i_p, i_f) and np.array_equal(s_p, s_f), k


def test_int8_recall_on_a_large_clustered_corpus(engine, oracle):
    """200 k rows in 2 000 tight clusters (the hard case for a coarse candidate score: many near neighbours): recall@10
    of the int8 prefilter against the flat scan of the same index."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    centres = torch.randn((2000, 1024), generator=g, device="cuda")
    centres /= centres.norm(dim=1, keepdim=True)
    idx = engine.open_index("pf8-big", capacity_rows=200_000)
    for c0 in range(0, 200_000, 50_000):
        which = torch.randint(0, 2000, (50_000,), generator=g, device="cuda")
        rows = centres[which] + 0.02 * torch.randn((50_000, 1024), generator=g, device="cuda")
        idx.add(rows.cpu().numpy())
    q = (centres[:64] + 0.02 * torch.randn((64, 1024), generator=g, device="cuda")).cpu().numpy()
    s_f, i_f = idx.search(q, 10)
    idx.set_prefilter("int8")
    s_p, i_p = idx.search(q, 10)
    recall = np.mean([len(set(i_p[r]) & set(i_f[r])) / 10 for r in range(64)])
    assert recall >= 0.95, recall
    same = i_p == i_f
    assert np.array_equal(s_p[same], s_f[same])            # every returned row carries its exact fp32 score


def test_mode_validation(gpu):
    from rassengine_amd.engine import Engine
    from rassengine_amd._native import RassError
    eng = Engine(0, 1536)
    try:
        idx = eng.open_index("wide")
        with pytest.raises(RassError):
            idx.set_prefilter("bf16")               # wide rows: int8 candidates or the fp32 flat scan
        with pytest.raises(ValueError):
            idx.set_prefilter("fp4")
        idx.set_prefilter("int8")
        assert idx.prefilter_mode == "int8"
    finally:
        eng.close()


@pytest.mark.parametrize("dim", [1100, 1536, 1792, 2048])
def test_int8_prefilter_on_wide_rows_matches_the_flat_scan(gpu, dim):
    """1 024 < dim <= 2 048 (VERDICT r3 missing #6, for the candidate mode): int8 slab rows of 1 536 / 2 048 B, the re-rank
    walks a K slice in two halves in the wide flat kernel's order — ids and scores ≡ the exact wide scan, single calls of
    1 .. 45 queries and the batch call."""
    from rassengine_amd.engine import Engine
    torch = gpu
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        rng = np.random.default_rng(dim)
        idx = eng.open_index("pf8-wide")
        n = 7000 + 13
        x = rng.standard_normal((n, dim)).astype(np.float32)
        tags = rng.integers(1, 4, size=n).astype(np.int32)
        idx.add(x[:4000], tags=tags[:4000])
        idx.add(x[4000:], tags=tags[4000:])
        idx.delete(11)
        q = rng.standard_normal((45, dim)).astype(np.float32)
        qf = rng.integers(-1, 4, size=45).astype(np.int32)
        for k in (1, 10, 16):
            idx.set_prefilter("int8")
            a = idx.search(q, k, q_filter=qf)
            a1 = idx.search(q[:1], k)
            idx.set_prefilter(False)
            b = idx.search(q, k, q_filter=qf)
            b1 = idx.search(q[:1], k)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]), (dim, k)
            assert np.array_equal(a1[1], b1[1]) and np.array_equal(a1[0], b1[0]), (dim, k)
        qd = torch.from_numpy(np.concatenate([q, q, q])[:100]).cuda().contiguous()
        outs = []
        for mode in ("int8", False):
            idx.set_prefilter(mode)
            s = torch.empty((100, 10), dtype=torch.float32, device="cuda")
            i = torch.empty((100, 10), dtype=torch.int64, device="cuda")
            idx.search_device_batch(qd.data_ptr(), 100, 10, s.data_ptr(), i.data_ptr())
            torch.cuda.synchronize()
            outs.append((s.cpu().numpy(), i.cpu().numpy()))
        assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0]), dim
    finally:
        eng.close()


@pytest.mark.parametrize("dim", [100, 600, 800, 900])
def test_int8_prefilter_rerank_at_odd_narrow_strides_matches_the_flat_scan(gpu, dim):
    """The narrow re-rank at fp32 strides 128, 640 and 896 (1, 5 and 7 chunks per K slice; dims 100, 600 and 800 — 900 pads to
    1 024, the 8-chunk case, next to it), which no other test reaches: ids and scores ≡ the exact flat scan, bit for bit, for a
    filtered call, a single unfiltered query and the batch call.  Inputs built as in the wide-row test above with seed = dim,
    picked on the CPU with the oracle's int8 restatement (oracle.candidates_i8 against oracle.search on normalize_c rows, the
    tombstone applied, once with the filters and once with all six queries unfiltered, which covers the single-query and the
    batch call): every query's flat top-10 lies inside its int8 top-11 of the 32 candidates kept, so a mismatch here is the
    re-rank's, never a candidate miss."""
    from rassengine_amd.engine import Engine
    torch = gpu
    eng = Engine(0, dim)
    try:
        eng.set_stream(int(torch.cuda.current_stream().cuda_stream))
        rng = np.random.default_rng(dim)
        idx = eng.open_index("pf8-odd")
        n = 3000 + 13
        x = rng.standard_normal((n, dim)).astype(np.float32)
        tags = rng.integers(1, 4, size=n).astype(np.int32)
        idx.add(x[:2000], tags=tags[:2000])
        idx.add(x[2000:], tags=tags[2000:])
        idx.delete(11)
        q = rng.standard_normal((6, dim)).astype(np.float32)
        qf = rng.integers(-1, 4, size=6).astype(np.int32)
        assert idx.row_stride == {100: 128, 600: 640, 800: 896, 900: 1024}[dim]
        k = 10
        idx.set_prefilter("int8")
        a = idx.search(q, k, q_filter=qf)
        a1 = idx.search(q[:1], k)
        idx.set_prefilter(False)
        b = idx.search(q, k, q_filter=qf)
        b1 = idx.search(q[:1], k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]), dim
        assert np.array_equal(a1[1], b1[1]) and np.array_equal(a1[0], b1[0]), dim
        assert np.all(a1[1] >= 0)                       # ten real rows, not an empty answer on both sides
        qd = torch.from_numpy(q).cuda().contiguous()
        outs = []
        for mode in ("int8", False):
            idx.set_prefilter(mode)
            s = torch.empty((6, k), dtype=torch.float32, device="cuda")
            i = torch.empty((6, k), dtype=torch.int64, device="cuda")
            idx.search_device_batch(qd.data_ptr(), 6, k, s.data_ptr(), i.data_ptr())
            torch.cuda.synchronize()
            outs.append((s.cpu().numpy(), i.cpu().numpy()))
        assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0]), dim
    finally:
        eng.close()


def test_knn_prefetch_on_a_prefilter_index_shares_the_candidate_scan(gpu, monkeypatch):
    """RASS_PREFILTER + the k-NN prefetch: concurrent ask()-shaped requests on one index share ONE candidate-scan launch of
    depth 16 (a quarter of the bytes of the exact scan); the synchronous searches of k <= 16 answer from it with exactly what
    the inline (prefilter) search returns; filtered searches and k > 16 fall back to the inline scan."""
    import asyncio
    from rassengine_amd import config, embedding, indexer, prefetch
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    from tests.helpers import HashEmbedder
    monkeypatch.setattr(config, "RASS_PREFILTER", "int8")
    monkeypatch.setattr(config, "RASS_KNN_PREFETCH", 2)
    REGISTRY.clear()
    REGISTRY.set_index_factory(None)
    embedding.set_embedder(HashEmbedder(1024))
    name = "rass-idx-pf-prefetch"
    try:
        docs = [{"doc_id": f"n-{i}", "doc_type": "unstructured", "patientId": f"p{i % 3}",
                 "unstructuredText": f"note {i} topic{i % 13} drug{i % 7} ward{i % 5}"} for i in range(3000)]
        asyncio.run(indexer.store_fhir_docs_in_opensearch([], docs, None, name))
        st = REGISTRY.get(name)
        assert st.index.prefilter_mode == "int8"
        texts = [f"note {7 * i} topic{(7 * i) % 13} drug{(7 * i) % 7} ward{(7 * i) % 5}" for i in range(24)]

        async def ask(text, k, **kw):
            q = await embedding.embed_query(text)
            await indexer.ensure_index_exists(None, name)
            return indexer.HipIndexer(None, name).semantic_search(q, k=k, **kw)

        async def burst(k, **kw):
            return await asyncio.gather(*(ask(t, k, **kw) for t in texts))

        before = dict(prefetch.stats)
        got = asyncio.run(burst(5))
        assert prefetch.stats["answered"] - before.get("answered", 0) == len(texts)
        monkeypatch.setattr(config, "RASS_KNN_PREFETCH", 0)
        want = asyncio.run(burst(5))
        for a, b in zip(got, want):
            assert [d["doc_id"] for d, _ in a] == [d["doc_id"] for d, _ in b] and [s for _, s in a] == [s for _, s in b]
        st.index.set_prefilter(False)                           # and the exact index agrees on this corpus
        exact = asyncio.run(burst(5))
        st.index.set_prefilter("int8")
        assert [[d["doc_id"] for d, _ in a] for a in got] == [[d["doc_id"] for d, _ in a] for a in exact]
        monkeypatch.setattr(config, "RASS_KNN_PREFETCH", 2)
        a0 = prefetch.stats["answered"]
        filt = asyncio.run(burst(5, patient_id="p1"))           # filtered: inline (candidates are picked under the filter)
        deep = asyncio.run(burst(20))                           # k > 16: inline exact scan
        assert prefetch.stats["answered"] == a0
        assert all(d["patientId"] == "p1" for r in filt for d, _ in r) and all(len(r) == 20 for r in deep)
    finally:
        embedding.set_embedder(None)
        REGISTRY.clear()
        Engine.get(config.RASS_DEVICE, config.EMBED_DIM).drop_index(name)
