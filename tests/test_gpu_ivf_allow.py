"""The IVF probe within a row bitmap (``rass_ivf_search_allowed_delta``): filtered k-NN that stays in the IVF.

Pinned, with no tolerance anywhere but the coarse ranking's near-ties: (1) every list probed == ``FlatIndex.search_allowed`` on
the same bitmap, ids and scores; (2) a partial probe == ``FlatIndex.search_allowed`` on (bitmap AND rows of the probed lists
+ delta), with the probed lists from ``rass_ivf_probe_lists``, themselves checked against the oracle's coarse ranking;
(3) bits on tombstones, past the row count and in surplus words allow nothing; (4) the work list's compaction, seen through
the scanned rows; (5) the device entry point; (6) the boundary (``HipIndexer.semantic_search_filtered``) with and without
``RASS_IVF_ALLOW``; (7) the error statuses; (8) ``rass_index_allow_count``.

Two worlds, built once: A (dim 128, 6 043 rows, 16 lists: the nprobe <= 32 branch) and B (dim 1 024, 20 011 rows, 64 lists:
the threshold branch at nprobe 64).  Both: tombstones before the build, a list of exactly 32 rows, an EMPTY list (a centroid
no row is near), lists that end inside a tile, ~900 rows appended after the build (the delta) and tombstones on both sides."""
import numpy as np
import pytest

from tests.ivf_allow_ref import member_bits

pytestmark = pytest.mark.gpu

PM, DM = 0x00FFFFFF, 0x7F000000
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
KNQ = ((10, 40), (1, 1), (32, 17), (5, 32))


def _clustered(rng, n, centres, sigma=1.0):
    dim = centres.shape[1]
    lab = rng.integers(0, centres.shape[0], size=n)
    return (centres[lab] + sigma * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)).astype(np.float32)


def _tags(rng, n):
    return (rng.integers(1, 5, size=n) | (rng.integers(1, 3, size=n) << 24)).astype(np.int32)


class World:
    pass


def _build_world(name, dim, n0, nlist, n_centres, seed):
    import torch
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import IvfBackedIndex, IvfIndex, IvfPolicy, assign_rows, train_centroids
    w = World()
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_centres, dim)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x0, tags0 = _clustered(rng, n0, centres), _tags(rng, n0)
    w.eng = Engine(0, dim)
    w.idx = idx = IvfBackedIndex(w.eng.open_index(name), IvfPolicy.manual(nprobe=4))
    idx.add(x0, tags=tags0)
    dead = [3, 64, n0 - 12]
    for r in dead:
        idx.delete(r)                                      # tombstones BEFORE the build: never enter the slab
    covered = n0 // 32 * 32
    cent = train_centroids(idx, nlist, 0, 6, 0)
    far = -torch.from_numpy(centres.sum(axis=0)).to(cent.device)
    cent[nlist - 1] = far / far.norm()                     # a centroid no row is near: an EMPTY list
    assign = assign_rows(idx, cent).astype(np.int32)
    alive0 = np.ones(n0, dtype=bool)
    alive0[dead] = False
    assign[assign == nlist - 1] = 0                        # (the few rows of a badly served cluster that still preferred it)
    small = nlist - 2                                      # ... and a list of exactly 32 live rows: the others move to list 0
    mine = np.nonzero((assign[:covered] == small) & alive0[:covered])[0]
    if mine.size < 32:
        spare = np.nonzero((assign[:covered] == 0) & alive0[:covered])[0][:32 - mine.size]
        assign[spare] = small
        mine = np.nonzero((assign[:covered] == small) & alive0[:covered])[0]
    assign[mine[32:]] = 0
    idx._swap_ivf(lambda: IvfIndex.build(idx, nlist=nlist, centroids=cent, assign=assign, n_rows=covered))
    w.ivf = ivf = idx.ivf
    lens = ivf.lists_device(want_assign=False)[1].cpu().numpy()
    assert ivf.covered_rows == covered and lens[small] == 32 and lens[nlist - 1] == 0 and np.any(lens % 32 != 0)
    x1, tags1 = _clustered(rng, 900, centres), _tags(rng, 900)
    assert idx.add(x1, tags=tags1) == n0 and idx.covered == covered
    dead += [100, covered // 2 + 1, int(mine[0]), covered + 5, n0 + 5, n0 + 899]   # both sides of `covered`, after the build
    for r in dead[3:]:
        idx.delete(r)
    w.n, w.covered, w.nlist, w.dim, w.dead, w.small = n0 + 900, covered, nlist, dim, dead, small
    w.cent, w.assign = cent, assign
    w.tags = np.concatenate([tags0, tags1])
    w.tags[dead] = -1
    w.alive = w.tags != -1
    w.q = (centres[rng.integers(0, n_centres, size=40)] + 0.7 * rng.standard_normal((40, dim)).astype(np.float32) / np.sqrt(dim)
           ).astype(np.float32)
    w.q[5] = x1[17]                                        # a query that IS a delta row
    w.q[6] = x0[100]                                       # ... and one that is a tombstoned covered row
    # the bitmaps every test shares: per query at density 0.5 and 0.01, and one shared
    w.bits = {"half": rng.random((40, w.n)) < 0.5, "sparse": rng.random((40, w.n)) < 0.01, "shared": rng.random(w.n) < 0.3}
    assert idx.rows == w.n
    return w


@pytest.fixture(scope="module")
def world_a(gpu):
    w = _build_world("ivf-allow-a", 128, 6_043, 16, 40, 21)
    yield w
    w.eng.close()


@pytest.fixture(scope="module")
def world_b(gpu):
    w = _build_world("ivf-allow-b", 1024, 20_011, 64, 150, 22)
    yield w
    w.eng.close()


def _allow(bits, nq):
    from rassengine_amd.engine import pack_allow
    return pack_allow(bits if bits.ndim == 1 else bits[:nq])


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


def _every_list_probed_equals_flat(w):
    from rassengine_amd.engine import FlatIndex
    idx, ivf, q = w.idx, w.ivf, w.q
    for kind, bits in w.bits.items():
        for k, nq in KNQ:
            allow = _allow(bits, nq)
            want = FlatIndex.search_allowed(idx, q[:nq], k, allow)
            s, i, _ = ivf.search_allowed_delta(idx, q[:nq], k, w.nlist, allow)
            _same((s, i), want, (kind, k, nq))
            assert not set(i.reshape(-1).tolist()) & set(w.dead)
        # plain (exact-tag) and masked filters, per query
        allow = _allow(bits, 40)
        qf = np.array([(r % 4 + 1) | ((r % 2 + 1) << 24) for r in range(40)], dtype=np.int32)
        for f, m in ((qf, None), (np.array([r % 4 + 1 for r in range(40)], dtype=np.int32), np.full(40, PM, dtype=np.int32)),
                     (np.array([(r % 2 + 1) << 24 for r in range(40)], dtype=np.int32), np.full(40, DM, dtype=np.int32))):
            want = FlatIndex.search_allowed(idx, q, 10, allow, f, m)
            s, i, _ = ivf.search_allowed_delta(idx, q, 10, w.nlist, allow, f, m)
            _same((s, i), want, (kind, "filter", m is not None))
            assert np.any(i >= 0)
    # under a bitmap that allows it, the delta row finds itself and the tombstoned covered row stays gone
    allow = _allow(np.ones(w.n, dtype=bool), 40)
    s, i, _ = ivf.search_allowed_delta(idx, q[5:7], 3, w.nlist, allow)
    assert i[0, 0] == w.n - 900 + 17 and 100 not in i[1].tolist()


def test_every_list_probed_equals_flat_bit_for_bit_world_a(world_a):
    _every_list_probed_equals_flat(world_a)                # nprobe = nlist = 16: the coarse scan's lists


def test_every_list_probed_equals_flat_bit_for_bit_world_b(world_b):
    _every_list_probed_equals_flat(world_b)                # nprobe = nlist = 64: the threshold branch


def _check_probe_lists(w, oracle, lists, nprobe):
    """``probe_lists`` against the oracle's coarse ranking: the nprobe best lists, or on a near-tie at the boundary the next one."""
    cn = oracle.normalize_ref(w.cent.cpu().numpy()).astype(np.float32)
    qn = oracle.normalize_ref(w.q).astype(np.float32)
    order = np.argsort(-oracle.scores(cn, qn, kind=oracle.KIND_F64), axis=1, kind="stable")
    np_eff = min(nprobe, w.nlist)
    assert lists.shape == (40, nprobe) and lists.dtype == np.int64
    assert np.all(lists[:, np_eff:] == -1)
    for r in range(40):
        got = lists[r, :np_eff].tolist()
        assert len(set(got)) == np_eff and min(got) >= 0 and max(got) < w.nlist
        assert set(got) <= set(order[r, :np_eff + 1].tolist()), (r, got)
        assert len(set(got) - set(order[r, :np_eff].tolist())) <= 1


def _partial_probe(w, oracle):
    from rassengine_amd.engine import FlatIndex, pack_allow
    idx, ivf, q, k = w.idx, w.ivf, w.q, 10
    bits = w.bits["half"].copy()
    bits[7::8] = w.bits["sparse"][7::8] & (np.arange(w.n) % 5 == 0)    # every eighth query: 1 row in 500 leaves its probe short
    bits[7::8, w.covered:] = False                         # ... with nothing in the delta (which every probe scans)
    for nprobe in (1, 4):
        lists = ivf.probe_lists(q, nprobe)
        _check_probe_lists(w, oracle, lists, nprobe)
        member = np.stack([member_bits(w.assign, lists[r], w.covered, w.n) for r in range(40)])
        inside = (bits & member & w.alive[None, :]).sum(axis=1)
        assert np.count_nonzero(inside >= k) >= 10 and np.any(inside < k), inside    # before the GPU is asked: full and short answers
        want = FlatIndex.search_allowed(idx, q, k, pack_allow(bits & member))
        s, i, scanned = ivf.search_allowed_delta(idx, q, k, nprobe, pack_allow(bits))
        _same((s, i), want, nprobe)
        assert np.array_equal((i >= 0).sum(axis=1), np.minimum(inside, k))
        short = i[inside < k]
        assert np.all(short[:, -1] == -1) and np.all(np.isneginf(s[inside < k][:, -1]))
        assert scanned > 0
        # with per-query filters on top
        qf = np.array([r % 4 + 1 for r in range(40)], dtype=np.int32)
        m = np.full(40, PM, dtype=np.int32)
        want = FlatIndex.search_allowed(idx, q, k, pack_allow(bits & member), qf, m)
        s, i, _ = ivf.search_allowed_delta(idx, q, k, nprobe, pack_allow(bits), qf, m)
        _same((s, i), want, (nprobe, "masked"))
    # the delta is always scanned: a query that is an allowed delta row finds it at nprobe 1
    one = np.zeros(w.n, dtype=bool)
    one[w.n - 900 + 17] = True
    s, i, scanned = ivf.search_allowed_delta(idx, q[5:6], 1, 1, pack_allow(one))
    assert i[0, 0] == w.n - 900 + 17 and scanned <= 32


def test_partial_probe_equals_flat_within_bitmap_and_probed_rows_world_a(world_a, oracle):
    _partial_probe(world_a, oracle)
    lists = world_a.ivf.probe_lists(world_a.q, 32)         # deeper than nlist = 16: -1 past the end
    _check_probe_lists(world_a, oracle, lists, 32)
    assert np.array_equal(np.sort(lists[:, :16], axis=1), np.tile(np.arange(16), (40, 1)))


def test_partial_probe_equals_flat_within_bitmap_and_probed_rows_world_b(world_b, oracle):
    _partial_probe(world_b, oracle)


def test_bits_that_must_allow_nothing(world_a):
    from rassengine_amd.engine import FlatIndex
    w = world_a
    idx, ivf, q = w.idx, w.ivf, w.q
    words = idx.allow_words
    # every bit set: tombstoned rows, the last word's bits past the row count, and five surplus words
    ones = np.full((40, words + 5), 0xFFFFFFFF, dtype=np.uint32)
    s, i, scanned = ivf.search_allowed_delta(idx, q, 10, w.nlist, ones)
    _same((s, i), FlatIndex.search_allowed(idx, q, 10, ones), "all ones")
    _same((s, i), FlatIndex.search(idx, q, 10), "all ones == the unfiltered search")
    assert i.min() >= 0 and i.max() < w.n and not set(i.reshape(-1).tolist()) & set(w.dead)
    # only the bits that may allow nothing
    nothing = np.zeros((40, words + 5), dtype=np.uint32)
    for r in w.dead:
        nothing[:, r >> 5] |= np.uint32(1 << (r & 31))
    nothing[:, words - 1] |= np.uint32((0xFFFFFFFF << (w.n & 31)) & 0xFFFFFFFF) if w.n & 31 else np.uint32(0)
    nothing[:, words:] = 0xFFFFFFFF
    s, i, _ = ivf.search_allowed_delta(idx, q, 10, w.nlist, nothing)
    assert np.all(i == -1) and np.all(np.isneginf(s))
    # an all-zero bitmap: the empty answer, nothing kept in the probe and nothing planned in the delta
    for zero in (np.zeros((40, words), dtype=np.uint32), np.zeros(words, dtype=np.uint32)):
        s, i, scanned = ivf.search_allowed_delta(idx, q, 10, w.nlist, zero)
        assert np.all(i == -1) and np.all(np.isneginf(s)) and scanned == 0


def test_compaction_shows_in_the_scanned_rows(world_a, world_b):
    from rassengine_amd.engine import FlatIndex, pack_allow
    for w in (world_a, world_b):
        idx, ivf, q = w.idx, w.ivf, w.q
        lens = np.bincount(w.assign[:w.covered][np.isin(np.arange(w.covered), w.dead[:3], invert=True)], minlength=w.nlist)
        _, _, whole = ivf.search_delta(idx, q, 10, w.nlist)
        assert whole == 2 * (int(lens.sum()) + w.n - w.covered)            # 40 queries = 2 groups, each the whole slab + the delta
        for lst in (1, w.small):
            only = np.zeros(w.n, dtype=bool)
            only[:w.covered] = w.assign[:w.covered] == lst
            allow = pack_allow(only)                                        # one shared bitmap: the rows of ONE list
            s, i, scanned = ivf.search_allowed_delta(idx, q, 10, w.nlist, allow)
            _same((s, i), FlatIndex.search_allowed(idx, q, 10, allow), lst)
            assert 0 < scanned <= 2 * (-(-int(lens[lst]) // 32) * 32), (lst, scanned)
            assert scanned == 2 * int(lens[lst])                            # every tile of the list keeps a bit: exactly its rows
        # per-query bitmaps over the same list: the same items, their masks narrowed
        s, i, scanned = ivf.search_allowed_delta(idx, q, 10, w.nlist, np.tile(allow, (40, 1)))
        _same((s, i), FlatIndex.search_allowed(idx, q, 10, allow), "per query")
        assert scanned == 2 * 32
        # only delta rows: the probe keeps nothing
        only = np.zeros(w.n, dtype=bool)
        only[w.covered:] = True
        s, i, scanned = ivf.search_allowed_delta(idx, q, 10, 4, pack_allow(only))
        _same((s, i), FlatIndex.search_allowed(idx, q, 10, pack_allow(only)), "delta only")
        assert scanned == 2 * (w.n - w.covered) and i[i >= 0].min() >= w.covered
        # a few delta rows: only their tiles are planned
        few = np.zeros(w.n, dtype=bool)
        few[[w.covered + 1, w.covered + 2, w.n - 1]] = True
        assert ivf.search_allowed_delta(idx, q[:3], 5, 4, pack_allow(few))[2] == 32 + (w.n - w.covered - 1) % 32 + 1


def test_device_entry_point_equals_the_host_form(world_a, gpu):
    torch = gpu
    from rassengine_amd.engine import pack_allow
    w = world_a
    idx, ivf = w.idx, w.ivf
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    q = np.concatenate([w.q, w.q[:30] + 0.05 * rng.standard_normal((30, w.dim)).astype(np.float32)])    # 70: 32 + 32 + 6
    bits = rng.random((70, w.n)) < 0.2
    qf = np.array([r % 4 + 1 for r in range(70)], dtype=np.int32)
    m = np.full(70, PM, dtype=np.int32)
    for allow, f, mm in ((pack_allow(bits), None, None), (pack_allow(bits), qf, m), (pack_allow(bits[0]), None, None)):
        for nprobe in (2, w.nlist):
            want = ivf.search_allowed_delta(idx, q, 7, nprobe, allow, f, mm)
            d_allow = torch.from_numpy(allow.view(np.int32)).to(dev)
            ds, di, dn = ivf.search_allowed_delta_device(idx, torch.from_numpy(q).to(dev), 7, nprobe, d_allow,
                                                         None if f is None else torch.from_numpy(f).to(dev),
                                                         None if mm is None else torch.from_numpy(mm).to(dev))
            w.eng.synchronize()
            _same((ds.cpu().numpy(), di.cpu().numpy()), want[:2], (nprobe, f is not None))
            assert int(dn.item()) == want[2] > 0
            # ... and a device bitmap through the host-shaped method
            got = ivf.search_allowed_delta(idx, q, 7, nprobe, d_allow, f, mm)
            _same(got[:2], want[:2], "device bitmap")
            assert got[2] == want[2]


def _boundary(monkeypatch, allow_switch):
    from rassengine_amd import config, indexer
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import Engine
    from rassengine_amd.ivf import open_backed_index
    monkeypatch.setattr(config, "RASS_IVF_NLIST", 16)
    monkeypatch.setattr(config, "RASS_IVF_NPROBE", 16)
    monkeypatch.setattr(config, "RASS_IVF_MIN_ROWS", 1500)
    monkeypatch.setattr(config, "RASS_IVF_REBUILD_FRACTION", 10.0)
    monkeypatch.setattr(config, "RASS_SCORE_MODE", "cosine")
    if allow_switch:
        monkeypatch.setattr(config, "RASS_IVF_ALLOW", True, raising=False)
    eng = Engine(0, 128)
    REGISTRY.clear()
    REGISTRY.set_index_factory(lambda name: open_backed_index(eng, name))
    rng = np.random.default_rng(31)
    name = "rass-idx-ivf-allow"
    docs = [{"doc_id": f"n-{i}", "doc_type": "note" if i % 5 == 0 else "unstructured",
             "patientId": "rare" if i % 160 == 0 else f"p{i % 3}"} for i in range(3200)]
    emb = rng.standard_normal((3200, 128)).astype(np.float32)
    for a in range(0, 3200, 800):
        indexer.add_documents(name, docs[a:a + 800], emb[a:a + 800])
    idx = REGISTRY.get(name).index
    assert idx.builds == 1 and idx.covered == 1600 and idx.rows == 3200     # built at 1 600 rows: half the index is the delta
    return eng, idx, indexer.HipIndexer(None, name), rng.standard_normal(128).astype(np.float32)


def test_boundary_routes_broad_filters_through_the_ivf(gpu, monkeypatch):
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import FlatIndex
    from rassengine_amd.ivf import IvfIndex
    eng, idx, hip, q = _boundary(monkeypatch, allow_switch=True)
    try:
        assert idx.policy.allow_probe is True
        served = {"ivf": 0, "flat": 0}
        real_ivf, real_flat = IvfIndex.search_allowed_delta, FlatIndex.search_allowed

        def via_ivf(self, *a, **kw):
            served["ivf"] += 1
            return real_ivf(self, *a, **kw)

        def via_flat(self, *a, **kw):
            served["flat"] += 1
            return real_flat(self, *a, **kw)
        monkeypatch.setattr(IvfIndex, "search_allowed_delta", via_ivf)
        monkeypatch.setattr(FlatIndex, "search_allowed", via_flat)
        broad = {"term": {"doc_type": "unstructured"}}                      # 2 560 chunks: 32 x that against 1 600 probed rows
        selective = {"term": {"patientId": "rare"}}                         # 20 chunks: 640 against 1 600
        got = [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=8, where=broad)]
        assert served == {"ivf": 1, "flat": 0} and idx.ivf_allowed == 1
        got_within = [(d["doc_id"], s) for d, s in hip.semantic_search_within(q, k=8, doc_types=["unstructured"])]
        assert served == {"ivf": 2, "flat": 0} and got_within == got
        got_sel = [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=8, where=selective)]
        assert served == {"ivf": 2, "flat": 1}
        got_big = [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=40, where=broad)]   # k > 32: the flat scan
        assert served == {"ivf": 2, "flat": 2} and got_big[:8] == got
        # nprobe = nlist: the IVF's answers are the flat scan's
        idx.policy.allow_probe = False
        assert [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=8, where=broad)] == got
        assert [(d["doc_id"], s) for d, s in hip.semantic_search_filtered(q, k=8, where=selective)] == got_sel
        assert served == {"ivf": 2, "flat": 4}
        assert len(got) == 8 and all(int(d[2:]) % 5 != 0 for d, _ in got)
        assert len(got_sel) == 8 and all(int(d[2:]) % 160 == 0 for d, _ in got_sel)
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()


def test_boundary_without_the_switch_takes_the_flat_path(gpu, monkeypatch):
    """The default: an index with an IVF answers a filtered search by the exact flat allow scan, whatever the filter."""
    from rassengine_amd import ivf as ivf_mod
    from rassengine_amd.docstore import REGISTRY
    from rassengine_amd.engine import FlatIndex
    eng, idx, hip, q = _boundary(monkeypatch, allow_switch=False)
    try:
        assert idx.ivf is not None and not getattr(idx.policy, "allow_probe", False)
        flat_calls = []
        real_flat = FlatIndex.search_allowed

        def via_flat(self, *a, **kw):
            flat_calls.append(1)
            return real_flat(self, *a, **kw)
        monkeypatch.setattr(FlatIndex, "search_allowed", via_flat)
        if hasattr(ivf_mod.IvfIndex, "search_allowed_delta"):
            def never(self, *a, **kw):
                raise AssertionError("the IVF served a filtered search although the switch is off")
            monkeypatch.setattr(ivf_mod.IvfIndex, "search_allowed_delta", never)
        got = hip.semantic_search_filtered(q, k=8, where={"term": {"doc_type": "unstructured"}})
        assert len(flat_calls) == 1 and len(got) == 8 and all(int(d["doc_id"][2:]) % 5 != 0 for d, _ in got)
        assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
    finally:
        REGISTRY.set_index_factory(None)
        REGISTRY.clear()
        eng.close()


def test_error_paths_leave_the_index_usable(world_b):
    from rassengine_amd._native import RassError
    from rassengine_amd.engine import FlatIndex, pack_allow
    from rassengine_amd.ivf import IvfIndex
    w = world_b
    idx, ivf, q = w.idx, w.ivf, w.q
    allow = pack_allow(w.bits["half"])
    want = ivf.search_allowed_delta(idx, q, 10, 4, allow)

    def refused(code, fn, *a):
        with pytest.raises(RassError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, str(e.value))
    for dtype in ("bf16", "int8"):                                          # their scans have no bitmap mode
        low = IvfIndex.build(idx, nlist=w.nlist, centroids=w.cent, assign=w.assign, dtype=dtype, n_rows=w.covered)
        try:
            refused(ERR_UNSUPPORTED, low.search_allowed_delta, idx, q, 10, 4, allow)
            assert low.search_delta(idx, q[:4], 5, 4)[1].min() >= 0        # ... and still probes
        finally:
            low.close()
    refused(ERR_UNSUPPORTED, ivf.search_allowed_delta, idx, q, 33, 4, allow)
    refused(ERR_INVALID, ivf.search_allowed_delta, idx, q, 0, 4, allow)
    refused(ERR_INVALID, ivf.search_allowed_delta, idx, q, 10, 0, allow)
    refused(ERR_INVALID, ivf.search_allowed_delta, idx, q, 10, 4, allow[:, :-1])         # words too small
    refused(ERR_INVALID, ivf.search_allowed_delta, idx, q, 10, 4, allow[:3])             # n_bitmaps neither 1 nor nq
    refused(ERR_UNSUPPORTED, ivf.probe_lists, q, 33)
    got = ivf.search_allowed_delta(idx, q, 10, 4, allow)
    _same(got[:2], want[:2], "after the refusals")
    assert got[2] == want[2]
    _same(FlatIndex.search_allowed(idx, q[:2], 3, allow[:2]), FlatIndex.search_allowed(idx, q[:2], 3, allow[:2]), "flat")


def test_a_compacted_source_is_refused(gpu):
    torch = gpu
    from rassengine_amd._native import RassError
    from rassengine_amd.engine import Engine, pack_allow
    from rassengine_amd.ivf import IvfIndex
    rng = np.random.default_rng(9)
    eng = Engine(0, 128)
    try:
        flat = eng.open_index("ivf-allow-stale")
        x = rng.standard_normal((2_048, 128)).astype(np.float32)
        flat.add(x)
        ivf = IvfIndex.build(flat, nlist=4, centroids=torch.from_numpy(x[:4].copy()).to("cuda:0"))
        allow = pack_allow(np.ones(2_048, dtype=bool))
        s, i, _ = ivf.search_allowed_delta(flat, x[:3], 1, 4, allow)
        assert i[:, 0].tolist() == [0, 1, 2]
        flat.delete(1)
        flat.compact()                                                      # the IVF's ids are ordinals of the old layout
        with pytest.raises(RassError) as e:
            ivf.search_allowed_delta(flat, x[:3], 1, 4, allow)
        assert e.value.code == ERR_INVALID and "compacted" in str(e.value)
        after = flat.search_allowed(x[:3], 1, allow)[1][:, 0].tolist()     # the source still answers: row 1 is gone, row 2 moved down
        assert after[0] == 0 and after[2] == 1
        ivf.close()
    finally:
        eng.close()


@pytest.mark.parametrize("n", [20, 1_000, 4_128])
def test_allow_count_equals_popcount_below_rows(gpu, n):
    torch = gpu
    from rassengine_amd._native import RassError
    from rassengine_amd.engine import Engine, unpack_allow
    rng = np.random.default_rng(n)
    eng = Engine(0, 128)
    try:
        flat = eng.open_index(f"allow-count-{n}")
        flat.add(rng.standard_normal((n, 128)).astype(np.float32))
        flat.delete(n // 2)                                                 # a tombstone still counts: the bitmap names it
        words = flat.allow_words + 2
        allow = rng.integers(0, 1 << 32, size=(5, words), dtype=np.uint64).astype(np.uint32)
        allow[3] = 0
        allow[4] = 0xFFFFFFFF
        want = unpack_allow(allow[:, :flat.allow_words], n).sum(axis=1).astype(np.int64)
        assert want[3] == 0 and want[4] == n
        assert np.array_equal(flat.allow_count(allow), want)
        assert np.array_equal(flat.allow_count(allow[1]), want[1:2])                       # one shared bitmap
        d = torch.from_numpy(allow.view(np.int32)).to("cuda:0")
        assert np.array_equal(flat.allow_count(d), want) and np.array_equal(flat.allow_count(d[2]), want[2:3])
        assert np.array_equal(flat.allow_count(allow[:, :flat.allow_words]), want)
        if flat.allow_words > 1:
            with pytest.raises(RassError):
                flat.allow_count(np.ascontiguousarray(allow[:, :flat.allow_words - 1]))
    finally:
        eng.close()
