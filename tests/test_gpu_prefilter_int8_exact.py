"""Prefilter mode 3 ("int8_exact"): the int8 candidate scan at depth 128 with hi + lo queries, the exact re-rank, the per-query
certificate and the fp32 fallback.  Every search is compared with the SAME index in mode 0, ids and scores bit for bit; the
candidate lists, tau and the flags are compared with the numpy restatement (tests/certified_ref.py) bit for bit."""
import numpy as np
import pytest

from tests import certified_ref as CR

pytestmark = pytest.mark.gpu


def _both(idx, q, k, qf=None, qm=None):
    idx.set_prefilter("off")
    s0, i0 = idx.search(q, k, q_filter=qf, q_filter_mask=qm)
    idx.set_prefilter("int8_exact")
    assert idx.prefilter_mode == "int8_exact"
    s3, i3 = idx.search(q, k, q_filter=qf, q_filter_mask=qm)
    return (s0, i0), (s3, i3)


def _same(a, b, what=""):
    (s0, i0), (s3, i3) = a, b
    assert np.array_equal(i0, i3), what
    assert np.array_equal(s0.view(np.uint32), s3.view(np.uint32)), what


@pytest.mark.parametrize("dim", [384, 768, 1024, 1100, 2048])
def test_mode3_equals_flat_bit_for_bit(gpu, dim):
    from rassengine_amd.engine import Engine
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(dim)
        n = 6000 + 37                                   # a ragged last tile
        x = rng.standard_normal((n, dim)).astype(np.float32)
        tags = rng.integers(0, 3, size=n).astype(np.int32)
        idx = eng.open_index("c")
        idx.add(x, tags=tags)
        idx.delete(5)
        for nq in (1, 17, 32):
            q = rng.standard_normal((nq, dim)).astype(np.float32)
            q[: nq // 2] = x[rng.integers(0, n, size=nq // 2)] + 0.01 * q[: nq // 2]   # easy and hard queries
            qf = rng.integers(-1, 3, size=nq).astype(np.int32)
            for k in (1, 10, 16, 32):
                a, b = _both(idx, q, k)
                _same(a, b, (dim, nq, k))
            a, b = _both(idx, q, 10, qf)
            _same(a, b, (dim, nq, "filter"))
        st = idx.certify_stats()
        assert st["queries"] > 0 and st["certified"] + st["fallbacks"] == st["queries"]
    finally:
        eng.close()


def test_masked_filters_tombstones_small_and_empty(gpu):
    from rassengine_amd.engine import Engine
    dim = 768
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(3)
        empty = eng.open_index("empty")
        q = rng.standard_normal((3, dim)).astype(np.float32)
        a, b = _both(empty, q, 10)
        _same(a, b, "empty")
        for n in (5, 100, 3000):                        # fewer eligible rows than k, than C, and more
            x = rng.standard_normal((n, dim)).astype(np.float32)
            tags = (rng.integers(0, 4, size=n) | (rng.integers(0, 3, size=n) << 24)).astype(np.int32)
            idx = eng.open_index(f"s{n}")
            idx.add(x, tags=tags)
            for r in range(0, n, 7):
                idx.delete(r)
            q = rng.standard_normal((17, dim)).astype(np.float32)
            qf = rng.integers(0, 4, size=17).astype(np.int32)
            qm = np.full(17, 0x00ffffff, dtype=np.int32)
            for k in (1, 10, 32):
                a, b = _both(idx, q, k, qf, qm)
                _same(a, b, (n, k, "masked"))
                a, b = _both(idx, q, k, qf)
                _same(a, b, (n, k, "exact filter"))
    finally:
        eng.close()


def _batch(idx, q, k, groups_stride):
    import torch
    nq = q.shape[0]
    dq = torch.from_numpy(q).cuda()
    ng = (nq + 31) // 32
    s = torch.full((ng * groups_stride,), 7.0, dtype=torch.float32, device="cuda")
    i = torch.full((ng * groups_stride,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    idx.search_device_batch(dq.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), out_scores_group_stride=groups_stride,
                            out_ids_group_stride=groups_stride)
    idx.engine.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def test_batch_api_1024_queries_with_group_strides(gpu):
    from rassengine_amd.engine import Engine
    dim, n, k = 1024, 20000, 10
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(11)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        idx = eng.open_index("b")
        idx.add(x)
        q = rng.standard_normal((1024, dim)).astype(np.float32)
        q[::2] = x[rng.integers(0, n, size=512)]
        gs = 32 * k + 8
        idx.set_prefilter("off")
        a = _batch(idx, q, k, gs)
        idx.set_prefilter("int8_exact")
        b = _batch(idx, q, k, gs)
        _same(a, b, "batch")
        st = idx.certify_stats()
        assert st["queries"] == 1024 and st["certified"] >= 512, st
    finally:
        eng.close()


def test_save_load_then_set_mode_again(gpu, tmp_path):
    from rassengine_amd.engine import Engine
    dim = 384
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(5)
        x = rng.standard_normal((2500, dim)).astype(np.float32)
        idx = eng.open_index("p")
        idx.add(x)
        idx.set_prefilter("int8_exact")
        q = rng.standard_normal((9, dim)).astype(np.float32)
        s1, i1 = idx.search(q, 10)
        path = str(tmp_path / "p.idx")
        idx.save(path)
        idx2 = eng.load_index("p2", path)
        idx2.set_prefilter("int8_exact")
        s2, i2 = idx2.search(q, 10)
        assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
        a, b = _both(idx2, q, 10)
        _same(a, b, "loaded")
    finally:
        eng.close()


def _adversarial(kind, dim, rng):
    if kind == "near_duplicates":   # 400 copies of the query below int8 resolution: ties in a(y), distinct fp32 scores
        n = 9000
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q = rng.standard_normal((4, dim)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        for j in range(4):
            rows = np.arange(400) + 1000 * j
            x[rows] = q[j] + 1e-4 * rng.standard_normal((400, dim)).astype(np.float32)
        return x, q
    # one row with a huge outlier component: R becomes large, every query falls back
    n = 5000
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[77, 3] = 500.0
    q = rng.standard_normal((4, dim)).astype(np.float32)
    return x, q


@pytest.mark.parametrize("kind", ["near_duplicates", "outlier"])
def test_adversarial_corpora_fall_back_and_stay_exact(gpu, kind):
    from rassengine_amd.engine import Engine
    dim = 1024
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(21)
        x, q = _adversarial(kind, dim, rng)
        idx = eng.open_index(kind)
        idx.add(x)
        a, b = _both(idx, q, 10)
        _same(a, b, kind)
        st = idx.certify_stats()
        assert st["fallbacks"] > 0, st
        if kind == "outlier":
            assert st["fallbacks"] == st["queries"] and st["R"] > 0.03, st   # iid unit rows: R ~ 0.014
        # the same corpus through the batch API
        qb = np.repeat(q, 16, axis=0)                    # 64 queries: two launch groups
        idx.set_prefilter("off")
        a = _batch(idx, qb, 10, 32 * 10)
        idx.set_prefilter("int8_exact")
        b = _batch(idx, qb, 10, 32 * 10)
        _same(a, b, kind + " batch")
        assert idx.certify_stats()["fallbacks"] > 0
    finally:
        eng.close()


def test_queries_from_stored_rows_all_certify(gpu):
    from rassengine_amd.engine import Engine
    dim, n = 1024, 50000
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(2)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        idx = eng.open_index("easy")
        idx.add(x)
        idx.set_prefilter("int8_exact")
        q = x[rng.integers(0, n, size=32)]
        idx.search(q, 10)
        st = idx.certify_stats()
        assert st["queries"] == 32 and st["certified"] == 32, st
    finally:
        eng.close()


@pytest.mark.parametrize("dim", [768, 1100])
def test_candidate_lists_tau_and_flags_equal_the_restatement(gpu, oracle, dim):
    import torch
    from rassengine_amd import ops
    from rassengine_amd.engine import Engine
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(40 + dim)
        n = 7000 + 13
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x[11] = 0.0
        tags = rng.integers(0, 3, size=n).astype(np.int32)
        idx = eng.open_index("par")
        idx.set_prefilter("int8_exact")
        idx.add(x[:4000], tags=tags[:4000])
        idx.add(x[4000:], tags=tags[4000:])
        idx.delete(17)
        tags[17] = -1
        xn = idx.get_rows(0, n)
        k = 10
        for nq in (1, 20):
            q = rng.standard_normal((nq, dim)).astype(np.float32)
            q[0] = x[5]
            qf = rng.integers(-1, 3, size=nq).astype(np.int32)
            for f in (None, qf):
                s, r, tau, cert = idx.candidates_exact_device(torch.from_numpy(q).cuda(), k, f)
                s, r, tau, cert = s.cpu().numpy(), r.cpu().numpy(), tau.cpu().numpy(), cert.cpu().numpy()
                # the query as the device normalised it: q_lo quantises a residual ~1/250 of q, so a 1-ulp difference in one
                # component of a host-side normalisation can move a q_lo entry across a rounding boundary
                qn = ops.normalize_rows(torch.from_numpy(q).cuda()).cpu().numpy()
                cs, cr, ct = CR.candidates(xn, qn, tags=tags, qfilter=f)
                assert np.array_equal(r, cr), (nq, f is not None)
                assert np.array_equal(s.view(np.uint32), cs.view(np.uint32)), (nq, f is not None)
                assert np.array_equal(tau.view(np.uint32), ct.view(np.uint32)), (nq, f is not None)
                # the flags: the certificate restated with the index's R, V, Y (recomputed here from the rows)
                rho, nu, yn = CR.row_terms(xn)
                qnorm, rq, qa = CR.query_terms(qn)
                B = CR.bound(rho.max(), nu.max(), yn.max(), qnorm, rq, qa, dim)
                exact = (qn.astype(np.float32) @ xn.T.astype(np.float32))
                ok = CR.eligible(n, nq, tags, f)
                for j in range(nq):
                    sc = np.sort(exact[j, cr[j][cr[j] >= 0]])[::-1]
                    tk = sc[k - 1] if len(sc) >= k else -np.inf
                    want = ct[j] == -np.inf or (ct[j] + B[j] < tk)
                    # the restated B uses fp64 norms, the device's their fp32 upper bounds: within 1e-5 of the boundary the
                    # two may decide differently, and only there is the flag not compared
                    margin = abs(float(ct[j]) + B[j] - float(tk)) if np.isfinite(ct[j]) else 1.0
                    if margin > 1e-5:
                        assert bool(cert[j]) == bool(want), (j, ct[j], B[j], tk)
                    assert ok[j].sum() > 0
    finally:
        eng.close()


@pytest.mark.parametrize("outlier", [False, True])
def test_caller_assigned_ids_equal_flat(gpu, outlier):
    """An index whose rows carry caller-assigned global ids (a serving shard): with no query failing (the idle fallback) and with
    every query failing (the fallback's ids go through the id map)."""
    from rassengine_amd.engine import Engine
    dim = 1024
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(31)
        n = 20000
        x = rng.standard_normal((n, dim)).astype(np.float32)
        if outlier:
            x[77, 3] = 60.0
        idx = eng.open_index("gid")
        idx.add(x[:12000], first_global_id=5_000_000)
        idx.add(x[12000:], first_global_id=9_000_000)
        assert idx.has_global_ids
        q = rng.standard_normal((20, dim)).astype(np.float32)
        q[:10] = x[rng.integers(0, n, size=10)]
        for k in (1, 10, 32):
            a, b = _both(idx, q, k)
            _same(a, b, ("gid", outlier, k))
        idx.set_prefilter("off")
        a = _batch(idx, q, 10, 32 * 10)
        idx.set_prefilter("int8_exact")
        b = _batch(idx, q, 10, 32 * 10)
        _same(a, b, ("gid batch", outlier))
        st = idx.certify_stats()
        assert (st["fallbacks"] == st["queries"]) if outlier else (st["fallbacks"] == 0), st
    finally:
        eng.close()


def test_device_row_maxima_bound_the_rows(gpu):
    """R and V as the index keeps them (atomicMax folds on add and re-quantisation) are upper bounds of max rho_y and max nu_y,
    and tight to fp32 rounding."""
    from rassengine_amd.engine import Engine
    dim = 768
    eng = Engine(0, dim)
    try:
        rng = np.random.default_rng(9)
        x = rng.standard_normal((5000, dim)).astype(np.float32)
        x[100, 1] = 30.0
        x[101] = 0.0
        idx = eng.open_index("rv")
        idx.set_prefilter("int8_exact")
        idx.add(x[:3000])
        idx.add(x[3000:])                               # an append that re-quantises a partly filled block
        rho, nu, _ = CR.row_terms(idx.get_rows(0, 5000))
        st = idx.certify_stats()
        assert rho.max() <= st["R"] <= rho.max() * (1 + 1e-6), (st, rho.max())
        assert nu.max() <= st["V"] <= nu.max() * (1 + 1e-6), (st, nu.max())
        idx.set_prefilter("off")
        idx.set_prefilter("int8_exact")                 # recomputed from the rows when the mode is set
        st2 = idx.certify_stats()
        assert st2["R"] == st["R"] and st2["V"] == st["V"] and st2["queries"] == 0
    finally:
        eng.close()
