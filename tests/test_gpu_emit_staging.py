"""The staging the host range, grouped and aggregation searches share: ONE pinned block per host slot (``HostSlot::h_io``)
and ONE device block per engine (``eng->d_io``), each grown to the layout the call needs and viewed as a Range / Group /
AggIoView.  The allow-list search runs through the same host loop (``host_groups``) beside them.

What can go wrong is a block grown, or viewed differently, under an answer that still lives in it: the calls below alternate
the kinds on one engine (the aggregation's layout is the largest, so its first call grows both blocks behind a range search)
and run two kinds at once on two slots.  600 rows x 64 columns, 33 queries = two host groups, the second of one query.
Expected answers come from a fresh engine holding the same rows AND from the CPU oracle, through the helpers of the
searches' own test files; everything must be EQUAL, no tolerance.
"""
import threading

import numpy as np
import pytest

from tests import test_gpu_aggregate as A
from tests import test_gpu_group_search as G
from tests import test_gpu_range_search as R

pytestmark = pytest.mark.gpu

N, DIM, NQ, N_GROUPS = 600, 64, 33, 6
PMASK = G.PMASK


def open_index(case):
    from rassengine_amd.engine import Engine
    eng = Engine(0, DIM)
    idx = eng.open_index("staging")
    idx.add(case.xn, tags=case.tags, normalize=False)
    return eng, idx


@pytest.fixture(scope="module")
def world(gpu, oracle):
    """The case (rows, 6 patient groups, 33 queries, the oracle's scores), its ranking, per-query thresholds with 1..40 hits,
    a shared bitmap, and one long-lived engine holding the rows."""
    from rassengine_amd.engine import pack_allow
    rng = np.random.default_rng(515)
    case = R.Corpus(gpu, oracle, N, DIM, NQ, seed=514, tags=G.patient_tags(rng, N, N_GROUPS, runs=False))
    ranked = case.ranked()
    thr = R.boundary_thresholds(ranked, 40)
    bits = rng.random((1, N)) < 0.3
    eng, idx = open_index(case)
    w = {"case": case, "ranked": ranked, "thr": thr, "bits": bits, "allow": pack_allow(bits)[0], "idx": idx, "hung": False}
    yield w
    if not w["hung"]:            # a call that never came back still owns the engine: leave it alone
        eng.close()


def calls(w):
    """(name, call(idx), the oracle's answer) in the order the first test runs them."""
    case, thr, allow = w["case"], w["thr"], w["allow"]

    def allowed_expect(k):
        es = np.full((NQ, k), R.NEG_INF, dtype=np.float32)
        ei = np.full((NQ, k), -1, dtype=np.int64)
        rows = np.flatnonzero(w["bits"][0])
        for q in range(NQ):
            s = case.scores[q, rows]
            order = np.lexsort((rows, -s))[:k]
            es[q, :len(order)], ei[q, :len(order)] = s[order], rows[order]
        return es, ei

    range8 = ("range 8", lambda idx: idx.search_range(case.q_raw, thr, max_hits=8), R.expect(w["ranked"], thr, 8, device=False))
    return [
        range8,
        ("counts 4096", lambda idx: idx.search_counts(case.q_raw, thr, 4096, PMASK, N_GROUPS),
         A.expect(case, case.tags, PMASK, N_GROUPS, 4096, thr)[:6]),
        ("grouped 16", lambda idx: idx.search_grouped(case.q_raw, 16, PMASK, N_GROUPS),
         G.expect(case, case.tags, PMASK, N_GROUPS, 16)[:4]),
        ("range 4096", lambda idx: idx.search_range(case.q_raw, thr, max_hits=4096), R.expect(w["ranked"], thr, 4096, device=False)),
        ("allowed 40", lambda idx: idx.search_allowed(case.q_raw, 40, allow), allowed_expect(40)),
        range8,
    ]


def same(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, j, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def test_growth_across_kinds(world):
    got = [(name, call(world["idx"]), want) for name, call, want in calls(world)]       # one engine, in this order
    for name, answer, want in got:
        same(answer, want, name + " vs the oracle")
    for (name, answer, _), (_, call, _) in zip(got, calls(world)):
        eng, idx = open_index(world["case"])
        try:
            same(answer, call(idx), name + " vs a fresh engine")
        finally:
            eng.close()
    same(got[0][1], got[-1][1], "the first and the last range answer")
    # the thresholds were chosen to overflow max_hits = 8 for some queries and not for others: both paths ran
    totals = got[0][1][2]
    assert (totals > 8).any() and (totals <= 8).any()


def test_two_slots_at_once(world):
    case, thr, idx = world["case"], world["thr"], world["idx"]
    jobs = [("range", lambda: idx.search_range(case.q_raw, thr, max_hits=64)),
            ("counts", lambda: idx.search_counts(case.q_raw, thr, 8, PMASK, N_GROUPS))]
    want = {name: call() for name, call in jobs}                                         # single-threaded, beforehand
    same(want["range"], R.expect(world["ranked"], thr, 64, device=False), "range vs the oracle")
    same(want["counts"], A.expect(case, case.tags, PMASK, N_GROUPS, 8, thr)[:6], "counts vs the oracle")
    problems = []

    def work(name, call):
        try:
            for it in range(20):
                same(call(), want[name], (name, "iteration", it))
        except BaseException as e:       # reported by the test's own thread
            problems.append((name, repr(e)))

    threads = [threading.Thread(target=work, args=job, daemon=True) for job in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    if any(t.is_alive() for t in threads):
        world["hung"] = True
        pytest.fail("a search did not come back within 60 s")
    assert not problems, problems
