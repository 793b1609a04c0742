"""What a semantic terms aggregation costs next to its siblings: 1 M x 1024 fp32 rows, 32 queries.

Rows are dealt to patients in runs of 32 adjacent rows (one document's chunks).  Per setting of n_groups (100 and 10 000) and
of the thresholds — taken from a k-NN answer's own scores: just above each query's best score (about 0 hits), its 1 000th
score (about 1 000 hits) and -inf (every row a hit) — in one process on one index of the same rows, alternating:
  (a) the aggregate launch group (rass_index_aggregate_device, size = 10), hipEvents on the engine stream, and its scan
      kernel alone (the engine's kernel timing);
  (b) a plain k = 10 launch group (rass_index_search_device);
  (c) the grouped launch group (rass_index_search_grouped_device, k = 10): the yardstick, it pays the first of the aggregate's
      two atomics for every matching row whatever the threshold.
Medians of 3 rounds of ITERS calls each.  One JSON line per (n_groups, threshold).  N=<rows> / ITERS=<n> in the environment
shrink it.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rassengine_amd.engine import Engine, HipTimer

n, dim, nq, k = int(os.environ.get("N", 1_000_000)), 1024, 32, 10
iters = int(os.environ.get("ITERS", 30))
rounds = 3
PMASK = 0x00FFFFFF
eng = Engine(0, dim)
rng = np.random.default_rng(7)
q_host = rng.standard_normal((nq, dim), dtype=np.float32)
q = torch.from_numpy(q_host).cuda()
timer = HipTimer()


def timed(fn, reps):
    """Mean milliseconds of fn() by a hipEvent pair on the engine stream."""
    for _ in range(3):
        fn()
    eng.synchronize()
    timer.start(eng.stream)
    for _ in range(reps):
        fn()
    timer.stop(eng.stream)
    eng.synchronize()
    return timer.elapsed_ms() / reps


def build(name, keys):
    """An index of n seeded rows (generated on the device, 65 536 at a time) tagged with `keys`."""
    idx = eng.open_index(name, n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    tags = torch.from_numpy(keys.astype(np.int32)).cuda()
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), m, tags[r0:r0 + m].data_ptr(), normalize=True)
        eng.synchronize()
    return idx


runs = np.arange(n) // 32
out_g = torch.empty((nq, k), dtype=torch.int32, device="cuda")
out_c = torch.empty((nq, k), dtype=torch.int64, device="cuda")
out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
n_buckets = torch.empty((nq,), dtype=torch.int64, device="cuda")
total = torch.empty((nq,), dtype=torch.int64, device="cuda")
status = torch.empty((1,), dtype=torch.int32, device="cuda")

for n_groups in (100, 10_000):
    idx = build("probe", runs % n_groups)
    knn_s, _ = idx.search(q_host, min(1000, n))
    thresholds = [("about 0", np.nextafter(knn_s[:, 0], np.float32(np.inf))), ("about 1000", knn_s[:, -1].copy()),
                  ("all rows", np.full(nq, -np.inf, dtype=np.float32))]
    topk = lambda: idx.search_device(q.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr())
    grouped = lambda: idx.search_grouped_device(q.data_ptr(), nq, k, PMASK, n_groups, out_s.data_ptr(), out_i.data_ptr(),
                                                out_g.data_ptr(), total.data_ptr(), status.data_ptr())
    for name, thr_host in thresholds:
        thr = torch.from_numpy(np.ascontiguousarray(thr_host, dtype=np.float32)).cuda()
        torch.cuda.synchronize()
        agg = lambda: idx.search_counts_device(q.data_ptr(), nq, thr.data_ptr(), k, PMASK, n_groups, out_g.data_ptr(),
                                               out_c.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), n_buckets.data_ptr(),
                                               total.data_ptr(), status.data_ptr())
        a_ms, b_ms, c_ms = [], [], []
        for _ in range(rounds):             # (a), (b) and (c) alternate: the ratios are taken inside one process on one index
            a_ms.append(timed(agg, iters))
            b_ms.append(timed(topk, iters))
            c_ms.append(timed(grouped, iters))
        eng.kernel_timing_begin(8)
        agg()
        eng.synchronize()
        scan_ms, launches = eng.kernel_timing_end()
        assert int(status.item()) == 0
        a, b, c = float(np.median(a_ms)), float(np.median(b_ms)), float(np.median(c_ms))
        print(json.dumps({
            "rows": n, "dim": dim, "nq": nq, "size": k, "n_groups": n_groups, "hits": name,
            "mean_total_hits": float(total.double().mean().item()), "mean_n_buckets": float(n_buckets.double().mean().item()),
            "a_aggregate_group_ms": round(a, 4), "a_rounds_ms": [round(v, 4) for v in a_ms],
            "a_scan_kernel_ms": round(scan_ms, 4), "a_scan_launches": launches,
            "a_rest_normalise_memset_select_ms": round(a - scan_ms, 4), "table_bytes": nq * n_groups * 12,
            "b_topk10_group_ms": round(b, 4), "b_rounds_ms": [round(v, 4) for v in b_ms],
            "c_grouped_group_ms": round(c, 4), "c_rounds_ms": [round(v, 4) for v in c_ms],
            "a_over_b": round(a / b, 3), "a_over_c": round(a / c, 3),
        }), flush=True)
    eng.drop_index("probe")
eng.close()
