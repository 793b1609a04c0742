"""What a score-threshold (range) search costs next to the top-k searches it replaces: 1 M x 1024 fp32 rows, 32 queries.

Per threshold setting (totals of about 0, 100 and 4 000 rows per query, and -inf: one atomic per (tile, query), every
row a hit, every query overflowing), in one process:
  (a) the range search of the group (rass_index_search_range_device), hipEvents on the engine stream;
  (b) a plain k = 10 launch group (rass_index_search_device), the same way;
  (c) rass_index_search_ex(k = max_hits) for the same max_hits: what a caller had to run before, ceil(max_hits / 32)
      corpus passes (host call: wall clock, its round trips included).
One JSON line per setting.  N=<rows> / ITERS=<n> in the environment shrink it.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rassengine_amd.engine import Engine, HipTimer

n, dim, nq = int(os.environ.get("N", 1_000_000)), 1024, 32
iters = int(os.environ.get("ITERS", 50))
eng = Engine(0, dim)
idx = eng.open_index("probe", n)
idx.fill_synthetic(n, 1234)
eng.synchronize()
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


# thresholds from the index's own ranking: the score at rank 100 / 4 000 of every query
top_s, _ = idx.search(q_host, 4096)
settings = [("about 0", np.nextafter(top_s[:, 0], np.float32(np.inf)), 256),
            ("about 100", top_s[:, 99].copy(), 256),
            ("about 4000", top_s[:, 3999].copy(), 4096),
            ("-inf", np.full(nq, -np.inf, dtype=np.float32), 4096)]

k10_s = torch.empty((nq, 10), device="cuda")
k10_i = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
topk_ms = timed(lambda: idx.search_device(q.data_ptr(), nq, 10, k10_s.data_ptr(), k10_i.data_ptr()), iters)

for name, thr_host, max_hits in settings:
    thr = torch.from_numpy(np.ascontiguousarray(thr_host, dtype=np.float32)).cuda()
    out_s = torch.empty((nq, max_hits), device="cuda")
    out_i = torch.empty((nq, max_hits), dtype=torch.int64, device="cuda")
    total = torch.empty((nq,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    range_ms = timed(lambda: idx.search_range_device(q.data_ptr(), nq, thr.data_ptr(), max_hits, out_s.data_ptr(),
                                                     out_i.data_ptr(), total.data_ptr()), iters)
    eng.kernel_timing_begin(8)
    idx.search_range_device(q.data_ptr(), nq, thr.data_ptr(), max_hits, out_s.data_ptr(), out_i.data_ptr(), total.data_ptr())
    eng.synchronize()
    scan_ms, launches = eng.kernel_timing_end()
    t0 = time.perf_counter()
    idx.search(q_host, max_hits)
    ex_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    idx.search_range(q_host, thr_host, max_hits=max_hits)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({
        "rows": n, "dim": dim, "nq": nq, "totals": name, "max_hits": max_hits,
        "mean_total": float(total.double().mean().item()),
        "a_range_group_ms": round(range_ms, 4), "a_range_scan_kernel_ms": round(scan_ms / max(launches, 1), 4),
        "b_topk10_group_ms": round(topk_ms, 4), "c_search_ex_k_max_hits_host_ms": round(ex_ms, 3),
        "range_host_call_ms": round(host_ms, 3),
        "a_over_b": round(range_ms / topk_ms, 3), "c_over_a": round(ex_ms / range_ms, 2),
    }), flush=True)
eng.close()
