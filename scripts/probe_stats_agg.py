"""What the stats sub-aggregation costs next to the aggregation it extends: 1 M x 1024 fp32 rows, 32 queries, size 10.

Per setting of the groups — 1 (the global form: no key column), 100 and 10 000, rows dealt to them in runs of 32 adjacent rows
(one document's chunks: the reduced path) and at random (the per-lane path) — and of the thresholds — taken from a k-NN
answer's own scores: just above each query's best score (0 hits), its 1 000th score (about 1 000 hits) and -inf (every row a
hit) — in one process on one index, alternating:
  (a) the stats launch group (rass_index_aggregate_stats_keys_device, a column of values uniform over int32), hipEvents on the
      engine stream, and its scan kernel alone (the engine's kernel timing);
  (b) the aggregate_keys launch group of the unchanged kernel (rass_index_aggregate_keys_device) on the same key column (for
      1 group: a column of zeros), with its run-to-run spread: the yardstick.
Medians of 3 rounds of ITERS calls each.  One JSON line per (groups, dealing, threshold), all of them also written to
profiles/probe_stats_agg_1M_B32.json.  N=<rows> / ITERS=<n> in the environment shrink it (then no file is written).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from rassengine_amd.engine import Engine, HipTimer

full = "N" not in os.environ and "ITERS" not in os.environ
n, dim, nq, size = int(os.environ.get("N", 1_000_000)), 1024, 32, 10
iters = int(os.environ.get("ITERS", 30))
rounds = 3
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


idx = eng.open_index("probe", n)
gen = torch.Generator(device="cuda")
gen.manual_seed(1234)
for r0 in range(0, n, 65536):                     # n seeded rows, generated on the device
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, 0, normalize=True)
    eng.synchronize()
idx.set_attr(0, 0, rng.integers(-(1 << 31) + 1, 1 << 31, size=n).astype(np.int32))
knn_s, _ = idx.search(q_host, min(1000, n))
thresholds = [("0", np.nextafter(knn_s[:, 0], np.float32(np.inf))), ("about 1000", knn_s[:, -1].copy()),
              ("all rows", np.full(nq, -np.inf, dtype=np.float32))]

out = [torch.empty((nq, size), dtype=t, device="cuda") for t in (torch.int32, torch.int64, torch.float32, torch.int64, torch.int64,
                                                                torch.int64, torch.int32, torch.int32)]
n_buckets = torch.empty((nq,), dtype=torch.int64, device="cuda")
total = torch.empty((nq,), dtype=torch.int64, device="cuda")
status = torch.empty((1,), dtype=torch.int32, device="cuda")
lines = []
for n_groups in (1, 100, 10_000):
    for dealing in (("runs of 32", "random") if n_groups > 1 else ("one group",)):
        keys_host = (np.arange(n) // 32) % n_groups if dealing != "random" else rng.integers(0, n_groups, size=n)
        keys = torch.from_numpy(keys_host.astype(np.int32)).cuda()
        for name, thr_host in thresholds:
            thr = torch.from_numpy(np.ascontiguousarray(thr_host, dtype=np.float32)).cuda()
            torch.cuda.synchronize()
            stats = lambda: idx.search_stats_by_keys_device(q.data_ptr(), nq, thr.data_ptr(), size, 0 if n_groups == 1 else keys.data_ptr(),
                                                            n, n_groups, 0, *[o.data_ptr() for o in out], n_buckets.data_ptr(),
                                                            total.data_ptr(), status.data_ptr())
            agg = lambda: idx.search_counts_by_keys_device(q.data_ptr(), nq, thr.data_ptr(), size, keys.data_ptr(), n, n_groups,
                                                           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                                           n_buckets.data_ptr(), total.data_ptr(), status.data_ptr())
            a_ms, b_ms = [], []
            for _ in range(rounds):             # (a) and (b) alternate: the ratio is taken inside one process on one index
                a_ms.append(timed(stats, iters))
                b_ms.append(timed(agg, iters))
            eng.kernel_timing_begin(8)
            stats()
            eng.synchronize()
            scan_ms, launches = eng.kernel_timing_end()
            assert int(status.item()) == 0
            a, b = float(np.median(a_ms)), float(np.median(b_ms))
            lines.append({
                "rows": n, "dim": dim, "nq": nq, "size": size, "n_groups": n_groups, "dealing": dealing, "hits": name,
                "mean_total_hits": float(total.double().mean().item()), "mean_n_buckets": float(n_buckets.double().mean().item()),
                "a_stats_group_ms": round(a, 4), "a_rounds_ms": [round(v, 4) for v in a_ms],
                "a_scan_kernel_ms": round(scan_ms, 4), "a_scan_launches": launches, "table_bytes": nq * n_groups * 32,
                "b_aggregate_keys_group_ms": round(b, 4), "b_rounds_ms": [round(v, 4) for v in b_ms],
                "b_spread": round((max(b_ms) - min(b_ms)) / b, 4), "a_over_b": round(a / b, 3),
                "a_inside_b_spread": bool(min(b_ms) <= a <= max(b_ms)),
            })
            print(json.dumps(lines[-1]), flush=True)
eng.drop_index("probe")
eng.close()
if full:
    with open(os.path.join(ROOT, "profiles", "probe_stats_agg_1M_B32.json"), "w", encoding="utf-8") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
