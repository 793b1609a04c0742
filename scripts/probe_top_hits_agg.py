"""What the terms aggregation with top hits costs next to the two calls it replaces: 1 M x 1024 fp32 rows, 32 queries, size = 10.

Rows are dealt to groups in runs of 32 adjacent rows (one document's chunks), at 100 and 10 000 groups; the thresholds give no
hit (above every cosine), about 1 000 hits per query (each query's 1 000th best score, from a torch matmul: "about") and every
row (-inf).  Per setting, in one process on one index and one key column, all on hipEvents on the engine stream:
  (a) the top-hits launch group (rass_index_aggregate_hits_keys_device) at top_hits 1, 3, 8 and 16 under the count order, and at
      3 under the score order; its scan kernel alone (the engine's kernel timing);
  (b) the aggregation launch group of the unchanged kernels (rass_index_aggregate_keys_device) at the same thresholds;
  (c) the group-hits launch group (rass_index_search_group_hits_keys_device, no threshold: every row) at the same group_size;
  (d) the two-call sequence (b) then (c) that (a) replaces, timed as one.
Every variant alternates with the others round by round; the first round is discarded and the medians of the others are taken.
One JSON line per setting, and the lines again, as a list, in profiles/probe_top_hits_agg_1M_B32.json (OUT=<path> moves it,
OUT= skips it).  N=<rows> / ITERS=<n> in the environment shrink it.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rassengine_amd.engine import Engine, HipTimer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n, dim, nq, size = int(os.environ.get("N", 1_000_000)), 1024, 32, 10
iters = int(os.environ.get("ITERS", 20))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "probe_top_hits_agg_1M_B32.json"))
rounds = 4                              # the first is discarded
SIZES = (1, 3, 8, 16)
eng = Engine(0, dim)
rng = np.random.default_rng(7)
q = torch.from_numpy(rng.standard_normal((nq, dim), dtype=np.float32)).cuda()
qn = torch.nn.functional.normalize(q, dim=1)
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
kth = min(1000, n)
best = torch.full((nq, 0), -2.0, device="cuda")
for r0 in range(0, n, 65536):          # n seeded rows, generated on the device; each query's 1 000 best cosines so far are kept
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    cos = qn @ torch.nn.functional.normalize(x, dim=1).T
    best = torch.topk(torch.cat([best, cos], dim=1), min(kth, best.shape[1] + m), dim=1).values
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, 0, normalize=True)
    eng.synchronize()

THRESHOLDS = {"no hit": torch.full((nq,), 2.0, device="cuda"), "about 1000 hits": best[:, kth - 1].contiguous(),
              "every row": torch.full((nq,), float("-inf"), device="cuda")}
runs = np.arange(n) // 32
out_g = torch.empty((nq, size), dtype=torch.int32, device="cuda")
out_c = torch.empty((nq, size), dtype=torch.int64, device="cuda")
out_s = torch.empty((nq, size, max(SIZES)), device="cuda")
out_i = torch.empty((nq, size, max(SIZES)), dtype=torch.int64, device="cuda")
n_buckets = torch.empty((nq,), dtype=torch.int64, device="cuda")
total = torch.empty((nq,), dtype=torch.int64, device="cuda")
status = torch.empty((1,), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
lines = []

for n_groups in (100, 10_000):
    keys = torch.from_numpy((runs % n_groups).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    for tname, thr in THRESHOLDS.items():
        def tophits(th, order="_count"):
            return lambda: idx.search_counts_hits_by_keys_device(q.data_ptr(), nq, thr.data_ptr(), size, keys.data_ptr(), n, n_groups, th,
                                                                 out_g.data_ptr(), out_c.data_ptr(), out_s.data_ptr(), out_i.data_ptr(),
                                                                 n_buckets.data_ptr(), total.data_ptr(), status.data_ptr(), order_by=order)

        agg = lambda: idx.search_counts_by_keys_device(q.data_ptr(), nq, thr.data_ptr(), size, keys.data_ptr(), n, n_groups, out_g.data_ptr(),
                                                       out_c.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), n_buckets.data_ptr(),
                                                       total.data_ptr(), status.data_ptr())

        def hits(gs):
            return lambda: idx.search_group_hits_device(q.data_ptr(), nq, size, keys.data_ptr(), n, n_groups, gs, out_s.data_ptr(),
                                                        out_i.data_ptr(), out_g.data_ptr(), total.data_ptr(), status.data_ptr())

        def both(gs):
            one, two = agg, hits(gs)
            return lambda: (one(), two())

        a_ms, c_ms, d_ms = ({th: [] for th in SIZES} for _ in range(3))
        b_ms, score3_ms = [], []
        for _ in range(rounds):             # every variant alternates inside one process on one index
            for th in SIZES:
                a_ms[th].append(timed(tophits(th), iters))
                c_ms[th].append(timed(hits(th), iters))
                d_ms[th].append(timed(both(th), iters))
            score3_ms.append(timed(tophits(3, "max_score"), iters))
            b_ms.append(timed(agg, iters))
        med = lambda v: float(np.median(v[1:]))
        scan = {}
        for th in SIZES:
            eng.kernel_timing_begin(8)
            tophits(th)()
            eng.synchronize()
            scan[th] = eng.kernel_timing_end()[0]
            assert int(status.item()) == 0
        hit_mean = float(total.double().mean().item())
        b = med(b_ms)
        line = {"rows": n, "dim": dim, "nq": nq, "size": size, "n_groups": n_groups, "threshold": tname, "hits_per_query": round(hit_mean, 1),
                "iters": iters, "rounds_kept": rounds - 1, "b_aggregate_keys_group_ms": round(b, 4),
                "b_rounds_ms": [round(v, 4) for v in b_ms[1:]], "a3_by_score_ms": round(med(score3_ms), 4)}
        for th in SIZES:
            a, c, d = med(a_ms[th]), med(c_ms[th]), med(d_ms[th])
            line["a%d_top_hits_group_ms" % th] = round(a, 4)
            line["a%d_rounds_ms" % th] = [round(v, 4) for v in a_ms[th][1:]]
            line["a%d_scan_kernel_ms" % th] = round(scan[th], 4)
            line["c%d_group_hits_group_ms" % th] = round(c, 4)
            line["d%d_two_calls_ms" % th] = round(d, 4)
            line["a%d_over_b" % th] = round(a / b, 3)
            line["a%d_over_c" % th] = round(a / c, 3)
            line["a%d_over_two_calls" % th] = round(a / d, 3)
        print(json.dumps(line), flush=True)
        lines.append(line)

eng.drop_index("probe")
eng.close()
if out_path:
    with open(out_path, "w", encoding="utf-8") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
