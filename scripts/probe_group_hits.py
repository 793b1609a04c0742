"""What the grouped search with inner hits costs next to the grouped search it extends: 1 M x 1024 fp32 rows, 32 queries, k = 10.

Rows are dealt to groups in runs of 32 adjacent rows (one document's chunks), at 100 and 10 000 groups.  Per setting, in one
process on one index and one key column:
  (a) the group-hits launch group (rass_index_search_group_hits_keys_device) at group_size 1, 3, 8 and 16, with and (at 3)
      without the capped list, hipEvents on the engine stream; its scan kernel alone (the engine's kernel timing);
  (b) the grouped launch group of the unchanged kernel (rass_index_search_grouped_keys_device) on the same column, the same
      way, interleaved with (a) round by round.  group_size chained group-max passes — the natural alternative — cost
      group_size x (b).
Medians over the rounds, as probe_group_search.py takes them.  One JSON line per setting, and the lines again, as a list, in
profiles/probe_group_hits_1M_B32.json (OUT=<path> moves it, OUT= skips it).  N=<rows> / ITERS=<n> in the environment shrink it.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rassengine_amd.engine import Engine, HipTimer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n, dim, nq, k = int(os.environ.get("N", 1_000_000)), 1024, 32, 10
iters = int(os.environ.get("ITERS", 30))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "probe_group_hits_1M_B32.json"))
rounds = 3
SIZES = (1, 3, 8, 16)
eng = Engine(0, dim)
rng = np.random.default_rng(7)
q = torch.from_numpy(rng.standard_normal((nq, dim), dtype=np.float32)).cuda()
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
for r0 in range(0, n, 65536):          # n seeded rows, generated on the device
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, 0, normalize=True)
    eng.synchronize()

runs = np.arange(n) // 32
out_s = torch.empty((nq, k, max(SIZES)), device="cuda")
out_i = torch.empty((nq, k, max(SIZES)), dtype=torch.int64, device="cuda")
out_g = torch.empty((nq, k), dtype=torch.int32, device="cuda")
cap_s = torch.empty((nq, k), device="cuda")
cap_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
total = torch.empty((nq,), dtype=torch.int64, device="cuda")
status = torch.empty((1,), dtype=torch.int32, device="cuda")
lines = []

for n_groups in (100, 10_000):
    keys = torch.from_numpy((runs % n_groups).astype(np.int32)).cuda()
    torch.cuda.synchronize()

    def hits(gs, capped=True):
        return lambda: idx.search_group_hits_device(q.data_ptr(), nq, k, keys.data_ptr(), n, n_groups, gs, out_s.data_ptr(),
                                                    out_i.data_ptr(), out_g.data_ptr(), total.data_ptr(), status.data_ptr(),
                                                    d_out_capped_scores_ptr=cap_s.data_ptr() if capped else 0,
                                                    d_out_capped_ids_ptr=cap_i.data_ptr() if capped else 0)

    grouped = lambda: idx.search_grouped_by_keys_device(q.data_ptr(), nq, k, keys.data_ptr(), n, n_groups, out_s.data_ptr(),
                                                        out_i.data_ptr(), out_g.data_ptr(), total.data_ptr(), status.data_ptr())
    h_ms = {gs: [] for gs in SIZES}
    g_ms, plain3_ms = [], []
    for _ in range(rounds):                 # every size and the unchanged kernel alternate inside one process on one index
        for gs in SIZES:
            h_ms[gs].append(timed(hits(gs), iters))
        plain3_ms.append(timed(hits(3, capped=False), iters))
        g_ms.append(timed(grouped, iters))
    scan = {}
    for gs in SIZES:
        eng.kernel_timing_begin(8)
        hits(gs)()
        eng.synchronize()
        scan[gs] = eng.kernel_timing_end()[0]
        assert int(status.item()) == 0
    eng.kernel_timing_begin(8)
    grouped()
    eng.synchronize()
    g_scan = eng.kernel_timing_end()[0]
    b = float(np.median(g_ms))
    line = {"rows": n, "dim": dim, "nq": nq, "k": k, "n_groups": n_groups, "rows_per_group": n // n_groups, "iters": iters, "rounds": rounds,
            "b_grouped_keys_group_ms": round(b, 4), "b_rounds_ms": [round(v, 4) for v in g_ms], "b_scan_kernel_ms": round(g_scan, 4),
            "a3_without_capped_list_ms": round(float(np.median(plain3_ms)), 4)}
    for gs in SIZES:
        a = float(np.median(h_ms[gs]))
        line["a%d_group_hits_group_ms" % gs] = round(a, 4)
        line["a%d_rounds_ms" % gs] = [round(v, 4) for v in h_ms[gs]]
        line["a%d_scan_kernel_ms" % gs] = round(scan[gs], 4)
        line["a%d_over_b" % gs] = round(a / b, 3)
        line["a%d_over_chained_passes" % gs] = round(a / (gs * b), 3)
    print(json.dumps(line), flush=True)
    lines.append(line)

eng.drop_index("probe")
eng.close()
if out_path:
    with open(out_path, "w", encoding="utf-8") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
