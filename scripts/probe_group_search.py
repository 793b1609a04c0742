"""What a grouped (collapsed) search costs next to the top-k searches it replaces: 1 M x 1024 fp32 rows, 32 queries.

Rows are dealt to patients in runs of 32 adjacent rows (one document's chunks).  Per setting of n_groups (about 100, 10 000
and 1 000 000 — there the bound is 1 000 000 and the 31 250 runs are one patient each — and, last, every row its own group),
in one process on one index of the same rows:
  (a) the grouped launch group (rass_index_search_grouped_device, k = 10), hipEvents on the engine stream;
      its scan kernel alone (the engine's kernel timing), and the rest of the group: normalise + memset + select.  A torch
      fill of as many bytes as the table, timed the same way, says how much of that rest is the memset;
  (b) a plain k = 10 launch group (rass_index_search_device) on the same index, the same way, interleaved with (a);
  (c) rass_index_search_ex(k = 4096), the host workaround the grouped search replaces (wall clock, round trips included).
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
settings = [("100", runs % 100, 100), ("10000", runs % 10_000, 10_000), ("1000000 (bound; one patient per run)", runs, 1_000_000),
            ("every row its own group", np.arange(n), max(n, 1))]
out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
out_g = torch.empty((nq, k), dtype=torch.int32, device="cuda")
total = torch.empty((nq,), dtype=torch.int64, device="cuda")
status = torch.empty((1,), dtype=torch.int32, device="cuda")

for name, keys, n_groups in settings:
    idx = build("probe", keys)
    grouped = lambda: idx.search_grouped_device(q.data_ptr(), nq, k, PMASK, n_groups, out_s.data_ptr(), out_i.data_ptr(),
                                                out_g.data_ptr(), total.data_ptr(), status.data_ptr())
    topk = lambda: idx.search_device(q.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr())
    g_ms, t_ms = [], []
    for _ in range(rounds):                 # (a) and (b) alternate: the ratio is taken inside one process on one index
        g_ms.append(timed(grouped, iters))
        t_ms.append(timed(topk, iters))
    eng.kernel_timing_begin(8)
    grouped()
    eng.synchronize()
    scan_ms, launches = eng.kernel_timing_end()
    assert int(status.item()) == 0
    table = torch.empty((nq * n_groups,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        table.zero_()
    e0.record()
    for _ in range(iters):
        table.zero_()
    e1.record()
    torch.cuda.synchronize()
    fill_ms = e0.elapsed_time(e1) / iters
    del table
    idx.search(q_host, 4096)
    t0 = time.perf_counter()
    idx.search(q_host, 4096)
    ex_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    idx.search_grouped(q_host, k, PMASK, n_groups)
    host_ms = (time.perf_counter() - t0) * 1e3
    a, b = float(np.median(g_ms)), float(np.median(t_ms))
    print(json.dumps({
        "rows": n, "dim": dim, "nq": nq, "k": k, "n_groups": name, "mean_group_total": float(total.double().mean().item()),
        "a_grouped_group_ms": round(a, 4), "a_rounds_ms": [round(v, 4) for v in g_ms],
        "a_scan_kernel_ms": round(scan_ms, 4), "a_scan_launches": launches,
        "a_rest_normalise_memset_select_ms": round(a - scan_ms, 4), "table_bytes": nq * n_groups * 8,
        "torch_fill_of_table_bytes_ms": round(fill_ms, 4),
        "b_topk10_group_ms": round(b, 4), "b_rounds_ms": [round(v, 4) for v in t_ms],
        "c_search_ex_k4096_host_ms": round(ex_ms, 3), "grouped_host_call_ms": round(host_ms, 3),
        "a_over_b": round(a / b, 3), "c_over_a": round(ex_ms / a, 2),
    }), flush=True)
    eng.drop_index("probe")
eng.close()
