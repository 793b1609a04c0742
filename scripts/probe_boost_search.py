"""What a boosted search costs next to the scans it sits beside: 1 M x 1024 fp32 rows, 32 queries, k = 10.

In one process on one index, interleaved (the ratios are taken inside one run), hipEvents on the engine stream around
whole launch groups (normalise + scan + merge + store), and the scan kernel alone from the engine's kernel timing:
  (a) the plain top-k launch group (rass_index_search_device): sample floor and all;
  (b) rass_index_search_allowed_device under an all-ones bitmap: the closest existing scan WITHOUT a sample floor — the
      yardstick, since the boosted scan has none either;
  (c) rass_index_search_boosted_device with one bonus column per query (32 x 4 B more per 4 096-B row: 3 %);
  (d) the same with ONE column shared by the 32 queries;
  (e) (c) under the opensearch transform with per-query boosts (a division per ranked (row, query)).
Then the column builders, wall clock of the host call (each ends in a stream sync): bonus_from_attr_clauses with 1, 8 and
64 clauses per query for 32 queries (replace), bonus_mask from 32 bitmaps, bonus_scatter of 1 000 text hits per query.
One JSON line.  N=<rows> / ITERS=<n> in the environment shrink it.
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


def kernel_ms(fn):
    eng.kernel_timing_begin(8)
    fn()
    eng.synchronize()
    return eng.kernel_timing_end()


idx = eng.open_index("probe", n)
gen = torch.Generator(device="cuda")
gen.manual_seed(1234)
for r0 in range(0, n, 65536):
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, 0, normalize=True)
    eng.synchronize()
for c in range(3):          # three attribute columns for the clause builder
    idx.set_attr(c, 0, rng.integers(0, 1000, size=n).astype(np.int32))

out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
ones = torch.full((idx.allow_words + idx.ALLOW_SLACK_WORDS,), -1, dtype=torch.int32, device="cuda")
per_query = idx.new_bonus(nq)
per_query.copy_(torch.randn(per_query.shape, generator=gen, device="cuda") * 0.05)
shared = per_query[0].clone()
boost = torch.from_numpy(rng.uniform(0.5, 2.0, size=nq).astype(np.float32)).cuda()
stride = int(per_query.shape[1])
torch.cuda.synchronize()

cases = {
    "a_topk": lambda: idx.search_device(q.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr()),
    "b_allowed_all_ones": lambda: idx.search_allowed_device(q.data_ptr(), nq, k, ones.data_ptr(), 1, int(ones.shape[0]), out_s.data_ptr(),
                                                            out_i.data_ptr()),
    "c_boosted_per_query": lambda: idx.search_boosted_device(q.data_ptr(), nq, k, per_query.data_ptr(), nq, n, stride, out_s.data_ptr(),
                                                             out_i.data_ptr()),
    "d_boosted_shared": lambda: idx.search_boosted_device(q.data_ptr(), nq, k, shared.data_ptr(), 1, n, stride, out_s.data_ptr(),
                                                          out_i.data_ptr()),
    "e_boosted_per_query_opensearch": lambda: idx.search_boosted_device(q.data_ptr(), nq, k, per_query.data_ptr(), nq, n, stride,
                                                                        out_s.data_ptr(), out_i.data_ptr(), d_boost_ptr=boost.data_ptr(),
                                                                        transform="opensearch"),
}
ms = {name: [] for name in cases}
for _ in range(rounds):
    for name, fn in cases.items():
        ms[name].append(timed(fn, iters))
med = {name: float(np.median(v)) for name, v in ms.items()}
kern = {name: kernel_ms(fn) for name, fn in cases.items()}

builders = {}
for per_q in (1, 8, 64):
    clauses = np.array([(qq, j % 3, 10 * j, 10 * j + 400, j % 2) for qq in range(nq) for j in range(per_q)], dtype=np.int64)
    weights = rng.standard_normal(len(clauses)).astype(np.float32)
    target = idx.new_bonus(nq)
    idx.bonus_from_attr_clauses(target, clauses, weights)      # warm-up
    best = []
    for _ in range(5):
        t0 = time.perf_counter()
        idx.bonus_from_attr_clauses(target, clauses, weights)
        best.append((time.perf_counter() - t0) * 1e3)
    builders[f"clauses_{per_q}_per_query_x32_ms"] = round(float(np.median(best)), 3)
bitmaps = torch.randint(-(1 << 31), (1 << 31) - 1, (nq, int(ones.shape[0])), dtype=torch.int64, device="cuda").to(torch.int32)
target = idx.new_bonus(nq)
best = []
for _ in range(6):
    t0 = time.perf_counter()
    idx.bonus_mask(target, bitmaps)
    eng.synchronize()
    best.append((time.perf_counter() - t0) * 1e3)
builders["mask_x32_ms"] = round(float(np.median(best[1:])), 3)
hits = 1000
q_of = np.repeat(np.arange(nq, dtype=np.int32), hits)
rows = np.concatenate([rng.choice(n, size=hits, replace=False) for _ in range(nq)]).astype(np.int64)
vals = rng.random(len(rows)).astype(np.float32)
best = []
for _ in range(6):
    t0 = time.perf_counter()
    idx.bonus_scatter(target, q_of, rows, vals)
    best.append((time.perf_counter() - t0) * 1e3)
builders["scatter_1000_hits_x32_ms"] = round(float(np.median(best[1:])), 3)

print(json.dumps({
    "rows": n, "dim": dim, "nq": nq, "k": k, "iters": iters, "rounds": rounds,
    "group_ms": {name: round(v, 4) for name, v in med.items()},
    "group_rounds_ms": {name: [round(x, 4) for x in v] for name, v in ms.items()},
    "scan_kernel_ms": {name: round(v[0], 4) for name, v in kern.items()},
    "scan_launches": {name: v[1] for name, v in kern.items()},
    "per_query_over_allowed": round(med["c_boosted_per_query"] / med["b_allowed_all_ones"], 3),
    "shared_over_allowed": round(med["d_boosted_shared"] / med["b_allowed_all_ones"], 3),
    "opensearch_over_allowed": round(med["e_boosted_per_query_opensearch"] / med["b_allowed_all_ones"], 3),
    "per_query_over_topk": round(med["c_boosted_per_query"] / med["a_topk"], 3),
    "allowed_over_topk": round(med["b_allowed_all_ones"] / med["a_topk"], 3),
    "bonus_bytes_per_query_column_block": nq * stride * 4,
    "builders": builders,
}), flush=True)
eng.drop_index("probe")
eng.close()
