"""What a function-score search costs next to the boosted search it is modelled on: 1 M x 1024 fp32 rows, 32 queries, k = 10.

In one process on one index, interleaved round by round (the ratios are taken inside one run), hipEvents on the engine stream
around whole launch groups (normalise + scan + merge + store):
  boosted                  rass_index_search_boosted_device, one bonus column per query: the yardstick (same bytes, same loads);
  scored_<mode>            rass_index_search_scored_device on the same block in each combine mode, no gate;
  scored_<mode>_gated      the same with a per-query min_score that about half the rows pass.
One round over all thirteen cases is run and thrown away (warm-up: code objects, clocks); then every case is timed `rounds`
times, ITERS launch groups each (200 by default: a window of about 0.15 s); the median and the spread (min .. max) of the
rounds are reported, and each scored case's median over the boosted median.  The boosted case's own spread is the noise to
read the ratios against.  No per-kernel figure is taken: a single launch timed on its own, after an idle gap, measured the
clock ramp more than the kernel (0.70 .. 0.94 ms for kernels inside 0.72 ms groups), so the field was dropped.
Then the column builder, wall clock of the host call (each ends in a stream sync): fn_from_attr with 1, 4 and 16 functions per
query for 32 queries (a mix of gauss / exp / linear decay, field_value_factor and filtered weights), and 4 functions into one
shared column.
One JSON line.  N=<rows> / ITERS=<n> / ROUNDS=<n> in the environment shrink it.
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
iters = int(os.environ.get("ITERS", 200))
rounds = int(os.environ.get("ROUNDS", 5))
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
for r0 in range(0, n, 65536):
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, 0, normalize=True)
    eng.synchronize()
idx.set_attr(0, 0, rng.integers(19000, 19800, size=n).astype(np.int32))      # a date, as days
idx.set_attr(1, 0, rng.integers(0, 1000, size=n).astype(np.int32))
idx.set_attr(2, 0, rng.integers(-50, 50, size=n).astype(np.int32))

out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
block = idx.new_bonus(nq)
block.copy_(torch.randn(block.shape, generator=gen, device="cuda") * 0.05 + 1.0)
boost = torch.from_numpy(rng.uniform(0.5, 2.0, size=nq).astype(np.float32)).cuda()
gate = torch.zeros((nq,), dtype=torch.float32, device="cuda")          # cos >= 0: about half of random rows
stride = int(block.shape[1])
torch.cuda.synchronize()

MODES = ("sum", "multiply", "avg", "max", "min", "replace")
cases = {"boosted": lambda: idx.search_boosted_device(q.data_ptr(), nq, k, block.data_ptr(), nq, n, stride, out_s.data_ptr(),
                                                      out_i.data_ptr(), d_boost_ptr=boost.data_ptr())}
for mode in MODES:
    for gated in (False, True):
        cases[f"scored_{mode}" + ("_gated" if gated else "")] = (
            lambda mode=mode, gated=gated: idx.search_scored_device(q.data_ptr(), nq, k, block.data_ptr(), nq, n, stride, out_s.data_ptr(),
                                                                    out_i.data_ptr(), d_boost_ptr=boost.data_ptr(), combine=mode,
                                                                    d_min_score_ptr=gate.data_ptr() if gated else 0))
ms = {name: [] for name in cases}
for r in range(rounds + 1):
    for name, fn in cases.items():
        took = timed(fn, iters)
        if r > 0:               # round 0 is warm-up for every case alike
            ms[name].append(took)
med = {name: float(np.median(v)) for name, v in ms.items()}

FNS = [
    {"kind": "gauss", "col": 0, "origin": 19700.0, "scale": 90.0, "offset": 7.0, "decay": 0.5},
    {"kind": "field_value_factor", "col": 1, "factor": 0.01, "modifier": "log1p", "missing": 1.0},
    {"kind": "weight", "weight": 2.0, "filter": 0},
    {"kind": "linear", "col": 2, "origin": 0.0, "scale": 20.0, "offset": 0.0, "decay": 0.5},
    {"kind": "exp", "col": 0, "origin": 19800.0, "scale": 365.0, "offset": 0.0, "decay": 0.5, "filter": 1},
    {"kind": "field_value_factor", "col": 1, "factor": 1.0, "modifier": "sqrt"},
]
filters = torch.randint(-(1 << 31), (1 << 31) - 1, (2, idx.allow_words + idx.ALLOW_SLACK_WORDS), dtype=torch.int64, device="cuda").to(torch.int32)
torch.cuda.synchronize()
builders = {}


def time_builder(target, fns):
    idx.fn_from_attr(target, fns, score_mode="multiply", filters=filters)      # warm-up
    took = []
    for _ in range(5):
        t0 = time.perf_counter()
        idx.fn_from_attr(target, fns, score_mode="multiply", filters=filters)
        took.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(took)), 3)


for per_q in (1, 4, 16):
    fns = [dict(FNS[j % len(FNS)], query=qq) for qq in range(nq) for j in range(per_q)]
    builders[f"fn_{per_q}_per_query_x32_ms"] = time_builder(idx.new_bonus(nq), fns)
builders["fn_4_shared_ms"] = time_builder(idx.new_bonus(), [dict(FNS[j]) for j in range(4)])

print(json.dumps({
    "rows": n, "dim": dim, "nq": nq, "k": k, "iters": iters, "rounds": rounds, "warmup_rounds_discarded": 1,
    "group_ms": {name: round(v, 4) for name, v in med.items()},
    "group_spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in ms.items()},
    "group_rounds_ms": {name: [round(x, 4) for x in v] for name, v in ms.items()},
    "over_boosted": {name: round(v / med["boosted"], 3) for name, v in med.items() if name != "boosted"},
    "boosted_spread_rel": round((max(ms["boosted"]) - min(ms["boosted"])) / med["boosted"], 3),
    "column_bytes_per_query_block": nq * stride * 4,
    "builders": builders,
}), flush=True)
eng.drop_index("probe")
eng.close()
