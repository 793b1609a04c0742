"""What a predicate over attribute columns costs: 1 M x 1024 fp32 rows, 32 queries, eight int32 columns.

In one process on one index, interleaved over three rounds:
  builder   rass_index_allow_from_attr_clauses with 1, 4 and 8 columns named (one range clause per column per query), as 32
            per-query bitmaps and as one shared bitmap, host wall clock per call (the call uploads its clauses and waits for
            the stream), next to allow_from_tag_values on the same index and to the bytes the kernel must move:
            rows x 4 x (1 + columns) + bitmaps x rows / 8, reported as a share of 8 TB/s;
  search    search_allowed_device (k = 10) behind a shared predicate on column 0 that matches 1 %, 10 %, 50 % and 100 % of the
            rows, hipEvents on the engine stream, next to the plain k = 10 launch group; and builder + search together.
Column 0 is uniform on 0 .. 999 per row, so consecutive rows differ and a selective predicate still touches most 32-row tiles:
the honest case for a filter that is not correlated with the row order.
One JSON line, printed and — at the full size — written to profiles/probe_attr_filter_1M_B32.json.  N=<rows> / ITERS=<n> in
the environment shrink it (print only).
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
HBM_BYTES_PER_S = 8.0e12
eng = Engine(0, dim)
rng = np.random.default_rng(11)
q = torch.from_numpy(rng.standard_normal((nq, dim), dtype=np.float32)).cuda()
timer = HipTimer()

idx = eng.open_index("probe", n)
gen = torch.Generator(device="cuda")
gen.manual_seed(4321)
tags = torch.from_numpy(((np.arange(n) // 32) % 2000 + 1).astype(np.int32)).cuda()
for r0 in range(0, n, 65536):
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, tags[r0:r0 + m].data_ptr(), normalize=True)
    eng.synchronize()
for c in range(8):
    idx.set_attr(c, 0, rng.integers(0, 1000, size=n).astype(np.int32))
words = idx.allow_words


def wall_ms(fn, reps):
    for _ in range(3):
        fn()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    eng.synchronize()
    timer.start(eng.stream)
    for _ in range(reps):
        fn()
    timer.stop(eng.stream)
    eng.synchronize()
    return timer.elapsed_ms() / reps


per_query = torch.empty((nq, words), dtype=torch.int32, device="cuda")
shared = torch.empty((words,), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()


def clauses(ncols, queries, hi=499):
    return np.array([(qq, c, 0, hi, 0) for qq in range(queries) for c in range(ncols)], dtype=np.int64)


cases = {}
for ncols in (1, 4, 8):
    cq, cs = clauses(ncols, nq), clauses(ncols, 1)
    cases[f"builder_{ncols}col_per_query"] = (lambda cq=cq: idx.allow_from_attr_clauses(cq, nq=nq, allow=per_query), wall_ms)
    cases[f"builder_{ncols}col_shared"] = (lambda cs=cs: idx.allow_from_attr_clauses(cs, nq=nq, shared=True, allow=shared), wall_ms)
cases["tag_values_one_patient"] = (lambda: idx.allow_from_tag_values(np.array([777], dtype=np.int32), PMASK), wall_ms)

out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
selective = {}
for pct in (1, 10, 50, 100):
    sel = idx.allow_from_attr_clauses(clauses(1, 1, hi=10 * pct - 1), nq=nq, shared=True)
    selective[pct] = sel
    cases[f"search_allowed_{pct}pct"] = (lambda sel=sel: idx.search_allowed_device(q.data_ptr(), nq, k, sel.data_ptr(), 1, int(sel.shape[0]),
                                                                                  out_s.data_ptr(), out_i.data_ptr()), event_ms)

    def both(pct=pct):
        b = idx.allow_from_attr_clauses(clauses(1, 1, hi=10 * pct - 1), nq=nq, shared=True, allow=shared)
        idx.search_allowed_device(q.data_ptr(), nq, k, b.data_ptr(), 1, words, out_s.data_ptr(), out_i.data_ptr())
    cases[f"builder_plus_search_{pct}pct"] = (both, wall_ms)
cases["plain_k10"] = (lambda: idx.search_device(q.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr()), event_ms)
cases["plain_k10_wall"] = (cases["plain_k10"][0], wall_ms)

ms = {name: [] for name in cases}
for _ in range(rounds):                     # interleaved: every ratio is taken inside one process on one index
    for name, (fn, how) in cases.items():
        ms[name].append(how(fn, iters))
med = {name: float(np.median(v)) for name, v in ms.items()}

# the 100 % predicate answers as the plain search does
cases["plain_k10"][0]()
eng.synchronize()
a_s, a_i = out_s.clone(), out_i.clone()
cases["search_allowed_100pct"][0]()
eng.synchronize()
assert torch.equal(a_s, out_s) and torch.equal(a_i, out_i)

result = {"rows": n, "dim": dim, "nq": nq, "k": k, "tiles": words}
for name in cases:
    result[name + "_ms"] = round(med[name], 4)
    result[name + "_rounds_ms"] = [round(v, 4) for v in ms[name]]
for ncols in (1, 4, 8):
    for form, bitmaps in (("per_query", nq), ("shared", 1)):
        must_move = n * 4 * (1 + ncols) + bitmaps * n // 8
        name = f"builder_{ncols}col_{form}"
        result[name + "_bytes"] = must_move
        result[name + "_share_of_hbm"] = round(must_move / HBM_BYTES_PER_S * 1e3 / med[name + "_ms"], 4)
for pct in (1, 10, 50, 100):
    result[f"tiles_touched_{pct}pct"] = len(idx.allow_plan(selective[pct], nq)[0])
    result[f"search_allowed_{pct}pct_over_plain"] = round(med[f"search_allowed_{pct}pct_ms"] / med["plain_k10_ms"], 3)
    result[f"builder_plus_search_{pct}pct_over_plain_wall"] = round(med[f"builder_plus_search_{pct}pct_ms"] / med["plain_k10_wall_ms"], 3)
result["builder_1col_shared_over_search_10pct"] = round(med["builder_1col_shared_ms"] / med["search_allowed_10pct_ms"], 3)
print(json.dumps(result), flush=True)
if n == 1_000_000 and nq == 32:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "probe_attr_filter_1M_B32.json"), "w", encoding="utf-8") as fh:
        fh.write(json.dumps(result) + "\n")
eng.close()
