"""What an allow-list search costs next to the searches it stands beside: 1 M x 1024 fp32 rows, 32 queries, k = 10.

Rows are dealt to 2 000 patients in runs of 32 adjacent rows (one document's chunks), so one patient owns ~500 rows in ~16
tiles.  In one process on one index, each a launch group on the device, hipEvents on the engine stream, interleaved:
  (a) the plain search (rass_index_search_device_ex);
  (b) the same with a one-patient tag filter: the whole slab is read, ~500 rows rank;
  (c) search_allowed with an all-ones bitmap: every tile is planned and scanned — the price of the mode over (a) (the plan,
      two scalar words per ranking step, no sample floor, the store);
  (d) search_allowed with the bitmap of (b)'s patient (allow_from_tag_values): only that patient's tiles are read;
  (e) search_allowed with a 40-row bitmap (allow_from_rows; rows spread over the index).
The scan kernel's share of (c), (d), (e) comes from the engine's kernel timing.  One JSON line, printed and — at the full
size — written to profiles/probe_allow_search_1M_B32.json.  N=<rows> / ITERS=<n> in the environment shrink it (print only).
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


def scan_ms(fn):
    eng.kernel_timing_begin(8)
    fn()
    eng.synchronize()
    return eng.kernel_timing_end()


n_patients = 2000
keys = ((np.arange(n) // 32) % n_patients + 1).astype(np.int32)
idx = eng.open_index("probe", n)
gen = torch.Generator(device="cuda")
gen.manual_seed(1234)
tags = torch.from_numpy(keys).cuda()
for r0 in range(0, n, 65536):
    m = min(65536, n - r0)
    x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m, tags[r0:r0 + m].data_ptr(), normalize=True)
    eng.synchronize()

patient = 777
words = idx.allow_words
ones = torch.full((words,), -1, dtype=torch.int32, device="cuda")
of_patient = idx.allow_from_tag_values(np.array([patient], dtype=np.int32), PMASK)
forty = idx.allow_from_rows(np.linspace(0, n - 1, 40).astype(np.int64))
qf = torch.full((nq,), patient, dtype=torch.int32, device="cuda")
out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
eng.synchronize()


def allowed(bitmap):
    return lambda: idx.search_allowed_device(q.data_ptr(), nq, k, bitmap.data_ptr(), 1, words, out_s.data_ptr(), out_i.data_ptr())


cases = {
    "a_plain": lambda: idx.search_device(q.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr()),
    "b_tag_filter": lambda: idx.search_device(q.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr(), d_q_filter_ptr=qf.data_ptr()),
    "c_allowed_all_ones": allowed(ones),
    "d_allowed_one_patient": allowed(of_patient),
    "e_allowed_40_rows": allowed(forty),
}
ms = {name: [] for name in cases}
for _ in range(rounds):                     # interleaved: every ratio is taken inside one process on one index
    for name, fn in cases.items():
        ms[name].append(timed(fn, iters))
med = {name: float(np.median(v)) for name, v in ms.items()}

# the answers agree where they must: (c) with (a), (d) with (b)
cases["a_plain"]()
eng.synchronize()
a_s, a_i = out_s.clone(), out_i.clone()
cases["c_allowed_all_ones"]()
eng.synchronize()
assert torch.equal(a_s, out_s) and torch.equal(a_i, out_i)
cases["b_tag_filter"]()
eng.synchronize()
b_s, b_i = out_s.clone(), out_i.clone()
cases["d_allowed_one_patient"]()
eng.synchronize()
assert torch.equal(b_s, out_s) and torch.equal(b_i, out_i)

result = {"rows": n, "dim": dim, "nq": nq, "k": k, "patients": n_patients, "rows_of_the_patient": int((keys == patient).sum()),
          "tiles": words, "tiles_of_the_patient": len(idx.allow_plan(of_patient, nq)[0]), "tiles_of_40_rows": len(idx.allow_plan(forty, nq)[0])}
for name in cases:
    result[name + "_ms"] = round(med[name], 4)
    result[name + "_rounds_ms"] = [round(v, 4) for v in ms[name]]
for name in ("a_plain", "c_allowed_all_ones", "d_allowed_one_patient", "e_allowed_40_rows"):
    t, launches = scan_ms(cases[name])
    result[name + "_scan_kernel_ms"] = round(t, 4)
    result[name + "_scan_launches"] = launches
result["c_over_a"] = round(med["c_allowed_all_ones"] / med["a_plain"], 3)
result["d_over_b"] = round(med["d_allowed_one_patient"] / med["b_tag_filter"], 4)
result["e_over_a"] = round(med["e_allowed_40_rows"] / med["a_plain"], 4)
print(json.dumps(result), flush=True)
if n == 1_000_000 and nq == 32:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "probe_allow_search_1M_B32.json"), "w", encoding="utf-8") as fh:
        fh.write(json.dumps(result) + "\n")
eng.close()
