"""What grouping by a key column costs next to grouping by the tag: 1 M x 1024 fp32 rows, 32 queries, k = size = 10.

Rows are dealt to groups in runs of 32 adjacent rows (one document's chunks); the group is in the tag's patient field AND in
attribute column 0 (group + 1: a keyword code), so the tag-keyed and the key-column forms see identical groups.  Per n_groups
(100 and 10 000), in one process on one index, alternating, hipEvents on the engine stream:
  (a) the tag-keyed grouped launch group (rass_index_search_grouped_device) and aggregate launch group
      (rass_index_aggregate_device, min_score = -inf: every row a hit): the baseline;
  (b) the key-column forms over the same groups (keys = column 0 - 1 by rass_index_keys_from_attr);
  (c) (b) with a shared bitmap, all bits set and 10 % of them set: the whole slab is streamed by design, recorded only;
  (d) the two key builders (value - base; 1 025 edges) and attr_minmax alone.
Medians of ROUNDS rounds of ITERS calls each, the rounds themselves listed (the run-to-run spread (b) is judged against).  One
JSON line per n_groups.  N=<rows> / ITERS=<n> in the environment shrink it.
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
thr = torch.full((nq,), float("-inf"), device="cuda")
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


def build(name, groups):
    """An index of n seeded rows (generated on the device, 65 536 at a time): tag = group, column 0 = group + 1."""
    idx = eng.open_index(name, n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    tags = torch.from_numpy(groups.astype(np.int32)).cuda()
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), m, tags[r0:r0 + m].data_ptr(), normalize=True)
        eng.synchronize()
    idx.set_attr(0, 0, groups.astype(np.int64) + 1)
    return idx


out_g = torch.empty((nq, k), dtype=torch.int32, device="cuda")
out_c = torch.empty((nq, k), dtype=torch.int64, device="cuda")
out_s = torch.empty((nq, k), device="cuda")
out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
n_buckets = torch.empty((nq,), dtype=torch.int64, device="cuda")
total = torch.empty((nq,), dtype=torch.int64, device="cuda")
status = torch.empty((1,), dtype=torch.int32, device="cuda")
P = lambda t: t.data_ptr()

for n_groups in (100, 10_000):
    groups = (np.arange(n) // 32) % n_groups
    idx = build("probe", groups)
    keys = idx.group_keys_from_attr(0, base=1)
    words = (n + 31) // 32
    all_set = torch.full((words,), -1, dtype=torch.int32, device="cuda")
    tenth = torch.from_numpy((np.random.default_rng(8).random((words, 32)) < 0.1).astype(np.uint64)
                             .dot(np.uint64(1) << np.arange(32, dtype=np.uint64)).astype(np.uint32).view(np.int32)).cuda()
    edges = np.arange(0, 1025, dtype=np.int64) * max(1, (n_groups + 1023) // 1024)
    torch.cuda.synchronize()

    def grouped_keys(allow=None):
        return lambda: idx.search_grouped_by_keys_device(P(q), nq, k, P(keys), keys.shape[0], n_groups, P(out_s), P(out_i), P(out_g),
                                                         P(total), P(status), d_allow_ptr=0 if allow is None else P(allow),
                                                         n_bitmaps=0 if allow is None else 1, words_per_bitmap=0 if allow is None else words)

    def counts_keys(allow=None):
        return lambda: idx.search_counts_by_keys_device(P(q), nq, P(thr), k, P(keys), keys.shape[0], n_groups, P(out_g), P(out_c),
                                                        P(out_s), P(out_i), P(n_buckets), P(total), P(status),
                                                        d_allow_ptr=0 if allow is None else P(allow),
                                                        n_bitmaps=0 if allow is None else 1, words_per_bitmap=0 if allow is None else words)

    legs = {
        "a_grouped_tag": lambda: idx.search_grouped_device(P(q), nq, k, PMASK, n_groups, P(out_s), P(out_i), P(out_g), P(total), P(status)),
        "b_grouped_keys": grouped_keys(),
        "c_grouped_keys_all_set": grouped_keys(all_set),
        "c_grouped_keys_tenth_set": grouped_keys(tenth),
        "a_aggregate_tag": lambda: idx.search_counts_device(P(q), nq, P(thr), k, PMASK, n_groups, P(out_g), P(out_c), P(out_s), P(out_i),
                                                            P(n_buckets), P(total), P(status)),
        "b_aggregate_keys": counts_keys(),
        "c_aggregate_keys_all_set": counts_keys(all_set),
        "c_aggregate_keys_tenth_set": counts_keys(tenth),
        "d_keys_from_attr": lambda: idx._L.rass_index_keys_from_attr(idx._h, 0, 1, -1, P(keys), keys.shape[0]),
    }
    ms = {name: [] for name in legs}
    for _ in range(rounds):                 # every leg in every round: the ratios are taken inside one process on one index
        for name, fn in legs.items():
            ms[name].append(timed(fn, iters))
    assert int(status.item()) == 0
    # the two builders that synchronise: wall clock of whole calls
    import time
    host = {}
    for name, fn in (("d_keys_from_attr_edges_1025", lambda: idx.group_keys_from_attr(0, edges=edges)), ("d_attr_minmax", lambda: idx.attr_minmax(0))):
        fn()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        host[name + "_call_ms"] = round((time.perf_counter() - t0) * 1e3 / iters, 4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    spread = lambda name: round((max(ms[name]) - min(ms[name])) / med[name], 4)
    line = {"rows": n, "dim": dim, "nq": nq, "k": k, "n_groups": n_groups, "iters": iters}
    for name in legs:
        line[name + "_ms"] = round(med[name], 4)
        line[name + "_rounds_ms"] = [round(v, 4) for v in ms[name]]
    line.update(host)
    line.update({"b_over_a_grouped": round(med["b_grouped_keys"] / med["a_grouped_tag"], 4), "a_grouped_spread": spread("a_grouped_tag"),
                 "b_over_a_aggregate": round(med["b_aggregate_keys"] / med["a_aggregate_tag"], 4),
                 "a_aggregate_spread": spread("a_aggregate_tag")})
    print(json.dumps(line), flush=True)
    eng.drop_index("probe")
eng.close()
