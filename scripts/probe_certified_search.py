"""Probe: the certified int8 search (prefilter mode 3, "int8_exact") against the exact fp32 scan (mode 0) IN THE SAME RUN,
1 024-query steps through rass_index_search_device_batch, timed with hipEvents on the engine's stream.

Corpora: bench.py's (1 M x 1024 Philox rows, seed 1234; queries torch.randn seed 4321), a sigma = 2 clustered corpus (1 000
centres), and an adversarial one (one row with a huge outlier component: R is large, every query falls back) that prices the
fallback.  Every mode-3 answer is also compared with mode 0's, ids and scores bit for bit.  Prints one JSON object (and writes it
to --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rassengine_amd.engine import Engine, HipTimer  # noqa: E402

HBM_BYTES_PER_S = 8.0e12   # MI355X HBM3E peak


def fill(idx, kind, rows, dim, dev):
    if kind == "iid":
        idx.fill_synthetic(rows, seed=1234)
        return None
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centres = torch.randn((1000, dim), generator=g, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    for lo in range(0, rows, 65536):
        n = min(65536, rows - lo)
        lab = torch.randint(0, 1000, (n,), generator=g, device=dev)
        x = centres[lab] + 2.0 * torch.randn((n, dim), generator=g, device=dev) / dim ** 0.5
        if kind == "outlier" and lo == 0:
            x[77, 3] = 8.0      # the other components fall between int8 steps: rho ~ 0.1
        x = x.contiguous()
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), n)
        idx.engine.synchronize()
    return centres


def queries(kind, nq, dim, dev, centres):
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    if centres is None:
        return torch.randn((nq, dim), generator=g, device=dev).contiguous()
    lab = torch.randint(0, centres.shape[0], (nq,), generator=g, device=dev)
    return (centres[lab] + 2.0 * torch.randn((nq, dim), generator=g, device=dev) / dim ** 0.5).contiguous()


def run(idx, q, k, steps, warmup):
    nq = q.shape[0]
    s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    torch.cuda.synchronize()
    for _ in range(warmup):
        idx.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr())
    idx.engine.synchronize()
    t = HipTimer()
    t.start(idx.engine.stream)
    for _ in range(steps):
        idx.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr())
    t.stop(idx.engine.stream)
    idx.engine.synchronize()
    ms = t.elapsed_ms() / steps
    return ms, s.cpu().numpy(), i.cpu().numpy()


def leg(eng, kind, rows, dim, nq, k, steps, warmup, dev):
    idx = eng.open_index(f"probe-{kind}", capacity_rows=rows)
    centres = fill(idx, kind, rows, dim, dev)
    q = queries(kind, nq, dim, dev, centres)
    idx.set_prefilter("off")
    ms0, s0, i0 = run(idx, q, k, steps, warmup)
    idx.set_prefilter("int8_exact")
    ms3, s3, i3 = run(idx, q, k, steps, warmup)
    st = idx.certify_stats()
    calls = steps + warmup
    stride_i8 = (idx.row_stride + 511) // 512 * 512
    passes = -(-nq // 16)
    i8_bytes = passes * rows * stride_i8 + nq * 128 * idx.row_stride * 4    # candidate scan + the re-rank's fp32 rows
    out = {
        "corpus": kind, "rows": rows, "dim": dim, "nq_per_step": nq, "k": k, "steps": steps,
        "exact_ms_per_step": round(ms0, 3), "int8_exact_ms_per_step": round(ms3, 3),
        "exact_qps": round(nq / ms0 * 1e3, 1), "int8_exact_qps": round(nq / ms3 * 1e3, 1),
        "speedup": round(ms0 / ms3, 3),
        "certified_fraction": round(st["certified"] / max(st["queries"], 1), 4),
        "fallbacks_per_step": st["fallbacks"] / calls, "R": st["R"], "V": st["V"],
        "int8_plus_rerank_bytes_per_step": i8_bytes,
        "hbm_fraction_int8_plus_rerank": round(i8_bytes / (ms3 * 1e-3) / HBM_BYTES_PER_S, 3),
        "identical_to_exact": bool(np.array_equal(i0, i3) and np.array_equal(s0.view(np.uint32), s3.view(np.uint32))),
    }
    eng.drop_index(f"probe-{kind}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--side-rows", type=int, default=200_000, help="rows of the clustered and adversarial corpora")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="iid,clustered,outlier")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dim, dev = 1024, torch.device("cuda:0")
    eng = Engine(0, dim)
    res = {"probe": "certified_int8_search", "legs": []}
    try:
        for kind in a.legs.split(","):
            rows = a.rows if kind == "iid" else a.side_rows
            res["legs"].append(leg(eng, kind, rows, dim, a.nq, a.k, a.steps, a.warmup, dev))
            print(json.dumps(res["legs"][-1]), flush=True)
    finally:
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
