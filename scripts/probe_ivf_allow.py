"""Probe: a bitmap-filtered search through the IVF (rass_ivf_search_allowed_delta_device) next to the exact flat allow scan
(rass_index_search_allowed_device) it may replace, timed IN THE SAME RUN on one clustered corpus — the generator of bench.py's
`--mode ivf` (8 192 Gaussian centres + sigma-noise, normalised), 12.5 M x 1024 rows by default, IVF-4096, fp32 slab.

Per bitmap density (1 %, 10 %, 50 % of the rows, iid per query) and nprobe (2, 8), over `--groups` launch groups of 32 queries:
  flat_ms    wall clock of one group's flat allowed search (median over the groups, each the median of `--repeats` runs)
  ivf_ms     the same for the IVF form, its allocations and the stream hand-over included
  recall10   of the IVF form against the flat one (which is exact within the bitmap)
  scanned    rows the IVF form streamed per group (probe tiles kept + delta tiles planned), and `flat_rows_bound` = 32 x the
             group's summed popcounts, `probe_rows_estimate` = nprobe x covered / nlist: the two sides of IvfPolicy.allow_route
  route      what IvfPolicy.allow_route (allow_exact_factor = 1.0, from bytes alone) decides for the group
This is where a measured `allow_exact_factor` would come from: the factor at which flat_ms and ivf_ms cross.

One JSON line on stdout; --out writes it to a file too.  A full run, every step under its own time limit:

  timeout -k 10 300 python scripts/probe_ivf_allow.py --rows 1000000 --nlist 1024 --out profiles/probe_ivf_allow_1M.json && \\
  timeout -k 10 900 python scripts/probe_ivf_allow.py --out profiles/probe_ivf_allow_12.5M.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rassengine_amd.engine import Engine  # noqa: E402
from rassengine_amd.ivf import IvfIndex, IvfPolicy, train_centroids  # noqa: E402

CENTRES, SIGMA, SEED = 8192, 1.0, 7      # bench.py: IVF_CENTRES, IVF_SIGMA, IVF_SEED


def _wall_ms(eng, fn):
    eng.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    eng.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _bitmaps(rows, words, density, g, dev):
    """int32 [32, words]: one iid bitmap per query of the group; bits past `rows` clear."""
    shifts = torch.arange(32, device=dev, dtype=torch.int64)
    out = torch.empty((32, words), dtype=torch.int32, device=dev)
    for q in range(32):
        bits = torch.rand((words * 32,), generator=g, device=dev) < density
        bits[rows:] = False
        w = (bits.view(words, 32).to(torch.int64) << shifts).sum(dim=1)
        out[q] = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.01, 0.1, 0.5])
    ap.add_argument("--nprobes", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    centres = torch.randn((CENTRES, a.dim), generator=g, device=dev)
    centres = centres / centres.norm(dim=1, keepdim=True)
    eng = Engine(0, a.dim)
    out = {"probe": "ivf_allow", "rows": a.rows, "dim": a.dim, "nlist": a.nlist, "k": a.k, "groups": a.groups,
           "repeats": a.repeats, "data": f"{CENTRES} Gaussian centres (seed {SEED}) + sigma {SIGMA} noise, normalised", "cases": []}
    try:
        flat = eng.open_index("probe-ivf-allow", capacity_rows=a.rows)
        g.manual_seed(SEED + 1)
        for lo in range(0, a.rows, 262144):
            n = min(262144, a.rows - lo)
            lab = torch.randint(0, CENTRES, (n,), generator=g, device=dev)
            x = centres[lab] + SIGMA * torch.randn((n, a.dim), generator=g, device=dev) / a.dim ** 0.5
            torch.cuda.synchronize()
            flat.add_device(x.data_ptr(), n, normalize=True)
            eng.synchronize()
        del x
        t0 = time.perf_counter()
        cent = train_centroids(flat, a.nlist, train_rows=0, iters=a.iters, seed=1)
        ivf = IvfIndex.build(flat, nlist=a.nlist, centroids=cent)
        out["train_build_s"] = round(time.perf_counter() - t0, 2)
        covered = ivf.covered_rows
        out["covered"] = covered
        g.manual_seed(4321)
        nq = 32 * a.groups
        lab = torch.randint(0, CENTRES, (nq,), generator=g, device=dev)
        q = (centres[lab] + SIGMA * torch.randn((nq, a.dim), generator=g, device=dev) / a.dim ** 0.5).contiguous()
        words = flat.allow_words
        policy = IvfPolicy(nlist=a.nlist, allow_probe=True)
        s_f = torch.empty((32, a.k), dtype=torch.float32, device=dev)
        i_f = torch.empty((32, a.k), dtype=torch.int64, device=dev)
        for density in a.densities:
            maps = [_bitmaps(a.rows, words, density, g, dev) for _ in range(a.groups)]
            counts = [flat.allow_count(m) for m in maps]
            flat_ms, truth = [], []
            for grp in range(a.groups):
                qg = q[32 * grp:32 * grp + 32]

                def run_flat():
                    flat.search_allowed_device(qg.data_ptr(), 32, a.k, maps[grp].data_ptr(), 32, words, s_f.data_ptr(), i_f.data_ptr())
                run_flat()
                flat_ms.append(float(np.median([_wall_ms(eng, run_flat)[0] for _ in range(a.repeats)])))
                truth.append(i_f.cpu().numpy().copy())
            for nprobe in a.nprobes:
                ivf_ms, recall, scanned = [], [], []
                for grp in range(a.groups):
                    qg = q[32 * grp:32 * grp + 32].contiguous()

                    def run_ivf():
                        return ivf.search_allowed_delta_device(flat, qg, a.k, nprobe, maps[grp])
                    run_ivf()
                    runs = [_wall_ms(eng, run_ivf) for _ in range(a.repeats)]
                    ivf_ms.append(float(np.median([r[0] for r in runs])))
                    _, di, dn = runs[-1][1]
                    got = di.cpu().numpy()
                    recall.append(float(np.mean([len(set(x.tolist()) & set(y.tolist()) - {-1}) / max(1, int((y >= 0).sum()))
                                                 for x, y in zip(got, truth[grp])])))
                    scanned.append(int(dn.item()))
                c_max = max(int(c.sum()) for c in counts)
                out["cases"].append({
                    "density": density, "nprobe": nprobe, "flat_ms": round(float(np.median(flat_ms)), 4),
                    "ivf_ms": round(float(np.median(ivf_ms)), 4), "recall10": round(float(np.mean(recall)), 4),
                    "scanned_rows_per_group": int(np.median(scanned)), "flat_rows_bound": 32 * c_max,
                    "probe_rows_estimate": round(nprobe * covered / a.nlist, 1),
                    "route": policy.allow_route(np.concatenate(counts), nq, False, nprobe, covered, a.nlist)})
        ivf.close()
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
