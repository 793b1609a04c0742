"""Probe: the device-planned IVF build and the absorb (rass_ivf_build_device, rass_ivf_absorb) against the paths they stand
next to, all timed IN THE SAME RUN on one clustered corpus (the generator of bench.py's ivf leg: Philox centres + noise).

Default: 2 M x 1024 rows, nlist 4096, fp32 slab.  Recorded (wall clock around calls that return with their work complete;
repeat 0 warms every shape and is not reported):

  build        host-planned build (IvfIndex.build = assign_rows + rass_ivf_build_prefix) vs IvfIndex.build_device, the same
               centroids; the two saved files are compared.
  delta 5 / 25 the IVF covers rows / (1 + delta); then a full rebuild (IvfBackedIndex.build_ivf: train + assign + host build)
               vs IvfBackedIndex.absorb_delta over the same rows (the absorb first, from the
               IVF + delta; the rebuild after it: it trains, assigns and places every row whatever the IVF covered).
  search       the 1 024-query step through search_delta at nprobe 2 and 8 with the delta unabsorbed (the parent commit's
               path) and after the absorb.
  recall       recall@10 against the flat scan, after absorbing 25 %, of the absorbed IVF and of a retrained one.

Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rassengine_amd.engine import Engine, FlatIndex  # noqa: E402
from rassengine_amd.ivf import IvfBackedIndex, IvfIndex, IvfPolicy, train_centroids  # noqa: E402


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _append_clustered(idx, centres, n, g, sigma, chunk=65536):
    dim = centres.shape[1]
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        lab = torch.randint(0, centres.shape[0], (m,), generator=g, device=centres.device)
        x = (centres[lab] + sigma * torch.randn((m, dim), generator=g, device=centres.device) / dim ** 0.5).contiguous()
        torch.cuda.synchronize()
        FlatIndex.add_device(idx, x.data_ptr(), m)
    idx.engine.synchronize()


def _step_ms(idx, q, k, nprobe, steps=3):
    nq = q.shape[0]
    s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    i = torch.empty((nq, k), dtype=torch.int64, device=q.device)

    def step():
        for a in range(0, nq, 32):
            idx.search_device(q[a:a + 32].data_ptr(), min(32, nq - a), k, s[a:a + 32].data_ptr(), i[a:a + 32].data_ptr(),
                              nprobe=nprobe)
    step()
    return float(np.median([_wall(step)[0] for _ in range(steps)]))


def _recall(idx, q, k, nprobe):
    qh = q.cpu().numpy()
    want = FlatIndex.search(idx, qh, k)[1]
    got = idx.search(qh, k, nprobe=nprobe)[1]
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(got, want)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--clusters", type=int, default=8192)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    centres = torch.nn.functional.normalize(torch.randn((a.clusters, a.dim), generator=g, device=dev), dim=1)
    q = (centres[torch.randint(0, a.clusters, (1024,), generator=g, device=dev)] +
         0.7 * torch.randn((1024, a.dim), generator=g, device=dev) / a.dim ** 0.5).contiguous()
    eng = Engine(0, a.dim)
    out = {"probe": "ivf_absorb", "rows": a.rows, "dim": a.dim, "nlist": a.nlist, "clusters": a.clusters, "sigma": a.sigma,
           "repeats": a.repeats, "build": {}, "delta": {}}
    tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"probe_ivf_absorb_{os.getpid()}")
    try:
        policy = IvfPolicy(nlist=a.nlist, nprobe=8, min_rows=1 << 62, iters=a.iters)      # nothing happens by itself
        for share in (5, 25):
            covered = int(a.rows / (1 + share / 100.0)) // 32 * 32
            rec = {k: [] for k in ("rebuild_ms", "absorb_ms")}
            for rep in range(a.repeats + 1):
                name = f"probe-absorb-{share}-{rep}"
                idx = IvfBackedIndex(eng.open_index(name, capacity_rows=a.rows), policy)
                _append_clustered(idx, centres, covered, g, a.sigma)
                cent = train_centroids(idx, a.nlist, 0, a.iters, 0)
                if share == 5 and not out["build"]:
                    host, dev_b = [], []
                    for r in range(a.repeats + 1):
                        th, ih = _wall(lambda: IvfIndex.build(idx, nlist=a.nlist, centroids=cent))
                        td, idv = _wall(lambda: IvfIndex.build_device(idx, cent))
                        if r == 0:
                            ih.save(tmp + ".h")
                            idv.save(tmp + ".d")
                            same = open(tmp + ".h", "rb").read() == open(tmp + ".d", "rb").read()
                            os.remove(tmp + ".h")
                            os.remove(tmp + ".d")
                        else:
                            host.append(round(th, 2))
                            dev_b.append(round(td, 2))
                        ih.close()
                        idv.close()
                    out["build"] = {"rows": covered, "host_planned_ms": host, "build_device_ms": dev_b, "same_file": same}
                idx.build_ivf(centroids=cent)
                _append_clustered(idx, centres, a.rows - covered, g, a.sigma)
                before = {f"nprobe{p}": round(_step_ms(idx, q, 10, p), 3) for p in (2, 8)}
                t_abs, new = _wall(idx.absorb_delta)
                assert new is not None and idx.covered == idx.rows // 32 * 32
                after = {f"nprobe{p}": round(_step_ms(idx, q, 10, p), 3) for p in (2, 8)}
                recall_absorbed = {f"nprobe{p}": round(_recall(idx, q, 10, p), 4) for p in (2, 8)}
                t_reb, _ = _wall(idx.build_ivf)                 # the parent's way out of the same delta: train + assign + host build
                recall_retrained = {f"nprobe{p}": round(_recall(idx, q, 10, p), 4) for p in (2, 8)}
                idx.drop_ivf()
                eng.drop_index(name)
                torch.cuda.empty_cache()
                if rep:
                    rec["rebuild_ms"].append(round(t_reb, 2))
                    rec["absorb_ms"].append(round(t_abs, 2))
            out["delta"][str(share)] = {**rec, "covered": covered, "delta_rows": a.rows - covered,
                                        "step_1024q_ms_unabsorbed": before, "step_1024q_ms_absorbed": after,
                                        "recall10_absorbed": recall_absorbed, "recall10_retrained": recall_retrained}
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
