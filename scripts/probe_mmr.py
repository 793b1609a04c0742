"""What the diversified (MMR) search costs next to the candidate search it rides on: 1 M x 1024 fp32 rows, 32 queries, k = 10,
lambda = 0.5, fetch_k = 32 and 128.

Per fetch_k, in one process on one index, everything on one stream, hipEvents around `iters` calls, three interleaved rounds:
  (a) rass_index_search_mmr_device: ceil(fetch_k / 32) chained scan passes + Gram + selection;
  (b) the candidates alone the way a device caller gets them without this entry point: rass_index_search_device (k = 32), then
      rass_index_search_device_after per further pass, the bound taken from the previous pass's last column on the device;
  (c) rass_index_rows_gram_device alone over (b)'s candidates.
The scan kernels inside (a) are timed by the engine's own kernel timing; (a) minus those is everything else the call
launches (normalise, merge, store, Gram, selection), and (a) - (b) is what the re-rank adds to the candidate search.  There is
no gather launch: the Gram kernel reads the slab.  One JSON line per fetch_k.  N=<rows> / ITERS=<n> in the environment shrink it.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rassengine_amd.engine import Engine, HipTimer

n, dim, nq, k = int(os.environ.get("N", 1_000_000)), 1024, 32, 10
iters = int(os.environ.get("ITERS", 20))
rounds = 3
eng = Engine(0, dim)
stream = torch.cuda.Stream()
eng.set_stream(int(stream.cuda_stream))
timer = HipTimer()

with torch.cuda.stream(stream):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    idx = eng.open_index("probe", n)
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        x = torch.randn((m, dim), generator=gen, device="cuda", dtype=torch.float32)
        idx.add_device(x.data_ptr(), m, 0, normalize=True)
        eng.synchronize()
    q = torch.from_numpy(np.random.default_rng(7).standard_normal((nq, dim), dtype=np.float32)).cuda()
    lam = torch.full((nq,), 0.5, device="cuda")
    after_s = torch.empty((nq,), device="cuda")
    after_r = torch.empty((nq,), dtype=torch.int64, device="cuda")

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

    for fetch_k in (32, 128):
        passes = (fetch_k + 31) // 32
        out_s = torch.empty((nq, k), device="cuda")
        out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        out_r = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        ps = [torch.empty((nq, 32), device="cuda") for _ in range(passes)]
        pi = [torch.empty((nq, 32), dtype=torch.int64, device="cuda") for _ in range(passes)]
        cand = torch.empty((nq, fetch_k), dtype=torch.int64, device="cuda")
        gram = torch.empty((nq, fetch_k, fetch_k), device="cuda")

        def mmr():
            idx.search_mmr_device(q.data_ptr(), nq, k, fetch_k, lam.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), out_r.data_ptr())

        def chain():
            idx.search_device(q.data_ptr(), nq, 32, ps[0].data_ptr(), pi[0].data_ptr())
            for p in range(1, passes):
                after_s.copy_(ps[p - 1][:, 31])
                after_r.copy_(pi[p - 1][:, 31])
                idx.search_device_after(q.data_ptr(), nq, 32, after_s.data_ptr(), after_r.data_ptr(), ps[p].data_ptr(), pi[p].data_ptr())

        def gram_only():
            idx.rows_gram_device(cand.data_ptr(), nq, fetch_k, gram.data_ptr())

        chain()
        cand.copy_(torch.cat(pi, dim=1)[:, :fetch_k])
        a_ms, b_ms, c_ms = [], [], []
        for _ in range(rounds):
            a_ms.append(timed(mmr, iters))
            b_ms.append(timed(chain, iters))
            c_ms.append(timed(gram_only, iters))
        eng.kernel_timing_begin(16)
        mmr()
        eng.synchronize()
        scan_ms, launches = eng.kernel_timing_end()
        a, b, c = float(np.median(a_ms)), float(np.median(b_ms)), float(np.median(c_ms))
        print(json.dumps({
            "rows": n, "dim": dim, "nq": nq, "k": k, "fetch_k": fetch_k, "lambda": 0.5, "passes": passes,
            "a_mmr_group_ms": round(a, 4), "a_rounds_ms": [round(v, 4) for v in a_ms],
            "a_scan_kernels_ms": round(scan_ms, 4), "a_scan_launches": launches, "a_rest_ms": round(a - scan_ms, 4),
            "b_candidates_chain_ms": round(b, 4), "b_rounds_ms": [round(v, 4) for v in b_ms],
            "c_gram_alone_ms": round(c, 4), "c_rounds_ms": [round(v, 4) for v in c_ms],
            "gather_ms": 0.0, "select_and_rest_ms": round(a - b - c, 4),
            "added_ms": round(a - b, 4), "added_over_candidates": round((a - b) / b, 4), "a_over_b": round(a / b, 4),
        }), flush=True)
eng.close()
