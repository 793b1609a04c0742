"""Probe: compaction of a flat fp32 index (rass_index_compact) against a hipMemcpyAsync device-to-device copy of the same byte
count timed IN THE SAME CALL, and the exact scan's queries/s before and after.

1 M x 1024 fp32 rows (Philox, seed 1234); 10 % / 30 % / 70 % random tombstones and one contiguous dead range.  Per case and
repeat the index is refilled from its seed and re-tombstoned; the repeats of the compaction's steps and of the yardstick
alternate.  The steps are timed with HIP events on the engine stream through the stateless launchers the C entry point is made
of (plan: rass_compact_plan on the index's tags; gather: rass_compact_rows_f32 from the index's slab into a scratch slab;
copy-rebuild: rass_index_set_prefilter's converters are part of rass_index_compact only, so it is the difference between the
whole call's wall time with --prefilter and the sum of the other two, 0 in mode off); the whole rass_index_compact call is
timed on the wall clock (it allocates, synchronises and frees).  Bytes = what the shapes say: tags read twice + the two maps
written (plan), live rows read + round_up(live, 16) rows written (gather).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rassengine_amd import _native as N  # noqa: E402
from rassengine_amd.engine import Engine, HipTimer  # noqa: E402

HIP_MEMCPY_D2D = 3


def _hip_memcpy_async():
    """hipMemcpyAsync of the HIP runtime this process already has mapped (the one librass_hip.so is bound to)."""
    fn = ctypes.CDLL(None).hipMemcpyAsync
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return fn


def _timed(eng, fn):
    t = HipTimer()
    t.start(eng.stream)
    fn()
    t.stop(eng.stream)
    eng.synchronize()
    return t.elapsed_ms()


def _dead(case, rows, rng):
    if case == "range30":
        d = np.zeros(rows, dtype=bool)
        d[rows // 3: rows // 3 + int(0.3 * rows)] = True
        return d
    return rng.random(rows) < float(case) / 100.0


def _scan_qps(idx, q, k, steps):
    nq = q.shape[0]
    s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    torch.cuda.synchronize()
    idx.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr())
    ms = _timed(idx.engine, lambda: [idx.search_device_batch(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr()) for _ in range(steps)])
    return nq * steps / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prefilter", default="off")
    ap.add_argument("--cases", default="10,30,70,range30")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = N.lib()
    memcpy = _hip_memcpy_async()
    dev = torch.device("cuda:0")
    eng = Engine(0, a.dim)
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    q = torch.randn((1024, a.dim), generator=g, device=dev).contiguous()
    out = {"probe": "compact", "rows": a.rows, "dim": a.dim, "prefilter": a.prefilter, "repeats": a.repeats, "cases": {}}
    try:
        for case in a.cases.split(","):
            rng = np.random.default_rng(11)
            dead = _dead(case, a.rows, rng)
            live = int((~dead).sum())
            rec = {k: [] for k in ("plan_ms", "gather_ms", "memcpy_ms", "compact_wall_ms")}
            for rep in range(a.repeats + 1):          # repeat 0 warms every shape and is not reported
                idx = eng.open_index(f"probe-{case}", capacity_rows=a.rows)
                idx.fill_synthetic(a.rows, seed=1234)
                if a.prefilter != "off":
                    idx.set_prefilter(a.prefilter)
                for r in np.flatnonzero(dead):
                    idx.delete(int(r))
                eng.synchronize()
                stride = idx.row_stride
                qps_before = _scan_qps(idx, q, 10, 5)
                new_row = torch.empty(a.rows, dtype=torch.int64, device=dev)
                src_row = torch.empty(a.rows, dtype=torch.int64, device=dev)
                n_live = torch.empty(1, dtype=torch.int64, device=dev)
                ws_bytes = int(L.rass_compact_plan_workspace_bytes(a.rows))
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                dst_rows = (live + 15) // 16 * 16
                dst = torch.empty((max(dst_rows, 16), stride), dtype=torch.float32, device=dev)
                gather_bytes = (live + dst_rows) * stride * 4
                half = torch.empty(gather_bytes // 2, dtype=torch.uint8, device=dev)   # the copy reads and writes as many bytes
                torch.cuda.synchronize()
                st = ctypes.c_void_p(eng.stream)
                plan = _timed(eng, lambda: N.check("plan", L.rass_compact_plan(
                    ctypes.c_void_p(idx.device_tags_ptr), a.rows, ctypes.c_void_p(new_row.data_ptr()),
                    ctypes.c_void_p(src_row.data_ptr()), ctypes.c_void_p(n_live.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                    ws_bytes, st)))
                assert int(n_live.item()) == live
                gather = _timed(eng, lambda: N.check("gather", L.rass_compact_rows_f32(
                    ctypes.c_void_p(idx.device_rows_ptr), ctypes.c_void_p(dst.data_ptr()), stride,
                    ctypes.c_void_p(src_row.data_ptr()), live, a.rows, st)))
                copy = _timed(eng, lambda: memcpy(ctypes.c_void_p(half.data_ptr()), ctypes.c_void_p(idx.device_rows_ptr),
                                                  gather_bytes // 2, HIP_MEMCPY_D2D, st))
                del dst, half, new_row, src_row
                torch.cuda.empty_cache()
                t0 = time.perf_counter()
                idx.compact()
                wall = (time.perf_counter() - t0) * 1e3
                assert idx.rows == idx.count == live
                qps_after = _scan_qps(idx, q, 10, 5)
                eng.drop_index(idx.name)
                if rep:
                    for key, v in (("plan_ms", plan), ("gather_ms", gather), ("memcpy_ms", copy), ("compact_wall_ms", wall)):
                        rec[key].append(round(v, 4))
            med = {k: float(np.median(v)) for k, v in rec.items()}
            out["cases"][case] = {
                **rec, "live": live, "gather_bytes": gather_bytes, "plan_bytes": a.rows * (4 + 4 + 8) + live * 8,
                "gather_GBps": round(gather_bytes / med["gather_ms"] / 1e6, 1),
                "memcpy_GBps": round(gather_bytes / med["memcpy_ms"] / 1e6, 1),
                "gather_vs_memcpy": round(med["memcpy_ms"] / med["gather_ms"], 3),
                "copy_rebuild_ms": round(max(0.0, med["compact_wall_ms"] - med["plan_ms"] - med["gather_ms"]), 4)
                if a.prefilter != "off" else 0.0,
                "scan_qps_before": round(qps_before, 1), "scan_qps_after": round(qps_after, 1),
                "scan_speedup": round(qps_after / qps_before, 3), "rows_over_live": round(a.rows / max(live, 1), 3)}
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
