#!/usr/bin/env python3
"""Which kernels do the encoder GEMM entry points launch?  A probe for comparing two builds of the library.

    python scripts/probe_gemm_routes.py --list                      # the switch settings, one per line
    rocprofv3 --kernel-trace --output-format csv -d OUT/s3 -- python scripts/probe_gemm_routes.py --setting 3 [--root TREE]
    python scripts/probe_gemm_routes.py --diff OUT_A OUT_B          # compare two sets of traces

--setting I calls rass_gemm_bf16, rass_gemm_bf16_ws, rass_gemm_bf16_residual_layernorm, rass_gemm_bf16_ln_input and
rass_gemm_bf16_fold on random data over the grid of tests/test_gemm_route_cpu.py (rows x the four GEMMs of the
1 024 / 4 096 and 768 / 3 072 models x epilogues x with / without scratch) with the I-th switch setting; one process per
setting (the kernels' attributes have process lifetime).  An entry point that refuses a shape is counted, not an error.
--root TREE imports rassengine_amd from another checkout (its built library), so that two builds run the same probe.
--diff reads the kernel traces (one directory per setting) and compares, launch by launch in order, the kernel name,
grid, workgroup and LDS size of every rass:: kernel: "identical, N launches", or the lines that differ."""
import argparse
import csv
import ctypes
import glob
import os
import sys

ROWS = [1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 300, 1024, 1025, 1536, 2048, 8192, 131072]
GEMMS = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (2304, 768), (768, 768), (3072, 768), (768, 3072)]
WS_FLOATS = 16 * 384 * 1024
SETTINGS = [
    {}, {"RASS_GEMM_FEWROWS": "0"}, {"RASS_GEMM_FEWROWS_MAX": "128"}, {"RASS_GEMM_FEWROWS_MAX": "64"},
    {"RASS_GEMM_FEWROWS_RES": "32"}, {"RASS_GEMM_MID": "0"}, {"RASS_GEMM_MID": "2"}, {"RASS_GEMM_VARIANT": "p4"},
    {"RASS_GEMM_VARIANT": "p5"}, {"RASS_GEMM_SPLITK_S": "2"}, {"RASS_GEMM_SPLITK_S": "4"}, {"RASS_GEMM_SPLITK_S": "8"},
    {"RASS_GEMM_SPLITK_S": "16"}, {"RASS_GEMM_MID_BM": "64"}, {"RASS_GEMM_MID_BM": "128"}, {"RASS_GEMM_LNIN_WAVES": "4"},
    {"RASS_GEMM_GRID": "64"}, {"RASS_P5_POLICY": "0"}, {"RASS_ENCODER_LN_FOLD": "0"},
]


def run_setting(index, root, max_rows):
    for k in list(os.environ):
        if k.startswith("RASS_GEMM_") or k in ("RASS_P5_POLICY", "RASS_ENCODER_LN_FOLD"):
            del os.environ[k]
    os.environ.update(SETTINGS[index])
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from rassengine_amd import _native
    L = _native.lib()
    rows = [m for m in ROWS if m <= max_rows]
    mp_max = (max(rows) + 255) // 256 * 256
    g = torch.Generator(device="cuda").manual_seed(index)

    def rnd(shape, dtype, scale=1.0):
        return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(dtype)

    bf, f32 = torch.bfloat16, torch.float32
    X = torch.empty((mp_max, 4096), dtype=bf, device="cuda")
    for r0 in range(0, mp_max, 8192):   # (in pieces: the fp32 temporary of a whole 1 GiB operand is 2 GiB)
        X[r0:r0 + 8192] = rnd((min(8192, mp_max - r0), 4096), bf)
    W = rnd((4096 * 4096,), bf, 1.0 / 32)
    R = torch.empty((mp_max, 4096), dtype=bf, device="cuda")
    R.view(-1)[:] = X.view(-1)
    Y = torch.empty((mp_max, 4096), dtype=bf, device="cuda")
    OUT = torch.empty((mp_max, 4096), dtype=bf, device="cuda")
    bias, gamma, beta, colsum = (rnd((4096,), f32) for _ in range(4))
    ws = torch.empty((WS_FLOATS,), dtype=f32, device="cuda")
    stats = torch.empty((mp_max * 32 * 2,), dtype=f32, device="cuda")
    mr = torch.empty((mp_max, 2), dtype=f32, device="cuda")
    mr[:, 0] = 0.0
    mr[:, 1] = 1.0
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    eps = ctypes.c_float(1e-12)
    calls = refused = 0
    for m in rows:
        mp = (m + 255) // 256 * 256
        for n, k in GEMMS:
            for epi in (0, 1, 2):
                rc = [L.rass_gemm_bf16(p(X), p(W), p(bias), p(R), p(Y), m, mp, n, k, epi, None),
                      L.rass_gemm_bf16_ws(p(X), p(W), p(bias), p(R), p(Y), m, mp, n, k, epi, p(ws), WS_FLOATS * 4, None)]
                calls += 2
                refused += sum(r != 0 for r in rc)
            for use_ws in (False, True):
                rc = L.rass_gemm_bf16_residual_layernorm(p(X), p(W), p(bias), p(R), p(Y), p(gamma), p(beta), eps, p(OUT), m, mp, n, k,
                                                         p(ws) if use_ws else None, WS_FLOATS * 4 if use_ws else 0, None)
                calls += 1
                refused += rc != 0
            for epi in (0, 2):
                rc = L.rass_gemm_bf16_ln_input(p(R), p(gamma), p(beta), eps, p(OUT), p(W), p(bias), p(Y), m, n, k, epi, None)
                calls += 1
                refused += rc != 0
            for epi in (3, 4, 5):
                rc = L.rass_gemm_bf16_fold(p(X), p(W), p(bias), p(R), p(Y), m, mp, n, k, epi, p(mr), p(gamma), p(beta), p(stats),
                                           p(colsum), None)
                calls += 1
                refused += rc != 0
        torch.cuda.synchronize()
    print("setting %d %s: %d calls, %d refused, rows up to %d" % (index, SETTINGS[index] or "default", calls, refused, max(rows)))


def _launches(path):
    rows = []
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r.get("Start_Timestamp", 0)), int(r.get("Dispatch_Id", 0))))
    keys = ["Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
            "LDS_Block_Size"]
    return [tuple(r.get(k, "") for k in keys) for r in rows if "rass" in r.get("Kernel_Name", "")]


def diff(a, b):
    total, bad = 0, []
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    for s in names:
        la, lb = _launches(os.path.join(a, s)), _launches(os.path.join(b, s))
        total += len(la)
        if len(la) != len(lb):
            bad.append("%s: %d launches vs %d" % (s, len(la), len(lb)))
        for i, (x, y) in enumerate(zip(la, lb)):
            if x != y:
                bad.append("%s launch %d: %s  vs  %s" % (s, i, x, y))
                if len(bad) > 40:
                    break
    print("identical, %d launches over %d settings" % (total, len(names)) if not bad and total else "\n".join(bad) or "no launches found")
    return 1 if bad or not total else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--setting", type=int)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--max-rows", type=int, default=131072)
    ap.add_argument("--diff", nargs=2)
    a = ap.parse_args()
    if a.list:
        for i, s in enumerate(SETTINGS):
            print(i, s or "default")
    elif a.diff:
        sys.exit(diff(*a.diff))
    else:
        run_setting(a.setting, a.root, a.max_rows)


if __name__ == "__main__":
    main()
