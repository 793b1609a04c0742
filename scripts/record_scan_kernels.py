"""Record which scan kernels the suite's stride sweeps launch: rewrites tests/golden/scan_kernels_launched.txt.

One child runs under ``rocprofv3 --kernel-trace`` (no counters, no other tracing; the program after ``--``): ``python -m
pytest -m gpu -x`` on the two matrix files and the files that already sweep every stride for the flat and batch modes.  The
child runs under ``timeout``; on any non-zero status nothing is rewritten and that status is returned.  Then the distinct
names of the six scan kernel families are read from the trace's Kernel_Name column and written, sorted, one per line, in
the spelling tests/test_scan_instantiations_build.py compares with the compiled set.  No test calls this script.

    python scripts/record_scan_kernels.py                        # the golden list
    python scripts/record_scan_kernels.py --without-matrix --out profiles/scan_kernels_launched_before_matrix.txt
"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_kernels_launched.txt")
MATRIX = ["tests/test_gpu_scan_matrix.py", "tests/test_gpu_ivf_matrix.py"]
SWEEPS = ["tests/test_gpu_scan.py", "tests/test_gpu_scan_pair.py", "tests/test_gpu_scan_pair_rank.py", "tests/test_gpu_sample_rep.py",
          "tests/test_gpu_lowprec_floor.py", "tests/test_gpu_prefilter_int8.py", "tests/test_gpu_prefilter_int8_exact.py"]
SCAN_KERNEL = re.compile(r"\brass::((?:scan_topk_f32(?:_wide|_pair)?|scan_bf16_topk|scan_i8_topk|scan_i8_cert)_kernel<[^>]*>)")


def kernel_names(trace_dir):
    """The distinct Kernel_Name values of every kernel-trace CSV under ``trace_dir`` (one per traced process), demangled."""
    names = set()
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s" % trace_dir)
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                names.add(row["Kernel_Name"])
    mangled = sorted(n for n in names if n.startswith("_Z"))
    if mangled:
        plain = subprocess.run(["c++filt"], input="\n".join(n.split(".kd")[0] for n in mangled) + "\n", check=True,
                               capture_output=True, text=True).stdout.splitlines()
        names = (names - set(mangled)) | set(plain)
    return names


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--without-matrix", action="store_true", help="leave the two matrix files out (what the sweeps alone launch)")
    ap.add_argument("--timeout", type=int, default=1100, help="seconds the traced run may take")
    ap.add_argument("--trace-dir", default=None, help="keep the trace here (default: a temporary directory)")
    args = ap.parse_args()
    files = SWEEPS if args.without_matrix else MATRIX + SWEEPS
    with tempfile.TemporaryDirectory() as tmp:
        trace_dir = args.trace_dir or tmp
        cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir,
               "--", sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "--durations=15"] + files
        print(" ".join(cmd), flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print("the traced run ended with status %d: nothing is rewritten" % rc, file=sys.stderr)
            return rc
        found = sorted({m.group(1) for n in kernel_names(trace_dir) for m in [SCAN_KERNEL.search(n)] if m})
    if not found:
        print("the trace names no scan kernel: nothing is rewritten", file=sys.stderr)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("".join(n + "\n" for n in found))
    print("%d distinct scan kernels launched -> %s" % (len(found), os.path.relpath(args.out, ROOT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
