"""Build guard for the sample stage of the fused fp32 batch (CPU: cross-compiles, runs nothing).

sample_rep_bf16_kernel<CH> (sample_rep.hip) is only worth its launch while it stays what it was written as, for EVERY
instantiation: bf16 MFMAs (v_mfma_f32_16x16x32_bf16) on rows converted in registers (v_cvt_pk_bf16_f32), no scratch (left to
itself hipcc hoists the loop-invariant row fragments out of the tile loop and spills 440 registers at CH = 8), its rows in at
most 160 KiB of LDS, and a tile loop that waits for one query fragment at a time (no s_waitcnt vmcnt below the number of k-steps between the
loop's MFMAs: hipcc merges the counts over the loop entry and the back edge, and with the prologue's loads out of order it
waited for nearly all of them at every tile).

The exact re-rank (scan_bf16.hip, rerank_f32_kernel<1..8> and its wide form) shares its fmaf chain with the stage's rescore
kernel through exact_score.h; factoring it out must not change its device code.  tests/golden/rerank_f32_device_code.json
holds, per kernel, the SHA-256 of the instruction text and resource lines as scripts/compare_device_code.py normalises them:

    python tests/test_sample_rep_build.py TREE/rassengine_amd/csrc > tests/golden/rerank_f32_device_code.json

First taken from the tree before the chain was factored out.  Taken again, from the tree that made the change, when
rerank_f32_body began to count a candidate whose exact score is NaN or -inf as no candidate (include/rass_engine.h, "Scores
that are not finite": one compare and a select ahead of the ranking; the fmaf chain of exact_score.h is untouched): all twelve
kernels changed with it, on purpose.  Any later change of these kernels must again be one that is meant.
"""
import hashlib
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rassengine_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rerank_f32_device_code.json")
KERNEL_A = re.compile(r"^_ZN4rass22sample_rep_bf16_kernelILi(\d+)EEE")
RERANK = re.compile(r"^_ZN4rass(17rerank_f32_kernel|22rerank_f32_wide_kernel)ILi\d+EEE")


def _compare_module():
    spec = importlib.util.spec_from_file_location("compare_device_code", os.path.join(ROOT, "scripts", "compare_device_code.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _hipcc():
    h = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not h and os.path.exists("/opt/rocm/bin/hipcc"):
        h = "/opt/rocm/bin/hipcc"
    return h


def _asm(csrc, unit, out):
    hipcc = _hipcc()
    assert hipcc, "hipcc not found (set HIPCC)"
    cmd = [hipcc] + _compare_module().flags(csrc, unit) + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(csrc, unit + ".hip")]
    subprocess.run(cmd, check=True, cwd=csrc, capture_output=True)
    return open(out, encoding="utf-8").read()


def rerank_fingerprints(csrc, out):
    table = _compare_module().kernels(_asm(csrc, "scan_bf16", out))
    return {k: hashlib.sha256(("\n".join([text] + desc)).encode()).hexdigest() for k, (text, desc) in sorted(table.items())
            if RERANK.match(k)}


@pytest.fixture(scope="module")
def kernel_a(tmp_path_factory):
    """{CH: (instruction lines of sample_rep_bf16_kernel<CH>, its .amdhsa_ descriptor lines)}"""
    asm = _asm(CSRC, "sample_rep", tmp_path_factory.mktemp("sample_rep_asm") / "sample_rep.s")
    found = {}
    for name, (text, desc) in _compare_module().kernels(asm).items():
        m = KERNEL_A.match(name)
        if m:
            found[int(m.group(1))] = (text.splitlines(), desc)
    assert sorted(found) == [1, 2, 3, 4, 5, 6, 7, 8], sorted(found)
    return found


def _desc_value(desc, key):
    for line in desc:
        parts = line.split()
        if parts[0] == key:
            return int(parts[1], 0)
    raise AssertionError(key)


def test_kernel_a_is_bf16_mfma_without_scratch_within_lds(kernel_a):
    for ch, (ins, desc) in sorted(kernel_a.items()):
        ops = [ln.split()[0] for ln in ins]
        mfma = [op for op in ops if op.startswith("v_mfma")]
        assert mfma and set(mfma) == {"v_mfma_f32_16x16x32_bf16"}, (ch, set(mfma))
        assert len(mfma) == 4 * 4 * ch, (ch, len(mfma))            # 4 row blocks x KS k-steps, one tile loop
        assert "v_cvt_pk_bf16_f32" in ops, ch
        assert _desc_value(desc, ".amdhsa_private_segment_fixed_size") == 0, ch
        assert not any(op.startswith("scratch_") for op in ops), ch
        lds = _desc_value(desc, ".amdhsa_group_segment_fixed_size")
        assert lds == 16384 * ch and lds <= 160 * 1024, (ch, lds)


def test_kernel_a_waits_for_one_query_fragment_at_a_time(kernel_a):
    for ch, (ins, _) in sorted(kernel_a.items()):
        first = next(i for i, ln in enumerate(ins) if ln.startswith("v_mfma"))
        last = max(i for i, ln in enumerate(ins) if ln.startswith("v_mfma"))
        waits = [int(m.group(1)) for ln in ins[first - 4:last] for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", ln)] if m]
        ks = 4 * ch
        print("CH = %d: vmcnt waits between the MFMAs: %s" % (ch, sorted(set(waits))))
        assert waits and min(waits) >= ks, (ch, waits)               # KS refills and the filter in flight: only the oldest is due


def test_rerank_kernels_are_the_device_code_they_were(tmp_path):
    golden = json.load(open(GOLDEN, encoding="utf-8"))
    assert len(golden) == 12, sorted(golden)                          # rerank_f32_kernel<1..8>, rerank_f32_wide_kernel<5..8>
    now = rerank_fingerprints(CSRC, tmp_path / "scan_bf16.s")
    assert sorted(now) == sorted(golden)
    changed = [k for k in sorted(golden) if now[k] != golden[k]]
    assert not changed, changed


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        json.dump(rerank_fingerprints(os.path.abspath(sys.argv[1]), os.path.join(tmp, "scan_bf16.s")), sys.stdout, indent=1)
        print()
