"""Build guard for the 64-query pair kernel of the batched exact fp32 scan (CPU: cross-compiles, runs nothing).

scan_topk_f32_pair_kernel<CH> (scan_topk.hip) must fit two waves per SIMD (256 registers per wave) with its 16 * CH
registers of query fragments and no scratch: a stride that spills must not be eligible (scan_pair_supported_stride).
So scan_topk.hip is compiled for gfx950 with the Makefile's flags and, for EVERY instantiation of the kernel found in the
assembly, the kernel descriptor must say .private_segment_fixed_size 0 and at most 256 VGPRs.

The pair kernel's claim to bit-identical scores rests on using the 32-query kernel's MFMA chain: every v_mfma in it must
be v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per wave slice), 2 blocks x CH chunks x 4 k-steps x 4 N-tiles of them in
the main loop (no 32x32x2 form, no other shape).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rassengine_amd", "csrc")
KERNEL = re.compile(r"^_ZN4rass25scan_topk_f32_pair_kernelILi(\d+)EEEvNS_8ScanArgsE$")


def _hipcc():
    h = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not h and os.path.exists("/opt/rocm/bin/hipcc"):
        h = "/opt/rocm/bin/hipcc"
    return h


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    arch = re.search(r"^ARCH \?= (\S+)", text, flags=re.M).group(1)
    base = re.search(r"^FLAGS := (.*)$", text, flags=re.M).group(1)
    return base.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = _hipcc()
    assert hipcc, "hipcc not found (set HIPCC)"
    out = tmp_path_factory.mktemp("scan_pair_asm") / "scan_topk.s"
    cmd = [hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "scan_topk.hip")]
    subprocess.run(cmd, check=True, cwd=CSRC)
    return out.read_text()


def _kernels(asm_text):
    """{CH: (body lines, descriptor lines)} of every pair-kernel instantiation."""
    found = {}
    lines = asm_text.splitlines()
    for n, raw in enumerate(lines):
        m = KERNEL.match(raw.split(":")[0]) if ":" in raw else None   # "<symbol>:   ; @<symbol>"
        if not m:
            continue
        end = next(i for i in range(n, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel"))
        desc = next(i for i in range(n, end) if lines[i].strip().startswith(".amdhsa_kernel"))
        found[int(m.group(1))] = (lines[n + 1:desc], lines[desc:end])
    return found


def _directive(desc, name):
    for raw in desc:
        t = raw.split(";")[0].split()
        if len(t) == 2 and t[0] == name:
            return int(t[1], 0)
    raise AssertionError("no %s in the kernel descriptor" % name)


def test_every_instantiation_has_no_scratch_and_fits_two_waves_per_simd(asm):
    ks = _kernels(asm)
    assert sorted(ks) == [1, 2, 3, 4, 5, 6, 7, 8], sorted(ks)   # one per eligible stride (scan_pair_supported_stride)
    for ch, (body, desc) in sorted(ks.items()):
        assert _directive(desc, ".amdhsa_private_segment_fixed_size") == 0, ch
        vgprs = _directive(desc, ".amdhsa_next_free_vgpr")
        print("CH = %d: %d VGPRs, scratch 0" % (ch, vgprs))
        assert vgprs <= 256, (ch, vgprs)
        assert not any(re.match(r"\s*scratch_", ln) for ln in body), ch


def test_main_loop_is_the_16x16x4_f32_chain_only(asm):
    ks = _kernels(asm)
    assert ks
    for ch, (body, _) in sorted(ks.items()):
        mfma = [ln.split()[0] for ln in body if ln.strip().startswith("v_mfma")]
        assert mfma and set(mfma) == {"v_mfma_f32_16x16x4_f32"}, (ch, sorted(set(mfma)))
        # one tile per iteration: 2 blocks x CH chunks x 4 k-steps x 4 N-tiles, nowhere else
        assert len(mfma) == 2 * ch * 4 * 4, (ch, len(mfma))
        # every chain starts from zero (C = 0 literal) exactly once per (block, N-tile)
        zero_c = [ln for ln in body if ln.strip().startswith("v_mfma") and ln.split("//")[0].split(";")[0].rstrip().endswith(", 0")]
        assert len(zero_c) == 2 * 4, (ch, len(zero_c))
