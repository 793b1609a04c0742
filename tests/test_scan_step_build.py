"""Build guard for the step kernel of the batched exact fp32 scan (CPU: cross-compiles, runs nothing).

scan_topk_f32_step_kernel<CH> (scan_step.hip) is the pair kernel's tile loop around which a workgroup switches query pairs on
its own.  It must keep the pair kernel's budget — two waves per SIMD (at most 256 VGPRs), no scratch, although the switch sits
inside the loop — and its arithmetic: the only MFMA is v_mfma_f32_16x16x4_f32, 2 blocks x CH chunks x 4 k-steps x 4 N-tiles of
them per tile iteration and none anywhere else (the switch multiplies nothing), every chain from zero.  The switch reloads the
query fragments; they must be waited for there: between a tile's MFMAs every vmcnt wait leaves the other 2 * CH loads of the
rolling refill in flight, as in the pair kernel.

That the change which brought the kernel left every kernel of scan_topk.hip as it compiled before is recorded, not tested (it
takes the parent's tree): profiles/scan_step_device_code_compare.txt is scripts/compare_device_code.py's output for that unit.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rassengine_amd", "csrc")
KERNEL = re.compile(r"^_ZN4rass25scan_topk_f32_step_kernelILi(\d+)EEEvNS_8ScanArgsE$")


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
def kernels(tmp_path_factory):
    """{CH: (body lines, descriptor lines)} of every step-kernel instantiation."""
    hipcc = _hipcc()
    assert hipcc, "hipcc not found (set HIPCC)"
    out = tmp_path_factory.mktemp("scan_step_asm") / "scan_step.s"
    cmd = [hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "scan_step.hip")]
    subprocess.run(cmd, check=True, cwd=CSRC)
    lines = out.read_text().splitlines()
    found = {}
    for n, raw in enumerate(lines):
        m = KERNEL.match(raw.split(":")[0]) if ":" in raw else None   # "<symbol>:   ; @<symbol>"
        if not m:
            continue
        end = next(i for i in range(n, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel"))
        desc = next(i for i in range(n, end) if lines[i].strip().startswith(".amdhsa_kernel"))
        found[int(m.group(1))] = (lines[n + 1:desc], lines[desc:end])
    assert sorted(found) == [1, 2, 3, 4, 5, 6, 7, 8], sorted(found)   # one per eligible stride (scan_pair_supported_stride)
    return found


def _directive(desc, name):
    for raw in desc:
        t = raw.split(";")[0].split()
        if len(t) == 2 and t[0] == name:
            return int(t[1], 0)
    raise AssertionError("no %s in the kernel descriptor" % name)


def test_every_instantiation_has_no_scratch_and_fits_two_waves_per_simd(kernels):
    for ch, (body, desc) in sorted(kernels.items()):
        assert _directive(desc, ".amdhsa_private_segment_fixed_size") == 0, ch
        vgprs = _directive(desc, ".amdhsa_next_free_vgpr")
        print("CH = %d: %d VGPRs, scratch 0" % (ch, vgprs))
        assert vgprs <= 256, (ch, vgprs)
        assert not any(re.match(r"\s*scratch_", ln) for ln in body), ch


def test_the_tile_loop_is_the_16x16x4_f32_chain_only(kernels):
    for ch, (body, _) in sorted(kernels.items()):
        at = [n for n, ln in enumerate(body) if ln.strip().startswith("v_mfma")]
        mfma = [body[n].split()[0] for n in at]
        assert mfma and set(mfma) == {"v_mfma_f32_16x16x4_f32"}, (ch, sorted(set(mfma)))
        # one tile per iteration: 2 blocks x CH chunks x 4 k-steps x 4 N-tiles, nowhere else
        assert len(mfma) == 2 * ch * 16, (ch, len(mfma))
        # every chain starts from zero (C = 0 literal) exactly once per (block, N-tile)
        zero_c = [n for n in at if body[n].split("//")[0].split(";")[0].rstrip().endswith(", 0")]
        assert len(zero_c) == 2 * 4, (ch, len(zero_c))
        # In the basic blocks that multiply (hipcc may lay the loop's last block out ahead of its header) every chunk waits for
        # its own load only: vmcnt(2 CH) with the rolling refill of the other loads in flight, 2 CH - 1 at the iteration's first
        # chunk, whose tag load was issued behind it.
        blocks, cur_block = [], []
        for ln in body:
            if re.match(r"^\.LBB\d+_\d+:", ln):
                blocks.append(cur_block)
                cur_block = []
            cur_block.append(ln.strip())
        blocks.append(cur_block)
        hot = [ln for b in blocks if any(x.startswith("v_mfma") for x in b) for ln in b]
        waits = [int(m.group(1)) for ln in hot for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", ln)] if m]
        assert waits and set(waits) <= {2 * ch - 1, 2 * ch}, (ch, waits)
