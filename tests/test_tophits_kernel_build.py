"""Build guard of the top-hits scan (CPU: cross-compiles, runs nothing).

scan_tophits.hip is compiled for gfx950 with the Makefile's flags.  It must yield exactly the 16 intended instantiations of
``scan_tophits_f32_kernel<CH, NT>`` — CH = 1 .. 8 (row strides 128 .. 1024), NT = 1 (<= 16 queries) and NT = 2 (17 .. 32); the
key column, the bitmap and top_hits are kernel arguments, not template parameters — and none of them may use scratch
(``.amdhsa_private_segment_fixed_size`` 0) or more than 256 VGPRs (512 threads, two waves per SIMD); static + dynamic LDS must
fit a CU's 160 KiB.  The Makefile must list the new sources and build the scan with the flags of the group-top scan (no flag
of its own: the scan adds no arithmetic to the score).  VGPR counts are printed.  Only kernel names and descriptor directives
are read from the assembly.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rassengine_amd", "csrc")
KERNEL = re.compile(r"\brass::(scan_tophits_f32_kernel<(\d+), (\d+)>)")
WANTED = {"scan_tophits_f32_kernel<%d, %d>" % (ch, nt) for ch in range(1, 9) for nt in (1, 2)}
VGPR_BUDGET = 256       # 512 threads, two waves per SIMD
RELAXED = ("-ffast-math", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fhip-fp32-correctly-rounded-divide-sqrt=0",
           "-funsafe-math-optimizations", "-freciprocal-math", "-fapprox-func", "-ffp-contract=fast", "-ffp-contract=on",
           "-fno-honor-nans", "-fno-honor-infinities", "-ffinite-math-only", "-fno-signed-zeros", "-fassociative-math")


def _hipcc():
    h = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not h and os.path.exists("/opt/rocm/bin/hipcc"):
        h = "/opt/rocm/bin/hipcc"
    return h


def _makefile_flags(source):
    """The Makefile's FLAGS plus what it adds for this source's object alone."""
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    arch = re.search(r"^ARCH \?= (\S+)", text, flags=re.M).group(1)
    base = re.search(r"^FLAGS := (.*)$", text, flags=re.M).group(1)
    flags = base.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    for extra in re.findall(r"^\$\(OBJDIR\)/%s\.o: FLAGS \+= (.*)$" % re.escape(source), text, flags=re.M):
        flags += extra.split()
    return flags


def _descriptors(asm_text):
    """{mangled name: {directive: value}} of every kernel descriptor (.amdhsa_kernel .. .end_amdhsa_kernel)."""
    found, cur = {}, None
    for raw in asm_text.splitlines():
        t = raw.split(";")[0].split()
        if not t:
            continue
        if t[0] == ".amdhsa_kernel":
            cur = found.setdefault(t[1], {})
        elif t[0] == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and len(t) == 2 and t[0].startswith(".amdhsa_"):
            try:
                cur[t[0]] = int(t[1], 0)
            except ValueError:
                pass
    return found


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{kernel name: (VGPRs, scratch bytes, static LDS bytes)} of scan_tophits.hip."""
    hipcc = _hipcc()
    assert hipcc, "hipcc not found (set HIPCC)"
    out = tmp_path_factory.mktemp("tophits_asm") / "scan_tophits.s"
    cmd = [hipcc] + _makefile_flags("scan_tophits") + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "scan_tophits.hip")]
    subprocess.run(cmd, cwd=CSRC, check=True)
    desc = _descriptors(out.read_text())
    mangled = sorted(desc)
    plain = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(plain) == len(mangled)
    kernels = {}
    for m, name in zip(mangled, plain):
        hit = KERNEL.search(name)
        assert hit, ("a kernel of another family in scan_tophits.hip", name)
        assert hit.group(1) not in kernels
        kernels[hit.group(1)] = (desc[m][".amdhsa_next_free_vgpr"], desc[m][".amdhsa_private_segment_fixed_size"],
                                 desc[m][".amdhsa_group_segment_fixed_size"])
    return kernels


def test_the_sixteen_instantiations_no_scratch_and_the_vgpr_budget(compiled):
    for name, (vgprs, scratch, lds) in sorted(compiled.items()):
        print("%-38s %3d VGPRs, scratch %d, static LDS %d" % (name, vgprs, scratch, lds))
    assert set(compiled) == WANTED, sorted(set(compiled) ^ WANTED)
    spilled = {n: v for n, v in compiled.items() if v[1] != 0}
    assert not spilled, spilled
    assert all(v[0] <= VGPR_BUDGET for v in compiled.values()), {n: v[0] for n, v in compiled.items() if v[0] > VGPR_BUDGET}
    # static LDS (filters, thresholds, tags, the parked keys) next to the 4 dynamic partial images
    for name, (_, _, lds) in compiled.items():
        nt = int(KERNEL.search("rass::" + name).group(3))
        assert lds + 4 * 8 * nt * 16 * 36 * 4 <= 160 * 1024, (name, lds)


def test_makefile_builds_the_scan_like_its_neighbours():
    flags = _makefile_flags("scan_tophits")
    assert flags == _makefile_flags("scan_grouptop") and "--offload-arch=gfx950" in flags and "-O3" in flags
    for f in flags:     # nothing that relaxes the score's arithmetic
        assert f not in RELAXED, f


def test_makefile_lists_the_new_sources():
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    srcs = re.search(r"^SRCS := (.*)$", text, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS := (.*)$", text, flags=re.M).group(1).split()
    assert {"scan_tophits.hip", "api_tophits.hip", "group_topk.hip"} <= set(srcs) and {"scan_flat.h", "scan_core.h"} <= set(hdrs)
    for s in ("scan_tophits.hip", "api_tophits.hip"):
        assert os.path.exists(os.path.join(CSRC, s)), s
