"""Completeness guard of the scan kernels (CPU: cross-compiles, runs nothing).

scan_topk.hip, scan_bf16.hip and scan_i8.hip are compiled for gfx950 with the Makefile's flags and every instantiation of
the six scan kernel families found in the assembly must be in tests/golden/scan_kernels_launched.txt: the sorted list of the
distinct scan kernels a GPU run of the suite's stride sweeps actually launched, written by scripts/record_scan_kernels.py.
A compiled kernel the list lacks was never run by those tests; a listed name that is no longer compiled makes the list stale.
``UNREACHED`` may hold kernels no public entry point can reach, each with its reason; a dead instantiation is better deleted.

Only kernel names and descriptor directives are read from the assembly.  The VGPR count and scratch size of every kernel are
printed, and no kernel of scan_topk.hip may need scratch.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rassengine_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_kernels_launched.txt")
SOURCES = ("scan_topk", "scan_bf16", "scan_i8")
# the six families: rass::<name><template arguments>
SCAN_KERNEL = re.compile(r"\brass::((?:scan_topk_f32(?:_wide|_pair)?|scan_bf16_topk|scan_i8_topk|scan_i8_cert)_kernel<[^>]*>)")
FAMILY_COUNTS = {"scan_topk_f32_kernel": 272, "scan_topk_f32_wide_kernel": 40, "scan_topk_f32_pair_kernel": 8,
                 "scan_bf16_topk_kernel": 32, "scan_i8_topk_kernel": 12, "scan_i8_cert_kernel": 4}   # int8 IVF: strides 512 / 1 024 only

# kernel name -> why no public entry point can reach it
UNREACHED = {}


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
    """{kernel name as the golden list spells it: (source, VGPRs, scratch bytes)} of the three scan sources."""
    hipcc = _hipcc()
    assert hipcc, "hipcc not found (set HIPCC)"
    out_dir = tmp_path_factory.mktemp("scan_asm")
    procs = []
    for src in SOURCES:      # side by side: scan_topk.hip alone takes most of the time
        out = out_dir / (src + ".s")
        cmd = [hipcc] + _makefile_flags(src) + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, src + ".hip")]
        procs.append((src, out, cmd, subprocess.Popen(cmd, cwd=CSRC)))
    kernels = {}
    for src, out, cmd, p in procs:
        assert p.wait() == 0, cmd
        desc = _descriptors(out.read_text())
        mangled = sorted(desc)
        plain = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(plain) == len(mangled)
        for m, name in zip(mangled, plain):
            hit = SCAN_KERNEL.search(name)
            if hit:
                assert hit.group(1) not in kernels, hit.group(1)
                kernels[hit.group(1)] = (src, desc[m][".amdhsa_next_free_vgpr"], desc[m][".amdhsa_private_segment_fixed_size"])
    return kernels


def _golden():
    names = [ln.strip() for ln in open(GOLDEN, encoding="utf-8") if ln.strip()]
    assert names == sorted(set(names)), "the golden list is sorted and holds every name once"
    return set(names)


def test_every_family_is_found(compiled):
    count = {}
    for name in compiled:
        count[name.split("<")[0]] = count.get(name.split("<")[0], 0) + 1
    assert count == FAMILY_COUNTS, count


def test_every_compiled_scan_kernel_was_launched_by_the_suite(compiled):
    launched = _golden()
    for name, reason in UNREACHED.items():
        assert reason and name in compiled and name not in launched, ("stale UNREACHED entry", name)
    never = sorted(set(compiled) - launched - set(UNREACHED))
    assert not never, ("compiled, but launched by no test of the recorded run", len(never), never)
    gone = sorted(launched - set(compiled))
    assert not gone, ("listed as launched, but no longer compiled", gone)


def test_resources_and_no_scratch_in_scan_topk(compiled):
    for name, (src, vgprs, scratch) in sorted(compiled.items()):
        print("%-14s %-70s %3d VGPRs, scratch %d" % (src, name, vgprs, scratch))
    spilled = {n: v for n, v in compiled.items() if v[0] == "scan_topk" and v[2] != 0}
    assert not spilled, spilled
    assert sum(1 for v in compiled.values() if v[0] == "scan_topk") == 320


def test_scan_kernel_name_names_a_compiled_kernel(compiled):
    """rass_scan_kernel_name (host code: the library loads without a GPU) at every supported stride and query-count class."""
    from rassengine_amd import _native
    L = _native.lib()
    strides = list(range(128, 1025, 128)) + list(range(1280, 2049, 256))
    for stride in strides:
        for dim in (stride, stride - 28):                 # the stride itself and a dim that ends inside it
            for nq in (1, 16, 17, 32):
                name = L.rass_scan_kernel_name(dim, nq).decode()
                assert name in compiled, (dim, nq, name)
                want_nt = ", 1, " if nq <= 16 else ", 2, "
                assert stride > 1024 or want_nt in name, (dim, nq, name)
    assert L.rass_scan_kernel_name(1100, 16) == b"scan_topk_f32_wide_kernel<5, 2, false, false, false, false>"
    assert L.rass_scan_kernel_name(2048, 32) == b"scan_topk_f32_wide_kernel<4, 4, false, false, false, false>"
    for dim, nq in ((0, 1), (2049, 1), (1024, 0), (1024, 33)):
        assert L.rass_scan_kernel_name(dim, nq) == b""
