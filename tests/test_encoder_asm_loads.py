"""Regression guard for the encoder kernels' inline-asm global loads (CPU: cross-compiles, runs nothing).

Several encoder kernels issue global loads from inline asm and retire them later with one hand-placed `s_waitcnt`
(the p5 epilogue's bias / (mean, rstd) / gamma / beta / colsum loads, gemm_p5.hip; ld16_issue, encoder_misc.hip;
attention64_kernel, encoder_attn.hip).  The compiler's waitcnt pass does not see those loads: if the register allocator
moved, copied or spilled a destination register before the wait, or reused it, the kernel would read a value that has
not landed yet and be silently wrong.  That is correct today only because of where this compiler puts things, so the
device assembly of these modules is checked here on every build:

for every `;;#ASMSTART` block that holds a `global_load*` / `buffer_load*` into VGPRs, the instructions that follow it
in the same function up to the first `s_waitcnt` whose vmcnt retires that load (the compiler's or an asm block's:
vmcnt(N) waits until at most N vector-memory operations are outstanding, and they complete in order, so it retires the
load once N or more were issued after it) must not name any of its destination registers — no read, no write, no
v_mov / v_accvgpr / scratch or buffer store (spill) of them — and the function must not end first.  Scratch use as such is fine (the p5 epilogue spills other registers, legitimately).  The walk is linear in
the assembly text, which is how the compiler lays these straight-line regions out.
"""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rassengine_amd", "csrc")
MODULES = ("gemm_tile128", "gemm_fewrows", "gemm_p5", "gemm_p4", "encoder_misc", "encoder_attn")

_VMEM = re.compile(r"^(global_|buffer_|scratch_|flat_)")
_ASM_LOAD = re.compile(r"^(global_load\w*|buffer_load\w*)\s+(v\d+|v\[\d+:\d+\])\s*,")
_VREG = re.compile(r"\bv(?:(\d+)\b|\[(\d+):(\d+)\])")
_VMCNT = re.compile(r"\bvmcnt\((\d+)\)")


def _hipcc():
    h = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not h and os.path.exists("/opt/rocm/bin/hipcc"):
        h = "/opt/rocm/bin/hipcc"
    return h


def _makefile_flags(module):
    """The Makefile's FLAGS (minus $(EXTRA)) plus its per-object additions for `module`."""
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    arch = re.search(r"^ARCH \?= (\S+)", text, flags=re.M).group(1)
    base = re.search(r"^FLAGS := (.*)$", text, flags=re.M).group(1)
    base = base.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    extra = re.findall(r"^\$\(OBJDIR\)/%s\.o: FLAGS \+= (.*)$" % re.escape(module), text, flags=re.M)
    return base + [f for line in extra for f in line.split()]


def _regs(operands):
    out = set()
    for m in _VREG.finditer(operands):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def _functions(asm_text):
    """(name, [(line number, instruction text, inside an asm block)]) per function of the assembly."""
    funcs, cur, name, in_asm = [], None, None, False
    for ln, raw in enumerate(asm_text.splitlines(), 1):
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m and cur is None and not m.group(1).startswith(".L"):
            name, cur = m.group(1), []
            continue
        if cur is not None and re.match(r"^\.Lfunc_end\d+:", s):
            funcs.append((name, cur))
            cur = None
            continue
        if cur is None:
            continue
        s = s.split(";", 1)[0].strip()   # comments
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append((ln, s, in_asm))
    return funcs


def scan_asm_loads(asm_text):
    """-> (number of asm loads checked, [problem strings])."""
    n_loads, problems = 0, []
    for fname, ins in _functions(asm_text):
        for i, (ln, s, in_asm) in enumerate(ins):
            m = _ASM_LOAD.match(s) if in_asm else None
            if not m or "_lds" in m.group(1) or re.search(r"\blds\b", s):
                continue
            n_loads += 1
            dst = _regs(m.group(2))
            issued_after, retired = 0, False
            for ln2, s2, _ in ins[i + 1:]:
                op = s2.split(None, 1)
                mnem, opnds = op[0], (op[1] if len(op) > 1 else "")
                if mnem.startswith("s_waitcnt"):
                    w = _VMCNT.search(opnds)
                    if w and issued_after >= int(w.group(1)):
                        retired = True
                        break
                    continue
                touched = _regs(opnds) & dst
                if touched:
                    problems.append("%s: asm load at line %d (%s): v%s used by `%s` at line %d before its s_waitcnt"
                                    % (fname, ln, s, min(touched), s2, ln2))
                    break
                if _VMEM.match(mnem):
                    issued_after += 1
            else:
                if not retired:
                    problems.append("%s: asm load at line %d (%s): the function ends before an s_waitcnt retires it"
                                    % (fname, ln, s))
    return n_loads, problems


def test_scanner_flags_a_use_before_the_wait():
    """The checker itself, on hand-written assembly: a wait that retires the load (vmcnt(1) with one later load in flight),
    one that does not (vmcnt(1) with nothing after it), a spill of a destination before the wait, a function ending first."""
    head = "k:\n"
    tail = ".Lfunc_end0:\n"
    ok = head + ";;#ASMSTART\nglobal_load_dwordx4 v[4:7], v[0:1], off\n;;#ASMEND\nglobal_load_dword v9, v[2:3], off\n" \
                "s_waitcnt vmcnt(1)\nv_add_f32_e32 v8, v4, v9\n" + tail
    n, p = scan_asm_loads(ok)
    assert n == 1 and p == []
    early = ok.replace("global_load_dword v9, v[2:3], off\ns_waitcnt vmcnt(1)", "s_waitcnt vmcnt(1)")
    n, p = scan_asm_loads(early)
    assert n == 1 and len(p) == 1 and "v4" in p[0]
    spill = head + ";;#ASMSTART\nglobal_load_dwordx2 v[4:5], v[0:1], off\n;;#ASMEND\n" \
                   "scratch_store_dword off, v5, s33 offset:8 ; 4-byte Folded Spill\n;;#ASMSTART\ns_waitcnt vmcnt(0)\n;;#ASMEND\n" + tail
    n, p = scan_asm_loads(spill)
    assert n == 1 and len(p) == 1 and "v5" in p[0] and "line 5" in p[0]
    unended = head + ";;#ASMSTART\nglobal_load_dword v4, v[0:1], off\n;;#ASMEND\ns_endpgm\n" + tail
    n, p = scan_asm_loads(unended)
    assert n == 1 and len(p) == 1 and "ends" in p[0]


def test_inline_asm_loads_are_waited_for_before_use(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed")

    def compile_one(mod):
        out = tmp_path / (mod + ".s")
        cmd = [hipcc] + _makefile_flags(mod) + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, mod + ".hip")]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900, cwd=CSRC)
        return mod, out.read_text()

    with ThreadPoolExecutor(len(MODULES)) as ex:
        asm = dict(ex.map(compile_one, MODULES))
    counts, problems = {}, []
    for mod in MODULES:
        n, p = scan_asm_loads(asm[mod])
        counts[mod] = n
        problems += ["%s.hip: %s" % (mod, x) for x in p]
    print("asm loads checked per module:", counts)
    # a refactor that removes the asm loads (or a scanner that stops finding them) must not pass silently
    # (of the GEMM units gemm_p5 holds them all: p4's loads are compiler builtins, which its waitcnt pass sees)
    assert counts["gemm_p5"] > 0 and counts["encoder_misc"] > 0 and counts["encoder_attn"] > 0, counts
    assert problems == [], "\n".join(problems[:20])
