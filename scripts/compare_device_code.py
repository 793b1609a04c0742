#!/usr/bin/env python3
"""Are the kernels of two source trees the same device code?  (CPU: cross-compiles, runs nothing.)

    python scripts/compare_device_code.py [--details] OLD/rassengine_amd/csrc NEW/rassengine_amd/csrc [UNIT ...]

Compiles the named units of each tree (scan_topk group_topk ...: UNIT.hip; by default every encoder GEMM unit,
encoder_gemm.hip and gemm_*.hip, whichever exist) with the Makefile's flags for that unit, its own "FLAGS +=" line
included, plus --cuda-device-only -S and compares, kernel by kernel: the instruction text of the function (local labels
.LBB* / .Ltmp* renumbered in order of appearance, comments and debug directives dropped) and the .amdhsa_ resource lines
of its kernel descriptor (VGPR / AGPR / SGPR counts, scratch, LDS).  One line per kernel; exit status 1 if a kernel
differs or the two sets of kernel symbols differ.  --details adds, under every kernel that differs, what moved: the
descriptor values old -> new and the instruction classes (a mnemonic's first two words) whose counts differ or agree."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def flags(csrc, unit):
    text = open(os.path.join(csrc, "Makefile"), encoding="utf-8").read()
    arch = re.search(r"^ARCH \?= (\S+)", text, flags=re.M).group(1)
    base = re.search(r"^FLAGS := (.*)$", text, flags=re.M).group(1)
    own = re.findall(r"^\$\(OBJDIR\)/%s\.o: FLAGS \+= (.*)$" % re.escape(unit), text, flags=re.M)
    return " ".join([base] + own).replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


def units(csrc, names=()):
    """The named units' sources (missing ones are left out: their kernels then show as ONLY IN the other tree); no names: the
    encoder GEMM units."""
    if names:
        return [p for p in (os.path.join(csrc, n + ".hip") for n in sorted(names)) if os.path.exists(p)]
    return sorted(p for p in glob.glob(os.path.join(csrc, "*.hip"))
                  if os.path.basename(p) == "encoder_gemm.hip" or os.path.basename(p).startswith("gemm_"))


def compile_unit(args):
    csrc, path, out = args
    unit = os.path.splitext(os.path.basename(path))[0]
    cmd = [os.environ.get("HIPCC", "hipcc")] + flags(csrc, unit) + ["--cuda-device-only", "-S", "-o", out, path]
    subprocess.run(cmd, check=True, capture_output=True, cwd=csrc)
    return open(out, encoding="utf-8").read()


_LABEL = re.compile(r"\.L(BB|tmp)\d+(_\d+)?")


def kernels(asm):
    """kernel symbol -> (normalised instruction text, sorted .amdhsa_ lines)"""
    body, desc, cur, name, dname = {}, {}, None, None, None
    for raw in asm.splitlines():
        s = raw.strip()
        m = re.match(r"^\.amdhsa_kernel\s+(\S+)", s)   # (the descriptor sits between s_endpgm and .Lfunc_end)
        if m:
            dname, desc[m.group(1)] = m.group(1), []
            continue
        if s.startswith(".end_amdhsa_kernel"):
            dname = None
            continue
        if dname is not None:
            if s.startswith(".amdhsa_"):
                desc[dname].append(s)
            continue
        m = re.match(r"^(_Z[\w$.]+):", s)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None and re.match(r"^\.Lfunc_end\d+:", s):
            body[name], cur = cur, None
            continue
        if cur is not None:
            s = s.split(";", 1)[0].strip() if not s.startswith(";;#") else s
            if s and not re.match(r"^\.(loc|file|cfi_|p2align|section|text)\b", s):
                cur.append(s)
    out = {}
    for k in desc:   # kernels only (functions with a descriptor)
        seen = {}
        text = "\n".join(_LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), ln) for ln in body.get(k, []))
        out[k] = (text, sorted(desc[k]))
    return out


def tree(csrc, tmp, tag, names):
    us = units(csrc, names)
    jobs = [(csrc, u, os.path.join(tmp, "%s_%s.s" % (tag, os.path.basename(u)))) for u in us]
    with ThreadPoolExecutor(max(1, len(jobs))) as ex:
        asms = list(ex.map(compile_unit, jobs))
    table = {}
    for u, a in zip(us, asms):
        for k, v in kernels(a).items():
            assert k not in table, "kernel %s in two units" % k
            table[k] = v + (os.path.basename(u),)
    return table


def classes(text):
    """instruction class -> count; the class of a mnemonic is its first two words (v_mfma, buffer_load, ds_read, s_waitcnt)."""
    out = {}
    for ln in text.splitlines():
        word = ln.split()[0]
        if not word.endswith(":") and not word.startswith((".", ";")):
            c = "_".join(word.split("_")[:2])
            out[c] = out.get(c, 0) + 1
    return out


def explain(old, new):
    """The lines --details prints under a kernel that differs: descriptor values old -> new (the registers, scratch and LDS
    always, the rest where they differ) and the instruction classes whose counts differ."""
    do, dn = (dict(ln.split(None, 1) for ln in d) for d in (old[1], new[1]))
    always = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_next_free_sgpr", ".amdhsa_private_segment_fixed_size",
              ".amdhsa_group_segment_fixed_size")
    desc = ["%s %s -> %s" % (k[len(".amdhsa_"):], do.get(k, "-"), dn.get(k, "-"))
            for k in sorted(set(do) | set(dn), key=lambda k: (k not in always, k)) if k in always or do.get(k) != dn.get(k)]
    co, cn = classes(old[0]), classes(new[0])
    diff = ["%s %d -> %d" % (c, co.get(c, 0), cn.get(c, 0)) for c in sorted(set(co) | set(cn)) if co.get(c, 0) != cn.get(c, 0)]
    same = sorted(c for c in co if co[c] == cn.get(c))
    return ["    " + "; ".join(desc),
            "    instructions %d -> %d; classes that differ: %s" % (sum(co.values()), sum(cn.values()), "; ".join(diff) or "none"),
            "    classes with equal counts: " + " ".join("%s=%d" % (c, co[c]) for c in same)]


def main():
    argv = [a for a in sys.argv[1:] if a != "--details"]
    details = len(argv) != len(sys.argv) - 1
    old_csrc, new_csrc = os.path.abspath(argv[0]), os.path.abspath(argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        old, new = tree(old_csrc, tmp, "old", argv[2:]), tree(new_csrc, tmp, "new", argv[2:])
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            res = "ONLY IN %s" % ("OLD" if k in old else "NEW")
        else:
            res = "identical" if old[k][:2] == new[k][:2] else \
                "DIFFERS (%s)" % ("code" if old[k][0] != new[k][0] else "resources")
        bad += res != "identical"
        n = len((new.get(k) or old[k])[0].splitlines())
        print("%-10s %6d lines  %-18s %s" % (res, n, (new.get(k) or old[k])[2], k))
        if details and res.startswith("DIFFERS"):
            print("\n".join(explain(old[k], new[k])))
    print("%d kernels, %d not identical" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
