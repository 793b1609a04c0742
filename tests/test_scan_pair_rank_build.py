"""Build guard for the ranking schedule of the 64-query pair kernel (CPU: cross-compiles, runs nothing).

scan_topk_f32_pair_kernel<CH> (scan_topk.hip) issues the LDS reads of a ranking part ahead of an MFMA chunk (rank_load in
multiply_and_refill_half's before(j)) and consumes them behind it (rank_use in between(j)).  That only pays while the compiler
keeps it so: left to itself hipcc sinks the reads to their first use, behind the MFMAs, and turns a short-circuit predicate
into exec-mask branches with one LDS round trip each.  So, for EVERY instantiation, inside the main loop (from its first
v_mfma to its s_barrier):
  * every run of the ranking's ds_read2st64_b32 (the 8 K-partials of a part) is followed by at least 16 v_mfma (one chunk:
    4 k-steps x 4 N-tiles) before the next s_waitcnt that waits on lgkmcnt
  * there is no s_cbranch_execz / s_cbranch_execnz
  * at CH = 1 (2 slots for 4 parts) the reads of the two parts that share a slot go to disjoint destination registers
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


def _instructions(lines):
    """[(mnemonic, operand text)] of the instruction lines (no labels, directives or comments)."""
    out = []
    for raw in lines:
        s = raw.split(";")[0].split("//")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op, _, rest = s.partition(" ")
        out.append((op, rest.strip()))
    return out


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    """{CH: instructions of the main loop, from its first v_mfma up to its s_barrier}"""
    hipcc = _hipcc()
    assert hipcc, "hipcc not found (set HIPCC)"
    out = tmp_path_factory.mktemp("scan_pair_rank_asm") / "scan_topk.s"
    cmd = [hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "scan_topk.hip")]
    subprocess.run(cmd, check=True, cwd=CSRC)
    lines = out.read_text().splitlines()
    found = {}
    for n, raw in enumerate(lines):
        m = KERNEL.match(raw.split(":")[0]) if ":" in raw else None
        if not m:
            continue
        end = next(i for i in range(n, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel"))
        ins = _instructions(lines[n + 1:end])
        first = next(i for i, (op, _) in enumerate(ins) if op.startswith("v_mfma"))
        barrier = next(i for i in range(first, len(ins)) if ins[i][0] == "s_barrier")
        found[int(m.group(1))] = ins[first:barrier]
    assert sorted(found) == [1, 2, 3, 4, 5, 6, 7, 8], sorted(found)
    return found


def _read_runs(loop):
    """The runs of ds_read2st64_b32 in the loop: [(index of the run's first read, index of its last read)].  A run ends at
    the first v_mfma or lgkmcnt wait behind it."""
    runs, start, last = [], None, None
    for i, (op, rest) in enumerate(loop):
        if op == "ds_read2st64_b32":
            start = i if start is None else start
            last = i
        elif start is not None and (op.startswith("v_mfma") or (op == "s_waitcnt" and "lgkmcnt" in rest)):
            runs.append((start, last))
            start = None
    if start is not None:
        runs.append((start, last))
    return runs


def test_ranking_reads_are_a_chunk_ahead_of_their_wait(loops):
    for ch, loop in sorted(loops.items()):
        runs = _read_runs(loop)
        # the 4 parts of a tile: those of slot 0 are issued ahead of the loop's first MFMA, every other one inside it
        assert runs, ch
        for start, last in runs:
            mfma = 0
            for op, rest in loop[last + 1:]:
                if op == "s_waitcnt" and "lgkmcnt" in rest:
                    break
                mfma += op.startswith("v_mfma")
            print("CH = %d: reads at %d..%d, %d v_mfma before the next lgkmcnt wait" % (ch, start, last, mfma))
            assert mfma >= 16, (ch, start, mfma)


def test_no_exec_mask_branch_in_the_main_loop(loops):
    for ch, loop in sorted(loops.items()):
        bad = [op for op, _ in loop if op in ("s_cbranch_execz", "s_cbranch_execnz")]
        assert not bad, (ch, bad)


def _dest_registers(rest):
    """The VGPRs an LDS read writes: its first operand, v7 or v[7:8]."""
    dst = rest.split(",")[0].strip()
    m = re.match(r"^v\[(\d+):(\d+)\]$", dst)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^v(\d+)$", dst)
    assert m, rest
    return {int(m.group(1))}


def test_parts_sharing_a_slot_have_their_own_registers(loops):
    """CH = 1: slot 1 (the second block's only chunk) carries parts 2 and 3.  Their 2 x 4 ds_read2st64_b32 and the reads of
    the tag, filters and floors are all in flight across that chunk: no two of them may write the same register."""
    loop = loops[1]
    runs = _read_runs(loop)
    assert len(runs) == 1, runs
    start, last = runs[0]
    end = next(i for i in range(last, len(loop)) if loop[i][0].startswith("v_mfma"))
    reads = [(op, rest) for op, rest in loop[start:end] if op.startswith("ds_read")]
    assert sum(op == "ds_read2st64_b32" for op, _ in reads) == 8, reads
    seen = set()
    for op, rest in reads:
        regs = _dest_registers(rest)
        assert not (regs & seen), (op, rest)
        seen |= regs
    assert len(seen) >= 2 * 8 + 3, sorted(seen)   # 16 partials; the shared row tag and the two queries' filters and floors
