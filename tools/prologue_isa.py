"""Static counts of the fused tick's learning prologue, read from the compiler's assembly.

Compiles one tree's swarm_tick.hip for gfx950 with build.FLAGS (device code only, no GPU needed)
and reports, for one tick_kernel instance (default: the headline's, GoTo <= 8 agents, complete
graph + GAT), the two prologues as they stand in the text:
  acting: from the acting entry (the target of the kernel's first scalar branch, blockIdx < n_act)
          to the weight-image barrier (the first s_barrier behind a ds_write_b128);
  TD:     from the kernel's start to its B0 barrier (same rule).
Per prologue:
  arrival -> barrier : instructions from the last s_waitcnt vmcnt in front of the clip norm's wave
                       sum (its first row_mirror DPP add) to the barrier, and the exec-mask regions
                       (s_*_saveexec_b64) among them.  These are counts of the text, every path
                       included (both norm forms, block 0's stores), not of one wave's execution;
  kernarg s_loads    : scalar loads from the kernarg segment (base s[0:1]) between the first
                       s_waitcnt lgkmcnt(0) and the barrier;
and for the kernel: VGPRs, SGPR-spill v_writelanes, scratch bytes and code bytes.

usage: python tools/prologue_isa.py TREE [MANGLED_KERNEL_SUBSTRING]
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swarm_amd  # noqa: E402,F401  (shim registers the package)
from swarm_amd import build as B  # noqa: E402

HEADLINE = "tick_kernelILi8ELi16ELi8ELi0ELi1EE"
INSTR = re.compile(r"^\t(s_|v_|ds_|global_|buffer_|flat_|scratch_)")


def assembly(tree):
    csrc = glob.glob(os.path.join(tree, "*", "csrc"))[0]
    out = os.path.join(tempfile.mkdtemp(prefix="prologue_isa_"), "tick.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([B.HIPCC, *flags, '-DSWARM_SRC_DIGEST="prologue_isa"', "--cuda-device-only", "-S", "-o", out,
                    os.path.join(csrc, "swarm_tick.hip")], check=True, stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def kernel_text(lines, name):
    start = next(i for i, ln in enumerate(lines) if ln.startswith("_Z") and name in ln and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    tail = "\n".join(lines[end:end + 150])
    return lines[start:end], tail


def prologue(text):
    """counts of one prologue: text from its entry up to and including its weight barrier"""
    wrote = False
    for bar, ln in enumerate(text):
        wrote = wrote or "ds_write_b128" in ln
        if wrote and "s_barrier" in ln:
            break
    text = text[:bar + 1]
    mirror = next(i for i, ln in enumerate(text) if "row_mirror" in ln)
    arrival = max(i for i in range(mirror) if "s_waitcnt vmcnt" in text[i])
    first_wait = next(i for i, ln in enumerate(text) if "s_waitcnt lgkmcnt(0)" in ln)
    stretch = text[arrival + 1:]
    return {"entry_to_barrier_instructions": sum(1 for ln in text if INSTR.match(ln)),
            "arrival_to_barrier_instructions": sum(1 for ln in stretch if INSTR.match(ln)),
            "arrival_to_barrier_exec_regions": sum(1 for ln in stretch if "_saveexec_b64" in ln),
            "kernarg_s_loads_first_wait_to_barrier": sum(1 for ln in text[first_wait:] if re.search(r"s_load_dword\w* .*, s\[0:1\],", ln))}


def main():
    tree = sys.argv[1]
    name = sys.argv[2] if len(sys.argv) > 2 else HEADLINE
    text, tail = kernel_text(assembly(tree), name)
    label = next(re.search(r"(\.LBB\d+_\d+)", ln).group(1) for ln in text if "s_cbranch_scc" in ln)
    act = next(i for i, ln in enumerate(text) if ln.startswith(label + ":"))
    print(f"kernel {name} of {os.path.abspath(tree)}")
    for key, pat in (("VGPRs", r"; NumVgprs: (\d+)"), ("scratch bytes", r"; ScratchSize: (\d+)"),
                     ("code bytes", r"; codeLenInByte = (\d+)")):
        print(f"  {key}: {re.search(pat, tail).group(1)}")
    print(f"  SGPR-spill v_writelane: {sum(1 for ln in text if 'v_writelane_b32' in ln)}")
    for side, t in (("acting", text[act:]), ("TD", text[:act])):
        for k, v in prologue(t).items():
            print(f"  {side}: {k}: {v}")


if __name__ == "__main__":
    main()
