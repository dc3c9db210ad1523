"""Static counts around the in-edge coefficient picks, read from the compiler's assembly.

Compiles each tree's swarm_tick.hip and swarm_td.hip for gfx950 with build.FLAGS (device code only,
no GPU needed) and reports, per tree, for the fused tick's headline instance, its 16-slot instance
and td_kernel's 32-slot instance (complete graph + GAT):
  - total instructions, exec-mask regions (s_*_saveexec_b64), branches (s_cbranch_*), packed f32 ops;
  - per forward (dl_forward: the TD part's, and for a tick the acting part's): instructions, exec-mask
    regions and branches between the first and the last MFMA of its aggregate.  A forward is found in
    the text as: the score sums' permlane swaps, then the softmax's v_exp_f32, then the aggregate's
    2 CT NS / 4 MFMAs (the first MFMAs behind the softmax);
  - B1 -> B2: the first barrier-to-barrier stretch behind the TD forward that stores 16-B rows (the
    dQ/dZ products and the dZ / X / cm / dO / dp images; B1 itself may stand in the text twice, once
    per wave kind, and the stretch in front of the online waves' copy stores no row);
  - per bwd_attention instance and target tile: from the first MFMA of g's chain (the last 8 CT
    MFMAs in front of permlane swaps that no softmax follows) to the last of those swaps (Gs, da_dst);
  - VGPRs, scratch bytes and occupancy of the kernel's metadata.
These are counts of the text, every path included, not of one wave's execution.

usage: python tools/picks_isa.py [LABEL=]TREE [[LABEL=]TREE ...] [--extra=-fno-slp-vectorize ...]
(a tree is reported under its label, or under the path as given)
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

# (translation unit, mangled-name substring, label, aggregate MFMAs of the TD forward, of the acting forward)
KERNELS = (("swarm_tick.hip", "tick_kernelILi8ELi16ELi8ELi0ELi1EE", "tick_kernel<8,16,8,GoTo,complete+GAT>", 8, 4),
           ("swarm_tick.hip", "tick_kernelILi16ELi16ELi16ELi1ELi1EE", "tick_kernel<16,16,16,OA,complete+GAT>", 8, 8),
           ("swarm_td.hip", "td_kernelILi32ELi32ELi1EE", "td_kernel<32,32,complete+GAT>", 32, None))
INSTR = re.compile(r"^\t(s_|v_|ds_|global_|buffer_|flat_|scratch_)")


def assembly(tree, src, extra):
    csrc = glob.glob(os.path.join(tree, "*", "csrc"))[0]
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory(prefix="picks_isa_") as tmp:
        out = os.path.join(tmp, src + ".s")
        p = subprocess.run([B.HIPCC, *flags, *extra, '-DSWARM_SRC_DIGEST="picks_isa"', "--cuda-device-only", "-S", "-o", out,
                            os.path.join(csrc, src)], capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit(f"hipcc failed on {src} of {tree}:\n{p.stderr[-4000:]}")
        with open(out) as f:
            return f.read().splitlines()


def kernel_text(lines, name):
    start = next(i for i, ln in enumerate(lines)
                 if ln.startswith("_Z") and name in ln and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [ln for ln in lines[start:end] if INSTR.match(ln)], "\n".join(lines[end:end + 150])


def counts(text):
    return {"instructions": len(text), "exec_regions": sum("_saveexec_b64" in ln for ln in text),
            "branches": sum("s_cbranch" in ln for ln in text)}


def fmt(c):
    return f"{c['instructions']} instructions, {c['exec_regions']} exec-mask regions, {c['branches']} branches"


def kind(ln):
    for k in ("v_mfma", "v_permlane", "v_exp_f32", "s_barrier"):
        if k in ln:
            return k
    return None


def forwards(text, n_aggs):
    """[(first, last)] instruction indices of the aggregate's first and last MFMA, per forward"""
    found, state, i = [], "", 0
    while i < len(text) and len(found) < len(n_aggs):
        k = kind(text[i])
        if k == "v_permlane":
            state = "scores"
        elif k == "v_exp_f32" and state in ("scores", "softmax"):
            state = "softmax"
        elif k == "v_mfma":
            if state == "softmax":
                n, j = n_aggs[len(found)], i
                idx = []
                while len(idx) < n:
                    if kind(text[j]) == "v_mfma":
                        idx.append(j)
                    j += 1
                found.append((idx[0], idx[-1]))
                i = idx[-1]
            state = ""
        i += 1
    return found


def attention_segments(text, stop, n_g):
    """[(first, last)]: the last n_g MFMAs of an MFMA run (g's chain of one target tile) and the
    permlane swaps that follow it (Gs and da_dst), with no softmax behind them (that is a forward)"""
    ev = [(i, kind(ln)) for i, ln in enumerate(text[:stop]) if kind(ln)]
    runs = []   # [kind, instruction indices]
    for i, k in ev:
        if runs and runs[-1][0] == k and k != "s_barrier":
            runs[-1][1].append(i)
        else:
            runs.append([k, [i]])
    runs.append(["end", []])
    out = []
    for a, b, c in zip(runs, runs[1:], runs[2:]):
        if a[0] == "v_mfma" and b[0] == "v_permlane" and c[0] != "v_exp_f32" and len(a[1]) >= n_g:
            out.append((a[1][-n_g], b[1][-1]))
    return out


def report(label, tree, extra):
    print(f"== {label}" + (f", extra flags {' '.join(extra)}" if extra else ""))
    asm = {}
    for src, name, label, n_td, n_act in KERNELS:
        if src not in asm:
            asm[src] = assembly(tree, src, extra)
        text, tail = kernel_text(asm[src], name)
        print(f" {label}")
        print(f"  kernel: {fmt(counts(text))}, {sum('v_pk_' in ln and '_f32' in ln for ln in text)} v_pk_*_f32")
        for key, pat in (("VGPRs", r"; NumVgprs: (\d+)"), ("scratch bytes", r"; ScratchSize: (\d+)"),
                         ("occupancy (waves per SIMD)", r"; Occupancy: (\d+)")):
            print(f"  {key}: {re.search(pat, tail).group(1)}")
        fw = forwards(text, [n_td] + ([n_act] if n_act else []))
        for side, (a, b) in zip(("TD forward", "acting forward"), fw):
            print(f"  {side}: aggregate, first to last MFMA: {fmt(counts(text[a:b + 1]))}")
        bars = [i for i, ln in enumerate(text) if "s_barrier" in ln and i > fw[0][1]]
        a, b = next((a, b) for a, b in zip(bars, bars[1:]) if any("ds_write_b128" in ln for ln in text[a:b]))
        print(f"  B1 -> B2: {fmt(counts(text[a:b + 1]))}")
        act_start = fw[1][0] if len(fw) > 1 else len(text)
        # the instances lie in the TD part, behind its forward and in front of the acting part
        n_g = n_td // 4 if n_td == 32 else 8   # 8 CT MFMAs per target tile
        for n, (a, b) in enumerate(x for x in attention_segments(text, act_start, n_g) if x[0] > fw[0][1]):
            print(f"  bwd_attention, g chain to da_dst, tile {n}: {fmt(counts(text[a:b + 1]))}")


def main():
    extra = [a[len("--extra="):] for a in sys.argv[1:] if a.startswith("--extra=")]
    for arg in [a for a in sys.argv[1:] if not a.startswith("--")]:
        label, sep, tree = arg.partition("=")
        report(label, tree if sep else label, extra)


if __name__ == "__main__":
    main()
