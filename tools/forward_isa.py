"""Static counts of the forward's LDS waits and reads, read from the compiler's assembly.

For the three kernels tools/picks_isa.py names (the fused tick's headline instance, its 16-slot
instance and td_kernel's 32-slot instance, complete graph + GAT), per forward (dl_forward: the TD
part's, and for a tick the acting part's):
  - between the first MFMA of lin0 and the last MFMA of lin2: the `s_waitcnt` instructions that
    wait on lgkmcnt and the `ds_read*` instructions, in three stretches:
      lin0 + scores + coefficients   first MFMA of lin0 .. first MFMA of the aggregate
      aggregate                      .. last MFMA of the aggregate
      epilogue + lin1 + lin2         .. last MFMA of lin2
    The first two stretches read the scores and the H rows of other nodes (state-dependent LDS
    reads that stay); the weight image is what is left once those are set aside, and the third
    stretch reads nothing else (in the headline kernel: plus the deferred pair geometry's four
    position reads, the forward's hook);
  - the Q epilogue, from the last MFMA of lin2 to the Q read-back (the first LDS read behind it
    that another LDS read follows with no LDS write between them: a row is read back in several
    pieces, a bias word read is followed by its Q word's store): exec-mask regions
    (s_*_saveexec_b64), ds_read* and ds_write* instructions;
  - VGPRs, scratch bytes and occupancy of the kernel's metadata.
A forward is found as picks_isa finds it (score sums' permlane swaps, softmax's v_exp_f32, the
aggregate's MFMAs); lin0's 4 CT MFMAs are the last in front of the aggregate, lin1's 16 CT and
lin2's 8 CT the first behind it.  These are counts of the text's opcodes, every path included, not
of one wave's execution, and no timing.  The windows are found by counting, not by understanding the
code: the tool stops with a message where a walk runs out of MFMAs or crosses a block barrier, or
finds no read-back in front of the next MFMA or barrier; a window that moved inside those limits
is not detected, so read the instruction totals beside the counts.

usage: python tools/forward_isa.py [LABEL=]TREE [[LABEL=]TREE ...]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picks_isa as PI  # noqa: E402

# column tiles of the TD forward, of the acting forward, per picks_isa.KERNELS row
TILES = ((1, 1), (1, 1), (2, None))


def window(text, agg, ct):
    """instruction indices (first MFMA of lin0, first of the aggregate, last of the aggregate, last of lin2)"""
    a, b = agg
    i, n = a, 0
    while n < 4 * ct and i > 0:
        i -= 1
        n += "v_mfma" in text[i]
    j, m = b, 0
    while m < 24 * ct and j < len(text) - 1:
        j += 1
        m += "v_mfma" in text[j]
    # the walks count MFMAs only: a block barrier inside the window (a forward has none) means
    # they left the forward
    if n < 4 * ct or m < 24 * ct or any("s_barrier" in ln for ln in text[i:j + 1]):
        raise SystemExit("forward_isa: lin0 / lin1 / lin2 are not where the MFMA counts put them; the code "
                         "generation moved and the windows need a new description")
    return i, a, b, j


def lds(text):
    return {"waits": sum(ln.startswith("\ts_waitcnt") and "lgkmcnt" in ln for ln in text),
            "reads": sum(ln.startswith("\tds_read") for ln in text)}


def report(label, tree):
    print(f"== {label}")
    asm = {}
    for (src, name, klabel, n_td, n_act), (ct_td, ct_act) in zip(PI.KERNELS, TILES):
        if src not in asm:
            asm[src] = PI.assembly(tree, src, [])
        text, tail = PI.kernel_text(asm[src], name)
        print(f" {klabel}")
        print("  " + ", ".join(f"{key} {re.search(pat, tail).group(1)}" for key, pat in
                               (("VGPRs", r"; NumVgprs: (\d+)"), ("scratch bytes", r"; ScratchSize: (\d+)"),
                                ("occupancy", r"; Occupancy: (\d+)"))) + f", {len(text)} instructions")
        fw = PI.forwards(text, [n_td] + ([n_act] if n_act else []))
        for side, agg, ct in zip(("TD forward", "acting forward"), fw, (ct_td, ct_act)):
            w = window(text, agg, ct)
            parts = [lds(text[w[k]:w[k + 1] + 1]) for k in range(3)]
            total = lds(text[w[0]:w[3] + 1])
            print(f"  {side}: lin0 first MFMA .. lin2 last MFMA: {w[3] - w[0] + 1} instructions, "
                  f"{total['waits']} lgkmcnt waits, {total['reads']} ds_read")
            for nm, c in zip(("lin0 + scores + coefficients", "aggregate", "epilogue + lin1 + lin2"), parts):
                print(f"    {nm}: {c['waits']} lgkmcnt waits, {c['reads']} ds_read")
            ds = [i for i in range(w[3], len(text)) if text[i].startswith("\tds_")]
            e = next((i for i, j in zip(ds, ds[1:]) if text[i].startswith("\tds_read") and text[j].startswith("\tds_read")),
                     None)
            if e is None or any("v_mfma" in ln or "s_barrier" in ln for ln in text[w[3] + 1:e]):
                raise SystemExit("forward_isa: no Q read-back found behind lin2 (two LDS reads in a row in front of "
                                 "the next MFMA or barrier)")
            epi = text[w[3]:e]
            print(f"    Q epilogue (lin2 last MFMA .. Q read-back): {len(epi)} instructions, "
                  f"{sum('_saveexec_b64' in ln for ln in epi)} exec-mask regions, {lds(epi)['reads']} ds_read, "
                  f"{sum(ln.startswith(chr(9) + 'ds_write') for ln in epi)} ds_write "
                  f"({sum(ln.startswith(chr(9) + 'ds_write_b128') for ln in epi)} of 16 B)")


def main():
    for arg in [a for a in sys.argv[1:] if not a.startswith("--")]:
        label, sep, tree = arg.partition("=")
        report(label, tree if sep else label)


if __name__ == "__main__":
    main()
