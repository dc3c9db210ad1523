"""Do two source trees compile to the same gfx950 device code?

For each translation unit of the library (build.SOURCES) both trees' source is compiled device-only
with this tree's build.FLAGS and one fixed SWARM_SRC_DIGEST, the gfx950 object is unbundled, and the
two objects are compared by names and bytes only (no instruction is inspected):
  - the sorted lists of .text function symbols (which kernels exist);
  - per symbol, its code bytes (address and size into .text; its position may differ, so the
    4-byte fields the linker relocated, a call's pc-relative offset to another function, are
    compared as (offset in the symbol, relocation type, target) instead of as bytes);
  - per kernel, its metadata note: VGPR / SGPR / AGPR counts, LDS, scratch and kernarg sizes;
  - per kernel, the occupancy (waves per SIMD) of the compiler's kernel-resource-usage remarks.
A host-side refactor must leave all of them equal: the kernels cannot tell who launched them.  A
kernel refactor may move code bytes and register counts; its LDS, scratch, kernarg and occupancy stay.

usage: python tools/codeobj_diff.py TREE_A TREE_B [--extra=-DSWARM_STAMPS=1 ...] [--keep DIR]
Translation units that only one tree has are named and left out of the comparison.
Exit status 0 when every translation unit both trees have is identical, 1 otherwise.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swarm_amd  # noqa: E402,F401  (shim registers the package)
from swarm_amd import build as B  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B.HIPCC))), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
             "kernarg_segment_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def compile_start(tree, src, extra, out):
    """the compiler's own resource remarks (registers, occupancy) of the unit go to out + '.remarks'"""
    csrc = glob.glob(os.path.join(tree, "*", "csrc"))[0]
    flags = [f for f in B.FLAGS if f != "-shared"]
    with open(out + ".remarks", "w") as err:
        return subprocess.Popen([B.HIPCC, *flags, '-DSWARM_SRC_DIGEST="codeobj_diff"', *extra, "--cuda-device-only", "-c",
                                 "-Rpass-analysis=kernel-resource-usage", "-Xoffload-linker", "--emit-relocs", "-o", out,
                                 os.path.join(csrc, src)], stderr=err)


def occupancy(obj):
    """{kernel: waves per SIMD} as the compiler printed them for obj"""
    text = open(obj + ".remarks").read()
    return dict(re.findall(r"Function Name: (\S+).*\n(?:.*\n)*?.*Occupancy \[waves/SIMD\]: (\d+)", text))


def describe(obj):
    """{symbol: (code bytes with relocated fields zeroed, relocations, metadata note or None)} of the
    gfx950 object bundled in obj"""
    co, text = obj + ".co", obj + ".text"
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={obj}", f"--output={co}")
    tool("llvm-objcopy", "-O", "binary", "--only-section=.text", co, text)
    base = next(int(ln.split()[3], 16) for ln in tool("llvm-objdump", "-h", co).splitlines()
                if len(ln.split()) > 3 and ln.split()[1] == ".text")
    code = open(text, "rb").read()
    notes, cur = {}, None
    for ln in tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^  (- |  )\.(\w+):\s+(\S+)$", ln)   # kernel-level keys; a kernel's args sit deeper
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is not None and m.group(2) in NOTE_KEYS:
            cur[m.group(2)] = m.group(3)
        elif cur is not None and m.group(2) == "name":
            notes[m.group(3)] = cur
    funcs = []   # (address in .text, size, name)
    for ln in tool("llvm-objdump", "-t", co).splitlines():
        f = ln.split()
        if ".text" in f[2:] and "F" in f[1:f.index(".text")]:   # addr flags.. F .text size [.protected] name
            funcs.append((int(f[0], 16) - base, int(f[f.index(".text") + 1], 16), f[-1]))

    def where(addr):   # position-independent name of a .text address
        return next((f"{n}+{addr - a}" for a, sz, n in funcs if a <= addr < a + sz), None)

    code, relocs, in_text = bytearray(code), {n: [] for _, _, n in funcs}, False
    for ln in tool("llvm-readelf", "-r", co).splitlines():
        f = ln.split()
        if ln.startswith("Relocation section"):
            in_text = "'.rela.text'" in ln
        elif in_text and len(f) >= 7 and f[2].startswith("R_AMDGPU"):
            off, target = int(f[0], 16) - base, int(f[3], 16) + int(f[-1], 16) * (-1 if f[-2] == "-" else 1)
            code[off:off + 4] = bytes(4)
            relocs[where(off).split("+")[0]].append((where(off), f[2], where(target - base) or " ".join(f[4:])))
    syms = {n: (bytes(code[a:a + sz]), relocs[n], notes.get(n)) for a, sz, n in funcs}
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--extra", action="append", default=[], help="extra compiler flag (repeatable)")
    ap.add_argument("--keep", help="directory for the objects (default: a temporary one)")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="codeobj_diff_")
    os.makedirs(tmp, exist_ok=True)
    def has(tree, src):
        return os.path.exists(os.path.join(glob.glob(os.path.join(tree, "*", "csrc"))[0], src))
    # translation units both trees have are compared; one that only one tree has is new (or gone)
    sources = [s for s in B.SOURCES if has(a.tree_a, s) and has(a.tree_b, s)]
    for s in B.SOURCES:
        if s not in sources:
            print(f"{s}: only in tree {'A' if has(a.tree_a, s) else 'B'} (not compared)")
    objs = {(t, s): os.path.join(tmp, f"{t}_{os.path.splitext(s)[0]}.o") for t in "ab" for s in sources}
    procs = [compile_start(a.tree_a if t == "a" else a.tree_b, s, a.extra, o) for (t, s), o in objs.items()]
    if any(p.wait() != 0 for p in procs):
        raise SystemExit("hipcc failed")
    print(f"codeobj_diff flags: {' '.join(B.FLAGS)} --cuda-device-only -Xoffload-linker --emit-relocs "
          f"{' '.join(a.extra)}".rstrip())
    same = True
    for s in sources:
        da, db = describe(objs["a", s]), describe(objs["b", s])
        names = sorted(set(da) & set(db))
        code = [n for n in names if da[n][:2] != db[n][:2]]
        note = [n for n in names if da[n][2] != db[n][2]]
        kernels = sum(1 for n in names if da[n][2] is not None)
        oa, ob = occupancy(objs["a", s]), occupancy(objs["b", s])
        occ = [n for n in names if oa.get(n) != ob.get(n)]
        ok = sorted(da) == sorted(db) and not code and not note and not occ
        same = same and ok
        print(f"{s}: {len(da)} / {len(db)} .text functions ({kernels} kernels with a metadata note), symbol lists "
              f"{'identical' if sorted(da) == sorted(db) else 'DIFFER'}, code bytes "
              f"{'identical' if not code else 'DIFFER'}, kernel metadata {'identical' if not note else 'DIFFER'}, "
              f"occupancy {'identical' if not occ else 'DIFFER'}")
        for n in sorted(set(da) ^ set(db)):
            print(f"  only in {'A' if n in da else 'B'}: {n}")
        for n in code:
            print(f"  code differs: {n} ({len(da[n][0])} / {len(db[n][0])} bytes)")
        for n in note:
            print(f"  metadata differs: {n}: {da[n][2]} / {db[n][2]}")
        for n in occ:
            print(f"  occupancy differs: {n}: {oa.get(n)} / {ob.get(n)} waves per SIMD")
        for n in names:   # tree A: size, relocated fields, the note in NOTE_KEYS order, waves per SIMD
            print(f"  = {len(da[n][0]):7d} B {len(da[n][1]):2d} rel  {da[n][2] and ' '.join(da[n][2][k] for k in NOTE_KEYS)}"
                  f"  occ {oa.get(n)}  {n}")
    print("IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
