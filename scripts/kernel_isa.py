#!/usr/bin/env python3
"""Per-kernel fingerprint of the gfx950 device code of a built tree.  Host only, no GPU.

    kernel_isa.py TREE            one line per kernel: object, symbol, sha1 of its disassembly, instruction count
    kernel_isa.py BEFORE AFTER    the kernels that differ, are missing or are new; exit 1 if there are any.  A missing
                                  kernel whose code reappears under a new symbol is reported as renamed, and is identical

TREE is the repository root (or its moc_amd/csrc) after `make`.  Every .hip object there is unbundled
(clang-offload-bundler), disassembled (llvm-objdump -d) and cut at the kernel symbols; addresses, encodings and
branch-target offsets are stripped, so a kernel whose code is the same hashes the same wherever it lands in the
object -- or in which object: the comparison is by symbol over the whole tree, and the line says when a kernel moved.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TARGET = "hip-amdgcn-amd-amdhsa--gfx950"
LABEL = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
TARGET_OFF = re.compile(r"<([^>+]+)\+0x[0-9a-f]+>")


def tool(name):
    p = os.path.join(ROCM, "llvm", "bin", name)
    return p if os.path.exists(p) else name


def csrc(tree):
    d = os.path.join(tree, "moc_amd", "csrc")
    return d if os.path.isdir(d) else tree


def kernels_of(obj, tmp):
    """{symbol: (sha1, instructions)} of one host object with a bundled device code object"""
    fb = os.path.join(tmp, os.path.basename(obj) + ".hipfb")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.check_call([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj])   # the bundle inside the host object
    subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                           "--input=" + fb, "--output=" + co])
    syms = subprocess.check_output([tool("llvm-readelf"), "--symbols", "--wide", co], text=True)
    # a kernel is a function with a kernel descriptor NAME.kd beside it
    kds = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.rstrip().endswith(".kd")}
    text = subprocess.check_output([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, name, lines = {}, None, []

    def close():
        while lines and lines[-1].split()[0] in ("s_nop", "s_code_end", "..."):
            lines.pop()                                             # padding behind a kernel depends on where it lies
        if name in kds:
            out[name] = (hashlib.sha1("\n".join(lines).encode()).hexdigest()[:16], len(lines))

    for ln in text.splitlines():
        m = LABEL.match(ln.strip())
        if m:
            if not m.group(1).startswith("L"):                      # a function, not a local label
                close()
                name, lines = m.group(1), []
            continue
        ln = ln.split("//")[0].strip()                              # "// 0000001234: BF8C0000" trails every instruction
        if name is None or not ln:
            continue
        lines.append(TARGET_OFF.sub(r"<\1>", ln))
    close()
    assert set(out) == kds, (obj, sorted(kds - set(out)))
    return out


def tree_kernels(tree):
    """{symbol: [(object, sha1, instructions), ...]} over every .hip object of the tree"""
    d = csrc(tree)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in sorted(f for f in os.listdir(d) if f.endswith(".hip")):
            obj = os.path.join(d, src[:-4] + ".o")
            if not os.path.exists(obj):
                sys.exit("%s: not built (run make in %s)" % (obj, d))
            for sym, (h, n) in kernels_of(obj, tmp).items():
                res.setdefault(sym, []).append((src[:-4], h, n))
    return res


def main(argv):
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    a = tree_kernels(argv[1])
    if len(argv) == 2:
        for sym in sorted(a, key=lambda s: (a[s][0][0], s)):
            for o, h, n in a[sym]:
                print("%-12s %s %6d  %s" % (o, h, n, sym))
        print("%d kernels" % sum(len(v) for v in a.values()))
        return 0
    b = tree_kernels(argv[2])
    na, nb = sum(map(len, a.values())), sum(map(len, b.values()))
    bad = moved = renamed = 0
    # a symbol that is gone and a new one with the same code (hash and instruction count): the kernel was renamed, e.g.
    # because a type in its signature changed namespace.  Paired in symbol order, each new symbol at most once.
    fresh = sorted(s for s in set(b) - set(a) if len(b[s]) == 1)
    for old in sorted(s for s in set(a) - set(b) if len(a[s]) == 1):
        new = next((s for s in fresh if b[s][0][1:] == a[old][0][1:]), None)
        if new is not None:
            fresh.remove(new)
            renamed += 1
            print("renamed  %s -> %s  (%s -> %s)" % (old, new, a[old][0][0], b[new][0][0]))
            del a[old], b[new]
    for sym in sorted(set(a) | set(b)):
        va, vb = a.get(sym, []), b.get(sym, [])
        if len(va) != 1 or len(vb) != 1:
            what = "missing" if not vb else "new" if not va else "duplicated"
        elif va[0][1:] != vb[0][1:]:
            what = "differs (%d -> %d instructions)" % (va[0][2], vb[0][2])
        else:
            if va[0][0] != vb[0][0]:
                moved += 1
                print("moved    %s -> %s  %s" % (va[0][0], vb[0][0], sym))
            continue
        bad += 1
        print("%-8s %s  %s" % (what, ",".join(o for o, _, _ in va + vb), sym))
    print("kernel_isa: %d kernels before, %d after: %d identical (%d of them moved, %d renamed), %d differ / missing / new"
          % (na, nb, len(set(a) | set(b)) - bad + renamed, moved, renamed, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
