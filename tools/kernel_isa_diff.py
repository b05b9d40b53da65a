"""Compare what two builds emit for the same kernels: two assembly listings of one source (hipcc ... -S), kernel by
kernel.

  python tools/kernel_isa_diff.py A.s B.s [name-regex] [--full] [--classes v_mfma,ds_read,...] [--window loop|all]

For every kernel symbol (mangled or demangled name) matching the regex and present in both listings it prints,
for each side, the opcode histogram (only the rows that differ unless --full), the opcode sequence of the
chosen classes inside the loop window -- from the first staging or LDS-DMA load (the first buffer_load* /
global_load* outside the ;;wg-partial markers) to the kernel's last s_barrier, the window
tools/check_wgrad_operands.py delimits -- run-length encoded, and the "; Kernel info:" figures.
--window all takes the whole kernel body as the window: for kernels whose last barrier precedes their main
loops (k_bres, k_critic_update, k_trunk3), which the loop window would cut off before them.

Opcodes are classified by prefix only (v_mfma, buffer_load, global_load, ds_read, ds_write, s_barrier,
s_waitcnt).  Exit status 1 when, for some kernel, B differs from A in
  - the count of any opcode of a chosen class,
  - the window's sequence of chosen-class opcodes,
  - Occupancy or LDSByteSize, a ScratchSize above 0 where A's is 0, or NumVgprs + NumAgprs above A's;
every other difference (other opcodes, register numbering, code length) is only listed.  The window shows the chosen
classes only: to look at what else moved inside it, widen them, e.g. --classes v_,s_,ds_,buffer_,global_ (every
opcode), and read the sequence diff.
"""
import collections
import difflib
import re
import subprocess
import sys

CLASSES = ("v_mfma", "buffer_load", "global_load", "ds_read", "ds_write", "s_barrier", "s_waitcnt")
INFO = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy", "LDSByteSize", "codeLenInByte")


def kernels(path):
    """{symbol: (opcodes of the body, info dict)} of every .amdhsa kernel of a listing."""
    lines = open(path).read().split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", l) for l in lines) if m}
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(\S+):", lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        name, ops, inpart = m.group(1), [], False
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            t = lines[i].strip()
            inpart = (inpart or ";;wg-partial-begin" in t) and ";;wg-partial-end" not in t
            if t and not t.startswith((";", ".")) and not t.endswith(":"):
                ops.append((t.split()[0], inpart))
            i += 1
        info = {}
        while i < len(lines) and "; Kernel info:" not in lines[i]:
            i += 1
        for l in lines[i:i + 40]:
            m = re.match(r";\s*(\w+)\s*[:=]\s*(\d+)", l)
            if m and m.group(1) in INFO:
                info.setdefault(m.group(1), int(m.group(2)))
        out[name] = (ops, info)
    return out


def cls(op, classes):
    return next((c for c in classes if op.startswith(c)), None)


def window(ops, classes, whole=False):
    if whole:
        return [o for o, _ in ops if cls(o, classes)]
    first = next((i for i, (o, part) in enumerate(ops) if o.startswith(("buffer_load", "global_load")) and not part), None)
    last = max((i for i, (o, _) in enumerate(ops) if o.startswith("s_barrier")), default=None)
    if first is None or last is None or last < first:
        return []
    return [o for o, _ in ops[first:last + 1] if cls(o, classes)]


def rle(seq):
    out = []
    for o in seq:
        if out and out[-1][0] == o:
            out[-1][1] += 1
        else:
            out.append([o, 1])
    return [f"{o} x{n}" if n > 1 else o for o, n in out]


def main():
    argv = sys.argv[1:]
    full = "--full" in argv
    classes = CLASSES
    if "--classes" in argv:
        i = argv.index("--classes")
        if i + 1 >= len(argv):
            sys.exit("--classes takes a comma-separated list of opcode prefixes")
        classes = tuple(argv[i + 1].split(","))
        del argv[i:i + 2]
    whole = False
    if "--window" in argv:
        i = argv.index("--window")
        if i + 1 >= len(argv) or argv[i + 1] not in ("loop", "all"):
            sys.exit("--window takes loop or all")
        whole = argv[i + 1] == "all"
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    if len(args) < 2:
        sys.exit(__doc__)
    rx = re.compile(args[2] if len(args) > 2 else ".")
    ka, kb = kernels(args[0]), kernels(args[1])
    both = list(dict.fromkeys([*ka, *kb]))
    dem = dict(zip(both, subprocess.run(["c++filt"], input="\n".join(both), capture_output=True, text=True).stdout.split("\n")))
    bad = 0
    for name in ka:
        if not (rx.search(name) or rx.search(dem[name])):
            continue
        print(f"== {dem[name][:110]}")
        if name not in kb:
            print("   only in A")
            bad += 1
            continue
        (oa, ia), (ob, ib) = ka[name], kb[name]
        ha, hb = collections.Counter(o for o, _ in oa), collections.Counter(o for o, _ in ob)
        why = []
        print(f"   instructions {len(oa)} -> {len(ob)}")
        for op in sorted(set(ha) | set(hb)):
            c = cls(op, classes)
            if full or ha[op] != hb[op]:
                print(f"   {'*' if c else ' '} {op:40s} {ha[op]:6d} {hb[op]:6d}")
            if c and ha[op] != hb[op]:
                why.append(f"count of {op}")
        print("   classes: " + ", ".join(
            f"{c} {sum(n for o, n in ha.items() if cls(o, classes) == c)}/{sum(n for o, n in hb.items() if cls(o, classes) == c)}"
            for c in classes))
        wa, wb = window(oa, classes, whole), window(ob, classes, whole)
        if wa == wb:
            print(f"   window: equal ({len(wa)} instructions of the chosen classes)")
            if full:
                print("      " + "; ".join(rle(wa)))
        else:
            why.append("window sequence")
            for l in difflib.unified_diff(rle(wa), rle(wb), "A", "B", lineterm="", n=2):
                print("      " + l)
        print("   info: " + ", ".join(f"{k} {ia.get(k)}/{ib.get(k)}" for k in INFO))
        if ia.get("Occupancy") != ib.get("Occupancy"):
            why.append("Occupancy")
        if ia.get("LDSByteSize") != ib.get("LDSByteSize"):
            why.append("LDSByteSize")
        if ia.get("ScratchSize") == 0 and ib.get("ScratchSize", 0) > 0:
            why.append("ScratchSize")
        if ib.get("NumVgprs", 0) + ib.get("NumAgprs", 0) > ia.get("NumVgprs", 0) + ia.get("NumAgprs", 0):
            why.append("NumVgprs + NumAgprs above A's")
        if why:
            bad += 1
            print("   DIFFERS: " + ", ".join(why))
    for name in kb:
        if name not in ka and (rx.search(name) or rx.search(dem[name])):
            print(f"== {dem[name][:110]}\n   only in B")
            bad += 1
    print(f"{bad} kernel(s) differ in a chosen class")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
