"""Static instruction counts of one k_chain instantiation, from the compiler's assembly listing.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S v2e_amd/csrc/emu.hip -o emu.s
    python scripts/chain_isa_count.py emu.s [mangled-name substring, default k_chainIdhLb0ELb1E] [--dump first:last]

Prints one line per basic block (label to label) of the kernel: its instructions and how many of them are VALU, SALU,
v_readlane, LDS reads, buffer loads / stores, global stores, float64 floors (one per frame body) and waits -- enough to tell
the unrolled light sub-pass (8 floors in one block) and the boundary behind it apart and to count what each part costs.
--dump prints the instructions of blocks first..last, for counting a part of a block by hand."""
import re
import sys


def kernel_lines(path, key):
    out, on = [], False
    for ln in open(path):
        if not on:
            if re.match(r"^_Z\w*%s\w*:" % re.escape(key), ln):
                on = True
            continue
        if ln.startswith(".Lfunc_end") or re.match(r"^\s+\.end_amdhsa_kernel", ln):
            break
        out.append(ln.rstrip("\n"))
    return out


def classify(op):
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
        return "rdl"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ldsr"
    if op.startswith("ds_"):
        return "ldsw"
    if op.startswith("buffer_load"):
        return "bufl"
    if op.startswith("buffer_store"):
        return "bufs"
    if op.startswith("global_store") or op.startswith("flat_store"):
        return "gst"
    if op.startswith("global_") or op.startswith("flat_"):
        return "gld"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def blocks(lines):
    cur, name = [], "entry"
    for ln in lines:
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith("."):
            m = re.match(r"^(\.LBB\w+):", s)
            if m:
                yield name, cur
                cur, name = [], m.group(1)
            continue
        cur.append(s.split(";")[0].strip())
    yield name, cur


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dump = None
    if "--dump" in sys.argv:
        a, b = sys.argv[sys.argv.index("--dump") + 1].split(":")
        dump = (int(a), int(b))
        args = [x for x in args if x != sys.argv[sys.argv.index("--dump") + 1]]
    key = args[1] if len(args) > 1 else "k_chainIdhLb0ELb1E"
    kinds = ["valu", "salu", "rdl", "ldsr", "ldsw", "bufl", "bufs", "gld", "gst", "wait", "other"]
    print("%4s %-14s %5s " % ("#", "block", "inst") + " ".join("%5s" % k for k in kinds) + "  floor")
    total = 0
    for i, (name, ins) in enumerate(blocks(kernel_lines(args[0], key))):
        c = dict.fromkeys(kinds, 0)
        for s in ins:
            c[classify(s.split()[0])] += 1
        fl = sum(1 for s in ins if s.startswith("v_floor_f64") or s.startswith("v_floor_f32"))
        total += len(ins)
        print("%4d %-14s %5d " % (i, name, len(ins)) + " ".join("%5d" % c[k] for k in kinds) + "  %5d" % fl)
        if dump and dump[0] <= i <= dump[1]:
            for s in ins:
                print("        " + s)
    print("total instructions: %d" % total)


if __name__ == "__main__":
    main()
