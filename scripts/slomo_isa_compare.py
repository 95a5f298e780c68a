"""Two builds of v2e_amd/csrc/slomo.hip side by side, without a GPU: every kernel's resources, and the instruction mix of every
k_conv* kernel between its first and its last v_mfma.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage v2e_amd/csrc/slomo.hip -o X.s 2> X.remarks
    python scripts/slomo_isa_compare.py parent.s parent.remarks new.s new.remarks

Kernels are matched by their demangled name with k_conv_s3p's former second template argument dropped.  Part 1 fails a kernel
whose scratch or spills rose from zero, whose occupancy fell or whose LDS changed; part 2 fails one whose MFMA, LDS-read,
LDS-write, global-load or barrier count between the first and the last MFMA changed, and prints every other difference.  The
instruction classes are scripts/chain_isa_count.py's."""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chain_isa_count import blocks, classify, kernel_lines  # noqa: E402

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("sspill", "SGPRs Spill"),
          ("vspill", "VGPRs Spill"), ("occ", "Occupancy [waves/SIMD]"), ("LDS", "LDS Size [bytes/block]")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for m, d in zip(names, out):
        d = d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        short[m] = re.sub(r"^(k_conv_s3p<\d+), 0>", r"\1>", d).replace(" ", "")
    return short


def resources(path):
    res, cur = collections.OrderedDict(), None
    for ln in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def steady_mix(path, mangled):
    ins = [s.split()[0] for _, b in blocks(kernel_lines(path, mangled[2:])) for s in b]
    at = [i for i, op in enumerate(ins) if op.startswith("v_mfma")]
    c = collections.Counter()
    for op in (ins[at[0]:at[-1] + 1] if at else []):   # (k_conv3x3_small is a VALU kernel: nothing to count)
        c["mfma" if op.startswith("v_mfma") else ("barrier" if op == "s_barrier" else classify(op))] += 1
    return c


def main():
    ps, pr, ns, nr = sys.argv[1:5]
    rp, rn = resources(pr), resources(nr)
    dp, dn = demangle(list(rp)), demangle(list(rn))
    byname_p = {dp[m]: m for m in rp}
    byname_n = {dn[m]: m for m in rn}
    assert set(byname_p) == set(byname_n), sorted(set(byname_p) ^ set(byname_n))
    print("%-44s %s" % ("kernel", "  ".join("%11s" % f for f, _ in FIELDS)))
    bad = 0
    for name in sorted(byname_p):
        a, b = rp[byname_p[name]], rn[byname_n[name]]
        va, vb = {f: int(a[k]) for f, k in FIELDS}, {f: int(b[k]) for f, k in FIELDS}
        marks = []
        for f in ("scratch", "sspill", "vspill"):
            if va[f] == 0 and vb[f] != 0:
                marks.append("FAIL " + f)
        if vb["occ"] < va["occ"]:
            marks.append("FAIL occ")
        if vb["LDS"] != va["LDS"]:
            marks.append("FAIL LDS")
        bad += len(marks)
        marks += [f + "+" for f in ("VGPRs", "AGPRs") if vb[f] > va[f]]
        print("%-44s %s %s" % (name, "  ".join("%4d -> %4d" % (va[f], vb[f]) for f, _ in FIELDS), " ".join(marks)))
    print("kernels: %d (k_conv*: %d) violations: %d" % (len(byname_p), sum(n.startswith("k_conv") for n in byname_p), bad))
    print()
    must = ["mfma", "ldsr", "ldsw", "gld", "barrier"]
    bad2 = same = 0
    for name in sorted(n for n in byname_p if n.startswith("k_conv")):
        a, b = steady_mix(ps, byname_p[name]), steady_mix(ns, byname_n[name])
        diff = {k: (a[k], b[k]) for k in sorted(set(a) | set(b)) if a[k] != b[k]}
        fail = [k for k in must if k in diff]
        bad2 += len(fail)
        same += not diff
        print("%-44s %s | %s%s" % (name, " ".join("%s %d" % (k, b[k]) for k in must), "same mix" if not diff else
                                   "  ".join("%s %d -> %d" % (k, v[0], v[1]) for k, v in diff.items()), "  FAIL " + ",".join(fail) if fail else ""))
    print("k_conv* kernels with the same mix in every class: %d; violations: %d" % (same, bad2))
    return 1 if bad or bad2 else 0


if __name__ == "__main__":
    sys.exit(main())
