"""Compare the device assembly of the persistent-row covariance kernels between two trees, kernel by kernel.

Usage:
    for f in cov_rows_*.hip kernel_rows_prod_*.hip predict_rows_*.hip; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S $f -o DIR/${f%.hip}.s
    done                                            # once in each tree
    python tools/rows_pipeline_isa.py PARENT_DIR HEAD_DIR > profiles/rows_pipeline_isa.txt

Per kernel: scratch and LDS size, registers, whole-kernel instruction counts by class (generic mnemonic prefixes only)
and the length of every loop that contains MFMAs.  A kernel PASSES when scratch is 0 (a miss says whether it is at
least not above the parent's), LDS is unchanged, registers and
loop lengths are not above the parent's and the class counts are equal.  Exit status 1 if any kernel misses.
"""
import glob
import os
import re
import sys

CLASSES = (
    ("mfma", re.compile(r"^v_mfma")),
    ("f64_valu", re.compile(r"^v_(?!mfma)\w*_f64")),
    ("gload", re.compile(r"^global_load")),
    ("gstore", re.compile(r"^global_store")),
    ("lds_read", re.compile(r"^ds_(read|load)")),
)
META = (".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_count", ".agpr_count")


def parse(path):
    """{kernel name: {"counts": {...}, "loops": [...], meta...}} of one assembly file."""
    lines = open(path).read().splitlines()
    kernels = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w*k_\w+):", lines[i])
        if not m:
            i += 1
            continue
        name, body = m.group(1), []
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            body.append(lines[i])
            i += 1
        insn = []          # (mnemonic, operands) or ("label", name, is_loop_header)
        for ln in body:
            lab = re.match(r"^(\.LBB\w+):(.*)", ln)
            if lab:
                insn.append(("label", lab.group(1), "Inner Loop Header" in lab.group(2)))
                continue
            code = ln.split(";")[0].strip()
            if code and not code.startswith("."):
                parts = code.split(None, 1)
                insn.append((parts[0], parts[1] if len(parts) > 1 else "", False))
        ops = [t for t in insn if t[0] != "label"]
        counts = {c: sum(1 for t in ops if rx.match(t[0])) for c, rx in CLASSES}
        counts["all"] = len(ops)
        loops = []
        for k, t in enumerate(insn):
            if t[0] == "label" and t[2]:
                back = [j for j in range(k, len(insn)) if insn[j][0].startswith(("s_cbranch", "s_branch")) and insn[j][1] == t[1]]
                if back:
                    inner = [u for u in insn[k:back[-1] + 1] if u[0] != "label"]
                    if any(u[0].startswith("v_mfma") for u in inner):
                        loops.append(len(inner))
        kernels[name] = {"counts": counts, "loops": loops}
    entry = {}
    for ln in lines + ["  - end"]:       # the metadata note at the end of the file: one list item per kernel
        if ln.startswith("  - "):
            if entry.get(".name") in kernels:
                kernels[entry[".name"]].update({k: int(entry[k]) for k in META})
            entry = {}
        m = re.match(r"^  (?:- |  )(\.\w+):\s+(\S+)", ln)
        if m:
            entry[m.group(1)] = m.group(2)
    return kernels


def demangled(name):
    m = re.search(r"\d+(k_\w+?)I(.*?)EEv6DevCov", name)
    if not m:
        return name
    args = [("-" + a[2:-1] if a[1] == "n" else a[2:-1]) if a.startswith("Li") else ("true" if a == "Lb1E" else "false")
            for a in re.findall(r"L[ib]n?\d+E", m.group(2))]
    return "%s<%s>" % (m.group(1), ",".join(args))


def load(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*.s"))):
        for k, v in parse(f).items():
            out[k] = dict(v, unit=os.path.basename(f)[:-2])
    return out


def main():
    parent, head = load(sys.argv[1]), load(sys.argv[2])
    missed = 0
    print("persistent-row kernels, gfx950 device assembly: parent -> head   (hipcc -O3 -std=c++17 --cuda-device-only -S)")
    print("columns: scratch | LDS | vgpr+agpr | " + " ".join(c for c, _ in CLASSES) + " | all | MFMA loop lengths")
    for name in sorted(parent, key=lambda k: (parent[k]["unit"], demangled(k))):
        p, h = parent[name], head.get(name)
        if h is None:
            print("%-58s MISSING in head" % demangled(name))
            missed += 1
            continue
        regs = lambda k: k[".vgpr_count"] + k[".agpr_count"]
        why = []
        if h[".private_segment_fixed_size"] != 0:
            why.append("scratch" + ("<=parent" if h[".private_segment_fixed_size"] <= p[".private_segment_fixed_size"] else ">parent"))
        if h[".group_segment_fixed_size"] != p[".group_segment_fixed_size"]: why.append("LDS")
        if regs(h) > regs(p): why.append("registers")
        why += [c for c, _ in CLASSES if h["counts"][c] != p["counts"][c]]
        if len(h["loops"]) != len(p["loops"]) or any(a > b for a, b in zip(h["loops"], p["loops"])): why.append("loops")
        missed += bool(why)
        row = lambda k: "%d | %d | %d | %s | %d | %s" % (
            k[".private_segment_fixed_size"], k[".group_segment_fixed_size"], regs(k),
            " ".join(str(k["counts"][c]) for c, _ in CLASSES), k["counts"]["all"], ",".join(map(str, k["loops"])))
        print("%-58s %s" % (demangled(name), "PASS" if not why else "MISS: " + " ".join(why)))
        print("    parent  " + row(p))
        print("    head    " + row(h))
    extra = sorted(set(head) - set(parent))
    for name in extra:
        print("%-58s only in head" % demangled(name))
    print("%d kernels compared, %d missed a condition" % (len(parent), missed + len(extra)))
    return 1 if missed or extra else 0


if __name__ == "__main__":
    sys.exit(main())
