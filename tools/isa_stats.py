#!/usr/bin/env python3
"""Per-kernel instruction mix from `hipcc --cuda-device-only -S` output: VALU / LDS / global / scratch counts,
overall and inside the largest loop bodies (backward-branch spans).

    isa_stats.py FILE.s [NAME_PART ...]
    isa_stats.py --compare PARENT.s THIS.s

--compare: for every function of the two files, whether the instruction stream is identical once comments, directives
and labels are stripped (labels that instructions refer to are renumbered in order of definition); where it is not,
the instruction counts, the opcode-count differences of the whole function and of its largest loop (the largest
backward-branch span whose target the compiler's label annotation places in a loop: a branch back to an early-exit
block spans most of a function without being one), and the kernel descriptor fields of both sides."""
import collections
import re
import sys

FUNC = re.compile(r"^(_ZN3gyp\w+):[^\n]*\n(.*?)^\.Lfunc_end", flags=re.S | re.M)
LABEL = re.compile(r"(\.LBB\d+_\d+):")
BRANCH = re.compile(r"s_cbranch_\w+ (\.LBB\d+_\d+)|s_branch (\.LBB\d+_\d+)")
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")


def functions(txt):
    """name -> the function's lines without blank lines and whole-line comments (labels kept: the loops are found by them)"""
    return {m.group(1): [l.strip() for l in m.group(2).split("\n") if l.strip() and not l.strip().startswith(";")]
            for m in FUNC.finditer(txt)}


def loops(lines):
    """(span, first, last) of every backward branch, as indices into lines"""
    label_at = {}
    for i, l in enumerate(lines):
        mm = LABEL.match(l)
        if mm:
            label_at[mm.group(1)] = i
    out = []
    for i, l in enumerate(lines):
        mm = BRANCH.match(l)
        if mm:
            tgt = mm.group(1) or mm.group(2)
            if tgt in label_at and label_at[tgt] < i:
                out.append((i - label_at[tgt], label_at[tgt], i))
    return out


def count(ls, pat):
    return sum(1 for l in ls if re.match(pat, l))


def mix(ls):
    return {"valu": count(ls, r"v_"), "ds": count(ls, r"ds_"), "gload": count(ls, r"global_load"), "gstore": count(ls, r"global_store"),
            "sload": count(ls, r"scratch_load"), "sstore": count(ls, r"scratch_store"), "wait": count(ls, r"s_waitcnt"),
            "barrier": count(ls, r"s_barrier"), "salu": count(ls, r"s_(?!waitcnt|barrier|nop)")}


def stats(path, want):
    for name, lines in functions(open(path).read()).items():
        if not any(w in name for w in want):
            continue
        print(name[:70], len(lines), mix(lines))
        for span, a, b in sorted(loops(lines), reverse=True)[:4]:
            print("   loop", lines[a][:14], "span", span, mix(lines[a:b]))


def normalise(lines):
    """instructions only: no comments, directives or labels; label operands renumbered in order of definition"""
    names = {}
    for l in lines:
        mm = LABEL.match(l)
        if mm:
            names.setdefault(mm.group(1), "L%d" % len(names))
    out = []
    for l in lines:
        l = l.split(";")[0].strip()
        if not l or l.startswith(".") or re.match(r"[\w.$]+:$", l):
            continue
        out.append(re.sub(r"\.LBB\d+_\d+", lambda m: names.get(m.group(0), m.group(0)), l))
    return out


def opcodes(lines):
    return collections.Counter(l.split()[0] for l in normalise(lines))


def opcode_diff(a, b):
    d = {k: (a[k], b[k]) for k in sorted(set(a) | set(b)) if a[k] != b[k]}
    return ", ".join("%s %d -> %d" % (k, v[0], v[1]) for k, v in d.items()) or "none"


def main_loop(lines):
    """The largest backward-branch span whose target the compiler's own annotation places in a loop ("Loop Header" / "in Loop"
    behind the label).  A backward branch to a block laid out early -- an early exit, a rare path -- spans most of a function
    without being a loop; where nothing is annotated, the largest span."""
    ls = loops(lines)
    if not ls:
        return []
    _, a, b = max([l for l in ls if "Loop" in lines[l[1]]] or ls)
    return lines[a:b]


def descriptors(txt):
    """kernel name -> {field: value} from the amdhsa.kernels metadata"""
    out = {}
    meta = txt[txt.find("amdhsa.kernels:"):]
    for block in re.split(r"^  - ", meta, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, flags=re.M)
        if name:
            out[name.group(1)] = {f: int(v) for f, v in re.findall(r"^\s+(\.\w+):\s+(\d+)\s*$", block, flags=re.M) if f in FIELDS}
    return out


def compare(path_a, path_b):
    ta, tb = open(path_a).read(), open(path_b).read()
    fa, fb, da, db = functions(ta), functions(tb), descriptors(ta), descriptors(tb)
    same = 0
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            print(name, "ONLY IN", path_a if name in fa else path_b)
            continue
        na, nb = normalise(fa[name]), normalise(fb[name])
        if na == nb:
            same += 1
            print(name, "identical")
            continue
        print(name, "DIFFERS")
        print("   instructions", len(na), "->", len(nb))
        print("   opcodes, whole:", opcode_diff(opcodes(fa[name]), opcodes(fb[name])))
        la, lb = main_loop(fa[name]), main_loop(fb[name])
        print("   largest loop: instructions", len(normalise(la)), "->", len(normalise(lb)))
        print("   opcodes, largest loop:", opcode_diff(opcodes(la), opcodes(lb)))
        for f in FIELDS:
            if name in da or name in db:
                va, vb = da.get(name, {}).get(f), db.get(name, {}).get(f)
                print("   %s %s -> %s%s" % (f, va, vb, "" if va == vb else "   CHANGED"))
    print("%d of %d functions identical" % (same, len(set(fa) | set(fb))))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        stats(sys.argv[1], sys.argv[2:] or ["corr_cells_kernelILi8ELb0E", "track_block_kernelILi8ELb0E", "grid_cells_wave_kernelILi2"])
