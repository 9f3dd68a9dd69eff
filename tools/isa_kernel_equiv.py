#!/usr/bin/env python3
"""Are two sets of device-assembly files the same kernels?  For moves of kernels between translation units (no GPU needed): a file-level hash cannot say,
because local labels (.LBB<function>_<block>, .Lfunc_end<n>) are numbered per translation unit and the order of functions follows the source.
    hipcc <the flags of mvlt_amd/build.py> --offload-device-only -S mvlt_amd/csrc/X.hip -o X.s          (once per file, old tree and new tree)
    python tools/isa_kernel_equiv.py --old old/gemm.s --new new/gemm.s new/gemm_nt_dma.s ...
Each file is cut into functions by symbol; comments, blank lines, the cuid object and the ident line are dropped and the local labels of a function are renumbered in
order of first appearance.  Per kernel name, the instruction text and the .amdhsa_* descriptor block (registers, LDS, scratch, occupancy hints) must be equal.  Prints the
names found on one side only, the names that differ with the first differing line, and a one-line total; exit status 1 on any difference."""
import argparse
import re
import sys

_LABEL = re.compile(r"\.L[A-Za-z_]+\d[\d_]*")


def _clean(line):
    return line.split(";", 1)[0].rstrip()


def kernels(text):
    """{kernel name: (instruction lines, descriptor lines)} of one assembly file"""
    lines = text.split("\n")
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", l)] if m}
    spans, name = [], None                            # (name, first line behind its label, its .Lfunc_end line)
    for i, l in enumerate(lines):
        if name is None and l[:1] not in ("", "\t", " ", ".") and l.split(":", 1)[0] in names:
            name, start = l.split(":", 1)[0], i + 1
        elif name is not None and l.startswith(".Lfunc_end"):
            spans.append((name, start, i))
            name = None
    out = {}
    for name, start, end in spans:
        body, desc, in_desc = [], None, False
        for l in lines[start:end]:
            l = _clean(l)
            if not l.strip() or "__hip_cuid_" in l or l.lstrip().startswith(".ident"):
                continue
            if re.match(r"\s*\.amdhsa_kernel\s", l):
                in_desc, desc = True, []
            elif re.match(r"\s*\.end_amdhsa_kernel", l):
                in_desc = False
            elif in_desc:
                desc.append(" ".join(l.split()))
            else:
                body.append(l)
        if desc is None:
            continue                                  # a device function that is no kernel
        number = {}
        out[name] = ([_LABEL.sub(lambda m: number.setdefault(m.group(0), f".L{len(number)}"), " ".join(l.split())) for l in body], desc)
    return out


def _first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"line {i + 1}: `{x}` | `{y}`"
    return f"line {min(len(a), len(b)) + 1}: {len(a)} lines | {len(b)} lines"


def compare(old_texts, new_texts):
    """(report lines, the last of them the total; number of differences)"""
    sides, report = [], []
    for tag, texts in (("old", old_texts), ("new", new_texts)):
        side = {}
        for t in texts:
            for name, k in kernels(t).items():
                if name in side:
                    report.append(f"twice in {tag}: {name}")
                side[name] = k
        sides.append(side)
    old, new = sides
    twice = len(report)
    only = [f"only in old: {n}" for n in sorted(set(old) - set(new))] + [f"only in new: {n}" for n in sorted(set(new) - set(old))]
    diff = []
    for n in sorted(set(old) & set(new)):
        for what, a, b in (("body", old[n][0], new[n][0]), ("descriptor", old[n][1], new[n][1])):
            if a != b:
                diff.append(f"differs: {n} ({what}) {_first_difference(a, b)}")
    differing = len({d.split()[1] for d in diff})
    report += only + diff
    report.append(f"{len(old)} kernels old, {len(new)} kernels new: {len(only)} on one side only, {differing} different" + (f", {twice} defined twice" if twice else ""))
    return report, len(only) + differing + twice


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    report, bad = compare([open(f).read() for f in a.old], [open(f).read() for f in a.new])
    print("\n".join(report))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
