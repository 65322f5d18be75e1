#!/usr/bin/env python3
"""Compare two builds' device assembly kernel by kernel: is a kernel the same code after its source moved?

    hipcc <the Makefile's CXXFLAGS> --offload-arch=gfx950 --cuda-device-only -S x.hip -o x.s     (+ VITFLAGS for viterbi.hip)
    tools/kernel_asm_diff.py [--json OUT] BEFORE.s AFTER.s [AFTER2.s ...]

A kernel's body is every line from its label to its .Lfunc_end, comments stripped; the function index of local labels
(.LBB<n>_<k> -> .LBB_<k>) and the number of temporary labels go: they change when a function changes file and mean
nothing.  Its entry in the metadata note is compared in the fields of META.  One line per kernel; exit status 1 when a
kernel on both sides differs or a kernel of BEFORE is in no AFTER.  The comparison is of text: no instruction is known.
"""
import argparse
import json
import re
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "max_flat_workgroup_size")
_LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+_(\d+)")      # .LBB12_7, .LJTI12_0
_TEMP = re.compile(r"\.L(tmp|func_begin|func_end)\d+")


def parse(text):
    """{kernel symbol: {"body": [normalised lines], "instructions": count, "meta": {field: value}}}"""
    lines = text.splitlines()
    entries = []                                          # the metadata note: one "  - " block per kernel
    for ln in lines[lines.index("amdhsa.kernels:") + 1:] if "amdhsa.kernels:" in lines else []:
        if not ln.startswith("  "):
            break
        if ln.startswith("  - "):
            entries.append({})
        m = re.match(r"^  [ -] \.(\w+):\s*(\S+)$", ln)
        if m:
            entries[-1][m.group(1)] = m.group(2)
    kernels = {}
    for e in entries:
        body, label = [], next(i for i, ln in enumerate(lines) if ln.startswith(e["name"] + ":"))
        for ln in lines[label + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = " ".join(_TEMP.sub(r".L\1", _LOCAL.sub(r".L\1_\2", ln.split(";", 1)[0])).split())
            if ln:
                body.append(ln)
        kernels[e["name"]] = {"body": body, "instructions": sum(not ln.startswith(".") for ln in body),
                              "meta": {k: e.get(k) for k in META}}
    return kernels


def compare(before, after):
    """one row per kernel of either side; the *equal fields are None where a side lacks the kernel"""
    rows = []
    for name in list(before) + [n for n in after if n not in before]:
        a, b = before.get(name), after.get(name)
        r = {"kernel": name, "instructions": [a and a["instructions"], b and b["instructions"]], "meta": [a and a["meta"], b and b["meta"]],
             "body_equal": a["body"] == b["body"] if a and b else None, "meta_equal": a["meta"] == b["meta"] if a and b else None}
        r["equal"] = r["body_equal"] and r["meta_equal"] if a and b else None
        rows.append(r)
    return rows


def failed(rows):
    return any(r["equal"] is False or r["instructions"][1] is None for r in rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after", nargs="+")
    ap.add_argument("--json", help="also write the rows to this file")
    args = ap.parse_args(argv)
    before, after = parse(open(args.before).read()), {}
    for path in args.after:
        after.update(parse(open(path).read()))
    rows = compare(before, after)
    for r in rows:
        verdict = {True: "equal", False: "DIFFERENT", None: "only in AFTER" if r["instructions"][0] is None else "MISSING"}[r["equal"]]
        if r["equal"] is False:
            verdict += " (" + ", ".join(w for w in ("body", "meta") if not r[w + "_equal"]) + ")"
        print(f"{r['kernel']}  {r['instructions'][0]}  {r['instructions'][1]}  {verdict}")
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)
    return 1 if failed(rows) else 0


if __name__ == "__main__":
    sys.exit(main())
