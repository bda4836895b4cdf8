"""Compare two device assembly files of one source, kernel by kernel: did a refactor leave the generated code as it was?

usage: python tools/isa_compare.py OLD.s NEW.s [--json out.json] [--quiet]

OLD.s / NEW.s come from `hipcc <CXXFLAGS of emernerf_amd/_build.py> --cuda-device-only -S` on the two versions of a .hip file (compile
inside a copy of the tree so that the relative includes resolve).  Needs no GPU.

Per kernel symbol the instruction lines (comments, directives and labels dropped) are classed as
  equal       the same lines;
  equivalent  the same number of lines, and every line that differs is the same mnemonic and destination with its two source operands
              swapped -- accepted only for the commutative ALU mnemonics listed in COMMUTATIVE;
  changed     anything else.
VGPRs, AGPRs, scratch, LDS, spills and occupancy of both files are printed from the kernel metadata (occupancy from the resource comment
the compiler writes behind each kernel).  Exit status 1 if a kernel is missing on either side or the resource gate is violated: no kernel
may use more VGPRs, AGPRs, scratch or LDS, spill more, or lose occupancy.  A decrease passes and is reported."""
import json
import re
import sys

# two-source ALU operations whose result does not depend on the order of the sources (plain, _e32 and _e64 encodings).  Multiply-adds are
# left out on purpose: only their first two sources commute, and a swap there has not been seen.
COMMUTATIVE = {
    "v_xor_b32", "v_and_b32", "v_or_b32", "v_add_u32", "v_add_f32", "v_mul_f32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_u32_u24", "v_max_f32",
    "v_min_f32", "v_max_u32", "v_min_u32", "v_add_f64", "v_mul_f64", "s_xor_b32", "s_and_b32", "s_or_b32", "s_add_i32", "s_mul_i32",
    "s_xor_b64", "s_and_b64", "s_or_b64",
}
GATED = ("vgpr", "agpr", "scratch", "lds", "vgpr_spill", "sgpr_spill")   # may not grow; "occupancy" may not shrink
META = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".private_segment_fixed_size": "scratch", ".group_segment_fixed_size": "lds",
        ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill"}


def parse(path):
    """{kernel symbol: {"code": [instruction lines], "res": {resource: value}}}"""
    text = open(path).read().split("\n")
    kernels, res = {}, {}
    # metadata: one YAML list item per kernel, keys in alphabetical order, .name among them
    item = None
    for line in text:
        s = line.strip()
        if line.startswith("  - ."):
            item = {}
            s = s[2:]
        elif not re.match(r"^    \.", line):   # (only the kernel's own keys: the entries of .args sit deeper)
            continue
        if item is not None and ":" in s:
            key, _, val = s.partition(":")
            key, val = key.strip(), val.strip()
            if key in META and val.isdigit():
                item[META[key]] = int(val)
            elif key == ".name":
                res[val] = item
    cur = None
    last = None
    for line in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and cur is None and m.group(1) in res:
            cur = m.group(1)
            kernels[cur] = {"code": [], "res": res[cur]}
            last = cur
            continue
        s = line.split(";", 1)[0].strip()
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                cur = None
            elif s and not s.startswith(".") and not s.endswith(":"):
                kernels[cur]["code"].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
        elif last is not None:
            m = re.match(r"^; Occupancy: (\d+)", line)
            if m and "occupancy" not in kernels[last]["res"]:
                kernels[last]["res"]["occupancy"] = int(m.group(1))
    return kernels


def split_ops(line):
    mnem, _, rest = line.partition(" ")
    return mnem, [o.strip() for o in rest.split(",")]


def swapped(a, b):
    ma, oa = split_ops(a)
    mb, ob = split_ops(b)
    base = re.sub(r"_e(32|64)$", "", ma)
    if ma != mb or base not in COMMUTATIVE or len(oa) != 3 or len(ob) != 3:
        return False
    return oa[0] == ob[0] and oa[1] == ob[2] and oa[2] == ob[1]


def classify(old, new):
    if old == new:
        return "equal", 0
    if len(old) != len(new):
        return "changed", None
    diff = [(a, b) for a, b in zip(old, new) if a != b]
    return ("equivalent" if all(swapped(a, b) for a, b in diff) else "changed"), len(diff)


def demangle_short(sym):
    """hashgrid_fwd_kernel<2,1,float,4,0> from the mangled name (integer, bool, float and half template arguments); else the symbol"""
    m = re.match(r"_ZN4emer\d+([a-z_0-9]+?kernel)I(.*?)EEv", sym)
    if not m:
        return sym[:60]
    args, rest = [], m.group(2) + "E"
    while rest and rest != "E":
        t = re.match(r"Li(\d+)E|Lb([01])E|(f)|(6__half|DF16_|Dh)", rest)
        if not t:
            return sym[:60]
        args.append(t.group(1) or t.group(2) or ("float" if t.group(3) else "half"))
        rest = rest[t.end():]
    return f"{m.group(1)}<{','.join(args)}>"


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out_json in argv:
        argv.remove(out_json)
    if len(argv) != 2:
        sys.exit(__doc__)
    old, new = parse(argv[0]), parse(argv[1])
    missing = sorted(set(old) ^ set(new))
    rows, bad, counts = [], [], {"equal": 0, "equivalent": 0, "changed": 0}
    for sym in sorted(set(old) & set(new)):
        cls, ndiff = classify(old[sym]["code"], new[sym]["code"])
        counts[cls] += 1
        ro, rn = old[sym]["res"], new[sym]["res"]
        viol = ["unparsed:" + k for k in GATED + ("occupancy",) if k not in ro or k not in rn]   # a number that is not there holds no gate
        viol += [k for k in GATED if k in ro and k in rn and rn[k] > ro[k]]
        if "occupancy" in ro and "occupancy" in rn and rn["occupancy"] < ro["occupancy"]:
            viol.append("occupancy")
        row = {"kernel": demangle_short(sym), "symbol": sym, "class": cls, "lines_old": len(old[sym]["code"]), "lines_new": len(new[sym]["code"]),
               "differing_lines": ndiff, "old": ro, "new": rn, "gate": "ok" if not viol else "FAIL " + ",".join(viol)}
        rows.append(row)
        if viol:
            bad.append(row)
    quiet = "--quiet" in sys.argv
    fmt = lambda r: f"{r.get('vgpr', '?')}/{r.get('agpr', '?')}/{r.get('scratch', '?')}/{r.get('lds', '?')}/occ{r.get('occupancy', '?')}"
    print(f"{'kernel':58s} {'class':10s} {'lines old>new':>14s} {'diff':>5s}  vgpr/agpr/scratch/lds/occ old -> new")
    for r in rows:
        if quiet and r["class"] == "equal" and r["gate"] == "ok" and r["old"] == r["new"]:
            continue
        print(f"{r['kernel']:58s} {r['class']:10s} {r['lines_old']:>6d}>{r['lines_new']:<7d} {str(r['differing_lines'] if r['differing_lines'] is not None else '-'):>5s}  "
              f"{fmt(r['old'])} -> {fmt(r['new'])}  {r['gate']}")
    print(f"{len(rows)} kernels on both sides: {counts['equal']} equal, {counts['equivalent']} equivalent, {counts['changed']} changed; "
          f"{len(missing)} missing on one side; {len(bad)} resource gate violations")
    for sym in missing:
        print("missing in", "NEW" if sym in old else "OLD", ":", sym)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"counts": counts, "missing": missing, "kernels": rows}, f, indent=1)
            f.write("\n")
    sys.exit(1 if (missing or bad) else 0)


if __name__ == "__main__":
    main()
