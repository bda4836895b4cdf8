"""How the matrix and the vector instructions of a kernel's largest loop are laid out in its device assembly (CPU only; opcodes are all it
reads).  The head backward kernels of csrc/mlp_fused.hip run one or two waves per SIMD, so what overlaps has to overlap inside one
instruction stream: a matrix instruction covers the vector instructions right behind it, a long run without one covers nothing.

usage: python tools/loop_schedule.py file.s kernel [--out file.json]
       kernel: the mangled symbol, or a part of it or of its demangled name as the `; -- Begin function` / label lines give it; the first
       kernel whose symbol contains it is taken (neck_bwdw_kernel<2,2,1> is spelled neck_bwdw_kernelILi2ELi2ELi1E).

Assembly: hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -S csrc/mlp_fused.hip

The loop: of all backward branches of the kernel (a branch whose target label stands above it), the one that spans the most instructions;
the rows describe the instructions from its target label to the branch itself.
  instructions            all of them
  matrix                  v_mfma_* / v_smfmac_*, by opcode
  vector                  every other v_* (of them: v_accvgpr_read / v_accvgpr_write / v_accvgpr_mov)
  lds / scalar / vmem     ds_* / s_* without s_nop and s_waitcnt / global_*, buffer_*, flat_*, scratch_*
  s_nop                   their number and the wait states they stand for (s_nop N = N + 1)
  s_waitcnt               their number
  matrix_back_to_back     matrix instructions that directly follow another one
  before_first / after_last   instructions in front of the first / behind the last matrix instruction of the loop
  matrix_free_runs        the runs of instructions BETWEEN two matrix instructions, longest first (the first eight)
  in_runs_longer_than_8   instructions inside such runs of more than eight
  vector_in_runs_longer_than_8   the vector instructions among them
"""
import collections
import json
import re
import sys

LABEL = re.compile(r"^([.\w$]+):")
INST = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b(.*)$")
BRANCH = re.compile(r"^s_c?branch")


def kernel_lines(path, kernel):
    """The body of the first function whose symbol contains `kernel`: from its label to its .Lfunc_end."""
    key = re.sub(r"[\s]", "", kernel)
    body, name = None, None
    with open(path) as f:
        for line in f:
            if body is None:
                m = LABEL.match(line)
                if m and not m.group(1).startswith(".") and key in m.group(1):
                    name, body = m.group(1), []
                continue
            if line.startswith(".Lfunc_end") or line.lstrip().startswith(".end_amdhsa_kernel"):
                break
            body.append(line.rstrip("\n"))
    if body is None:
        raise SystemExit(f"{path}: no function whose symbol contains '{key}'")
    return name, body


def parse(body):
    """-> ([(opcode, operand text)], {label: index of the instruction it stands in front of})"""
    insts, labels = [], {}
    for line in body:
        code = line.split(";", 1)[0]
        m = LABEL.match(code)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        m = INST.match(code)
        if m and not m.group(1).startswith("."):
            insts.append((m.group(1), m.group(2).strip()))
    return insts, labels


def largest_loop(insts, labels):
    best = None
    for i, (op, args) in enumerate(insts):
        if BRANCH.match(op):
            tgt = labels.get(args.split(",")[-1].strip())
            if tgt is not None and tgt <= i and (best is None or i - tgt > best[1] - best[0]):
                best = (tgt, i)
    if best is None:
        raise SystemExit("no backward branch in this kernel")
    return best


def kind(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "matrix"
    if op.startswith("v_"):
        return "vector"
    if op.startswith("ds_"):
        return "lds"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("s_"):
        return "scalar"
    if op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        return "vmem"
    return "other"


def schedule(insts):
    kinds = [kind(op) for op, _ in insts]
    n = collections.Counter(kinds)
    by_op = collections.Counter(op for (op, _), k in zip(insts, kinds) if k == "matrix")
    acc_moves = sum(1 for op, _ in insts if op.startswith("v_accvgpr"))
    nop_states = sum(int(a.split()[0], 0) + 1 for (op, a), k in zip(insts, kinds) if k == "s_nop" and a)
    pos = [i for i, k in enumerate(kinds) if k == "matrix"]
    res = {"instructions": len(insts), "matrix": n["matrix"], "matrix_by_opcode": dict(by_op.most_common()),
           "vector": n["vector"], "vector_accvgpr_moves": acc_moves, "lds": n["lds"], "scalar": n["scalar"], "vmem": n["vmem"],
           "s_nop": n["s_nop"], "s_nop_wait_states": nop_states, "s_waitcnt": n["s_waitcnt"], "other": n["other"]}
    if not pos:
        return res
    gaps = [(b - a - 1, a + 1) for a, b in zip(pos, pos[1:])]
    long_runs = [(g, s) for g, s in gaps if g > 8]
    res.update({"matrix_back_to_back": sum(1 for g, _ in gaps if g == 0), "before_first": pos[0], "after_last": len(insts) - 1 - pos[-1],
                "matrix_free_runs": sorted((g for g, _ in gaps), reverse=True)[:8],
                "in_runs_longer_than_8": sum(g for g, _ in long_runs),
                "vector_in_runs_longer_than_8": sum(kinds[s:s + g].count("vector") for g, s in long_runs)})
    return res


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) != 2:
        raise SystemExit(__doc__)
    name, body = kernel_lines(argv[0], argv[1])
    insts, labels = parse(body)
    lo, hi = largest_loop(insts, labels)
    res = {"kernel": name, "kernel_instructions": len(insts), "loop": {"first": lo, "last": hi}, **schedule(insts[lo:hi + 1])}
    text = json.dumps(res, indent=1)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
