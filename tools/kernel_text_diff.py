"""Kernel by kernel, the text of two device compilations (`hipcc -S --cuda-device-only ... -o X.s`):
    python3 tools/kernel_text_diff.py PARENT.s BRANCH.s [--rename 'REGEX=>REPLACEMENT' ...] [--only REGEX] [--diff REGEX]
For every kernel (.amdhsa_kernel) of either file, by its demangled name without anonymous namespaces and argument list:
    identical             the same instructions, operands included
    register names only   the same opcodes in the same order, some operand differs
    opcode sequence differs
with the instruction count, VGPRs, SGPRs, scratch bytes and static LDS bytes of both sides (.amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr,
.amdhsa_private_segment_fixed_size, .amdhsa_group_segment_fixed_size), then the kernels new and gone, then whether the kernels both files
have come in the same order, then the kernels in which the branch needs more of a resource than the parent.
A --rename rule rewrites the PARENT's names before the match (a renamed kernel beside its twin).  --only: list only the names that match
(the summary counts all).  --diff: also the unified diff of the instructions of the kernels that match and differ.  Only the numbers of
the block labels (.LBB<n>_<m>) are normalised: they count the functions of the file.  The tool compares text; it looks for no particular
instruction."""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"\.LBB\d+_")
RES = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr", "scratch": ".amdhsa_private_segment_fixed_size",
       "lds": ".amdhsa_group_segment_fixed_size"}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt")
    if not tool or not names:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return out if len(out) == len(names) else list(names)


def short(name):
    """`void (anonymous namespace)::k<a, b>(float*, int)` -> `k<a, b>`"""
    name = name.replace("(anonymous namespace)::", "").replace("> >", ">>").replace("> >", ">>")
    depth, cut = 0, len(name)
    for i in range(len(name) - 1, -1, -1):  # the argument list: the last parenthesis group at depth 0
        c = name[i]
        if c == ")":
            depth += 1
        elif c == "(":
            depth -= 1
            if depth == 0:
                cut = i
                break
    name = name[:cut] if name.endswith(")") else name
    return name[5:] if name.startswith("void ") else name


def parse(path):
    """[(mangled, instructions, resources)] in the order of the function bodies"""
    lines = open(path, errors="replace").read().splitlines()
    bodies, order, res, funcs = {}, [], {}, set()
    cur = None
    for i, ln in enumerate(lines):
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):  # (the descriptor follows the body, before the function's end)
            r = res[s.split()[1]] = {}
            for m in lines[i + 1:]:
                t = m.split()
                if not t or t[0] == ".end_amdhsa_kernel":
                    break
                for key, d in RES.items():
                    if t[0] == d:
                        r[key] = int(t[1], 0)
            continue
        if cur is None:
            if s.startswith(".type") and s.endswith(",@function"):
                funcs.add(s.split()[1].rsplit(",", 1)[0])
            elif s.split(":", 1)[0] in funcs and s.split(":", 1)[0] not in bodies:  # (`name: ; @name`)
                cur = s.split(":", 1)[0]
                bodies[cur] = []
                order.append(cur)
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        code = s.split(";", 1)[0].strip()
        if not code or (code.startswith(".") and not code.endswith(":")):  # (directives; block labels stay)
            continue
        bodies[cur].append(LABEL.sub(".LBB_", code))
    return [(k, bodies[k], res[k]) for k in order if k in res]


def fmt(n, r):
    return f"{n:5d} instr {r.get('vgpr', -1):3d} v {r.get('sgpr', -1):3d} s {r.get('scratch', -1):4d} scratch {r.get('lds', -1):6d} lds"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=>REPLACEMENT on the parent's names")
    ap.add_argument("--only", default=None, help="list only the kernels whose name (either side) matches")
    ap.add_argument("--diff", default=None, help="print the unified diff of the kernels whose name matches")
    a = ap.parse_args()
    rules = [(re.compile(x.split("=>", 1)[0]), x.split("=>", 1)[1]) for x in a.rename]
    only = re.compile(a.only) if a.only else None

    def load(path, rename):
        ks = parse(path)
        names = [short(d) for d in demangle([k for k, _, _ in ks])]
        if len(set(names)) != len(names):  # (overloads: keep the whole symbol)
            names = [k for k, _, _ in ks]
        if rename:
            was = list(names)
            for rx, rep in rules:
                names = [rx.sub(rep, x) for x in names]
            return names, {x: (b, r, w) for x, w, (_, b, r) in zip(names, was, ks)}
        return names, {x: (b, r, x) for x, (_, b, r) in zip(names, ks)}

    pn, P = load(a.parent, True)
    bn, B = load(a.branch, False)
    count = {"identical": 0, "register names only": 0, "opcode sequence differs": 0}
    scratch, more = [], []
    for x in bn:
        if B[x][1].get("scratch", 0):
            scratch.append(x)
        if x not in P:
            continue
        (pb, pr, was), (bb, br, _) = P[x], B[x]
        verdict = "identical" if pb == bb else "register names only" if [i.split()[0] for i in pb] == [i.split()[0] for i in bb] else "opcode sequence differs"
        count[verdict] += 1
        up = [f"{k} {pr.get(k, 0)} -> {br.get(k, 0)}" for k in RES if br.get(k, 0) > pr.get(k, 0)]
        if up:
            more.append(f"{x}: " + ", ".join(up))
        if only is None or only.search(x) or only.search(was):
            twin = f"  (parent: {was})" if was != x else ""
            print(f"{verdict:24s} {x}{twin}\n{'':24s}   parent {fmt(len(pb), pr)} | branch {fmt(len(bb), br)}")
        if a.diff and verdict != "identical" and re.search(a.diff, x):
            print("\n".join(difflib.unified_diff(pb, bb, "parent", "branch", lineterm="", n=2)))
    new, gone = [x for x in bn if x not in P], [x for x in pn if x not in B]
    print(f"\nnew ({len(new)}):")
    for x in new:
        print(f"  {x}   {fmt(len(B[x][0]), B[x][1])}")
    print(f"gone ({len(gone)}):")
    for x in gone:
        print(f"  {P[x][2]}   {fmt(len(P[x][0]), P[x][1])}")
    po, bo = [x for x in pn if x in B], [x for x in bn if x in P]
    print(f"\nkernels: parent {len(pn)}, branch {len(bn)}, in both {len(po)}: " + ", ".join(f"{v} {k}" for k, v in count.items()))
    if po == bo:
        print("order of the kernels in both: the same")
    else:
        moved = [x for x, y in zip(po, bo) if x != y]
        print(f"order of the kernels in both: DIFFERS, first at parent `{moved[0]}`")
        rest = [x for x in po if only is None or not only.search(x)]
        print("  without the --only kernels: " + ("the same" if rest == [x for x in bo if x in set(rest)] else "DIFFERS"))
    print(f"kernels in which the branch needs more than the parent ({len(more)}):" + "".join("\n  " + m for m in more))
    if only:
        listed = [x for x in scratch if only.search(x)]
        print(f"kernels of the branch with scratch: {len(scratch)}; among the --only kernels: " + (", ".join(listed) if listed else "none"))
    else:
        print("kernels of the branch with scratch: " + (", ".join(scratch) if scratch else "none"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
