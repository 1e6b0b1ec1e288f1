"""Are the kernels of two source trees the same instructions?

    python tools/kernel_asm_diff.py <tree A> <tree B>

Compiles make_prg_amd/csrc/mprg_api.hip of each tree to gfx950 assembly with the product's flags (__graft_entry__._hip_command of
this tree, with -S --cuda-device-only and without the link flags), both compiles side by side, splits the assembly per kernel,
drops the comments and the directives, renumbers the local labels in order of appearance, and compares kernel by kernel.  Prints
the kernels that differ, the kernels only one side has, and the instruction totals; exits 1 on any difference.  No GPU is needed.

The usual use is a refactor that must leave every kernel what it was: `git worktree add <dir> <parent commit>`, then
`python tools/kernel_asm_diff.py <dir> .`."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIP_SRC, _hip_command  # noqa: E402

LINK_FLAGS = ("-shared", "-fPIC", "-lz", "-pthread")
LABEL = re.compile(r"\.L[A-Za-z0-9_$]+")


def asm_command(tree: str, out: str) -> list:
    """The product's hipcc line, for `tree`'s mprg_api.hip, stopping at the device assembly."""
    cmd = _hip_command(os.path.join(os.path.dirname(out), "unused.so"), force=True)
    src = os.path.join(os.path.abspath(tree), os.path.relpath(HIP_SRC, ROOT))
    cmd = [src if a == HIP_SRC else a for a in cmd[:cmd.index("-o")] if a not in LINK_FLAGS]
    return cmd + ["-S", "--cuda-device-only", "-o", out]


def kernels(asm_path: str) -> dict:
    """{kernel symbol: its instructions and labels, one per line, normalised}."""
    with open(asm_path) as f:
        lines = f.read().split("\n")
    is_kernel = {ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")}
    out, name, body, labels = {}, None, [], {}
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln:
            continue
        if name is None:
            if ln.endswith(":") and ln[:-1] in is_kernel:
                name, body, labels = ln[:-1], [], {}
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = body
            name = None
        elif not ln.startswith(".") or ln.endswith(":"):          # an instruction or a label, not a directive
            body.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), " ".join(ln.split())))
    return out


def n_instructions(body: list) -> int:
    return sum(not ln.endswith(":") for ln in body)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", help="a source tree")
    ap.add_argument("b", help="the other source tree")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, side + ".s") for side in "ab"]
        procs = [subprocess.Popen(asm_command(tree, out)) for tree, out in zip((args.a, args.b), paths)]
        if any([p.wait() for p in procs]):
            print("kernel_asm_diff: a compile failed")
            return 2
        ka, kb = (kernels(p) for p in paths)
    differ = sorted(k for k in ka.keys() & kb.keys() if ka[k] != kb[k])
    for k in differ:
        first = next((i for i, (x, y) in enumerate(zip(ka[k], kb[k])) if x != y), min(len(ka[k]), len(kb[k])))
        print("differs: %s (%d against %d instructions, first at line %d: %r against %r)" % (
            k, n_instructions(ka[k]), n_instructions(kb[k]), first, ka[k][first:first + 1], kb[k][first:first + 1]))
    for tag, only in (("only in A", ka.keys() - kb.keys()), ("only in B", kb.keys() - ka.keys())):
        for k in sorted(only):
            print("%s: %s" % (tag, k))
    ta, tb = (sum(n_instructions(b) for b in k.values()) for k in (ka, kb))
    print("kernels: %d against %d; differing: %d; on one side only: %d; instructions: %d against %d" % (
        len(ka), len(kb), len(differ), len(ka.keys() ^ kb.keys()), ta, tb))
    return 1 if differ or ka.keys() != kb.keys() or ta != tb else 0


if __name__ == "__main__":
    sys.exit(main())
