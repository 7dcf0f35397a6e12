"""Compares two gfx950 assembly files of one translation unit, function by function: what a refactor that moves host code (and with it
the order in which templates are instantiated) has to leave unchanged.  Make the two files with the Makefile's flags, e.g.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S tandem_amd/csrc/dr_fusion.hip -o new.s

at the parent and at the tree (plain and with -DDR_PARITY_HOOKS), then  python tools/compare_kernel_asm.py parent.s new.s.
Each function's text runs from its .type line to the next function's first line; block, jump-table and function-end labels are
renumbered per file by the compiler, so their numbers are dropped, as are runs of blanks (comment columns follow the label's width)
and the compilation unit's id symbol (__hip_cuid_*, a hash of the source).  Prints the kernel counts, the names on one side only and
every function whose text differs; exit status 1 if there is any.  No GPU needed."""
import re
import sys

FUNC = re.compile(r"^\t\.type\t(\S+),@function")


def functions(path):
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    starts = [i for i, l in enumerate(lines) if FUNC.match(l)]
    end = next(i for i, l in enumerate(lines) if ".amdgpu_metadata" in l)
    out, order = {}, []
    for a, b in zip(starts, starts[1:] + [end]):
        name = FUNC.match(lines[a]).group(1)
        body = []
        for l in lines[a + 1:b]:
            if "-- Begin function" in l or re.match(r"^\t\.type\t\S+,@object", l):
                break
            l = re.sub(r"BB\d+_", "BB_", l)
            l = re.sub(r"\.Lfunc_(end|begin)\d+", r".Lfunc_\1", l)
            l = re.sub(r"\.LJTI\d+_", ".LJTI_", l)
            l = re.sub(r"\s+", " ", l).strip()
            # section switches and what closes the text section (.set amdgpu.max_num_*, the padding behind the last function) stand
            # between functions: they follow the order, not the function
            if l and not re.match(r"^\.(section|text|protected|globl|weak|hidden|p2align|p2alignl|fill)\b", l) and not l.startswith(".set amdgpu.max_num_"):
                body.append(l)
        assert name not in out, name
        out[name] = body
        order.append(name)
    kernels = sum(1 for l in lines if l.startswith("\t.amdhsa_kernel "))
    return out, order, kernels


def main():
    (fa, oa, ka), (fb, ob, kb) = functions(sys.argv[1]), functions(sys.argv[2])
    print("kernels: %d and %d; functions: %d and %d; same order: %s" % (ka, kb, len(fa), len(fb), oa == ob))
    one_side = sorted(set(fa) ^ set(fb))
    for n in one_side:
        print("only in %s: %s" % (sys.argv[1] if n in fa else sys.argv[2], n))
    differ = [n for n in oa if n in fb and fa[n] != fb[n]]
    for n in differ:
        k = next((i for i, (x, y) in enumerate(zip(fa[n], fb[n])) if x != y), min(len(fa[n]), len(fb[n])))
        print("differs: %s (line %d of %d / %d)" % (n, k, len(fa[n]), len(fb[n])))
    print("instructions and directives compared: %d; functions that differ: %d" % (sum(len(v) for v in fa.values()), len(differ)))
    sys.exit(1 if one_side or differ or ka != kb else 0)


if __name__ == "__main__":
    main()
