#!/usr/bin/env python3
"""Are the device functions of two builds the same code?  Compares `make asm` output per function symbol:

    tools/diag/compare_kernel_asm.py before/*.s -- after/*.s

Each side is any number of .s files (hipcc --cuda-device-only -S).  A function's text runs from its "-- Begin function" line to
the next one: instructions, the .amdhsa_* kernel descriptor and the resource figures the compiler prints after it.  What only
numbers things within one file is normalised away (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>, ..., and runs of blanks), the lines that
switch sections or carry debug and ident information are dropped, and so is everything after the file's last function (the
padding of the code, the metadata note, which repeats the descriptors).
Prints "N symbols, M identical" and the names that differ or exist on one side only; exit status 0 only if all match."""
import difflib
import re
import sys

BEGIN = re.compile(r";\s*-- Begin function (\S+)")
FILE_NUMBER = re.compile(r"(\.L(?:JTI|func_begin|func_end|tmp)|\bBB|\.LBB)\d+")  # (BB<n>_<m> also in the loop comments)
DROPPED = (".section", ".text", ".file", ".loc", ".ident", ".cfi_")
PAST_FUNCTIONS = (".p2alignl", ".section\t.AMDGPU.gpr_maximums", ".amdgpu_metadata")  # (.p2alignl: the padding after a file's last function)


def functions(paths):
    """{symbol: normalised text} of every function in the files; a symbol defined twice with different text maps to None"""
    out = {}
    for path in paths:
        symbol, lines = None, []

        def close():
            if symbol is not None:
                text = "\n".join(lines)
                out[symbol] = text if out.get(symbol, text) == text else None

        with open(path) as f:
            for raw in f:
                line = raw.strip()
                if line.startswith(PAST_FUNCTIONS):
                    break
                m = BEGIN.search(line)
                if m:
                    close()
                    symbol, lines = m.group(1), []
                if symbol is None or not line or line.startswith(DROPPED):
                    continue
                lines.append(FILE_NUMBER.sub(r"\1", " ".join(line.split())))  # (a longer label shifts the comment column)
        close()
    return out


def main(argv):
    verbose = "-v" in argv
    argv = [a for a in argv if a != "-v"]
    if "--" not in argv:
        sys.exit(__doc__)
    cut = argv.index("--")
    a, b = functions(argv[:cut]), functions(argv[cut + 1:])
    names = sorted(set(a) | set(b))
    same = [n for n in names if n in a and n in b and a[n] is not None and a[n] == b[n]]
    print(f"{len(names)} symbols, {len(same)} identical")
    for n in names:
        if n in same:
            continue
        if n not in a or n not in b:
            print(f"  only {'after' if n not in a else 'before'}: {n}")
        elif a[n] is None or b[n] is None:
            print(f"  defined twice, differently, on one side: {n}")
        else:
            print(f"  differs: {n}")
            if verbose:
                for d in list(difflib.unified_diff(a[n].split("\n"), b[n].split("\n"), "before", "after", lineterm="", n=1))[:40]:
                    print("    " + d)
    return 0 if len(same) == len(names) and names else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
