#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (csrc: `make build/<unit>.s`), kernel by kernel.

    tools/kernel_diff.py OLD.s NEW.s [--rename OLD_TEXT=NEW_TEXT ...]

Kernels are matched by demangled name.  --rename rewrites OLD's names before matching (the first
rule whose OLD_TEXT occurs in a name is applied to it, once), for kernels that were renamed or
gained template arguments.  Per kernel, comments and debug/bookkeeping directives are dropped,
branch-label numbers and the kernel's own symbol are normalised, and the instruction list and the
whole .amdhsa_* block are compared line by line.  Exit status 1 on any difference or on a kernel
that only one side has."""
import argparse
import re
import shutil
import subprocess
import sys

# assembler lines that emit no code: sections, symbol bookkeeping, debug information
SKIP = re.compile(r"\.(section|text|globl|weak|protected|hidden|type|size|set|file|loc|cfi_\w+|ident|addrsig\w*)\b")
LABEL_NO = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not symbols:
        return list(symbols)
    # _Float16 (DF16_) given as the older half type (Dh), which every c++filt knows; neither is a
    # substitution candidate, so the rest of the name is unaffected
    text = "\n".join(symbols).replace("DF16_", "Dh") + "\n"
    out = subprocess.run([tool], input=text, capture_output=True, text=True, check=True).stdout
    return [n.replace("(anonymous namespace)::", "") for n in out.splitlines()]


def short(name):
    """a demangled kernel name without its return type and parameter list"""
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            name = name[:i]
            break
    return name[5:] if name.startswith("void ") else name


def kernels(path):
    """{demangled name: (instructions, .amdhsa directives)} of every kernel of an assembly file"""
    lines = [ln.split(";", 1)[0].strip() for ln in open(path)]
    symbols = [ln.split()[1] for ln in lines if ln.startswith(".amdhsa_kernel ")]
    found = {}
    for sym, name in zip(symbols, demangle(symbols)):
        begin = lines.index(sym + ":")
        end = next(i for i in range(begin, len(lines)) if lines[i].startswith(".Lfunc_end"))
        code, directives, in_text = [], [], True  # the kernel descriptor sits in .rodata, mid-function
        for ln in lines[begin + 1:end]:
            if ln.startswith(".section"):
                in_text = ".text" in ln
            elif ln.startswith(".amdhsa_") and ln != ".amdhsa_kernel " + sym:
                directives.append(ln)
            elif in_text and ln and not SKIP.match(ln):
                code.append(LABEL_NO.sub(r".L\1", ln).replace(sym, "<self>"))
        found[name] = (code, directives)
    return found


def first_difference(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"{what} {i}: '{x}' | '{y}'"
    return f"{what} count: {len(a)} | {len(b)}" if len(a) != len(b) else None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD_TEXT=NEW_TEXT")
    args = ap.parse_args(argv)
    rules = [r.split("=", 1) for r in args.rename]
    old = {}
    for name, k in kernels(args.old).items():
        for a, b in rules:
            if a in name:
                name = name.replace(a, b)
                break
        old[name] = k
    new = kernels(args.new)
    bad = 0
    for name in old:
        if name not in new:
            print(f"only in {args.old}: {short(name)}")
            bad += 1
            continue
        d = first_difference(old[name][0], new[name][0], "instruction") or \
            first_difference(old[name][1], new[name][1], "directive")
        print(f"differs: {short(name)} (first difference at {d})" if d else f"identical: {short(name)}")
        bad += d is not None
    for name in new:
        if name not in old:
            print(f"only in {args.new}: {short(name)}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
