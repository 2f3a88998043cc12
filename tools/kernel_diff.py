#!/usr/bin/env python3
"""Compare every gfx950 kernel of two builds of the engine library, instruction by instruction.

usage: kernel_diff.py LIB_A LIB_B

Unbundles both code objects (as disasm.py), disassembles them, and reports the kernels present in
only one build and those whose instruction streams (mnemonics, operands and encodings) differ.
Exit status 0 when every kernel is in both builds and identical: the check a host-only refactoring
has to pass in both operand libraries.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disasm  # noqa: E402


def kernels(lib):
    with tempfile.TemporaryDirectory() as d:
        co = disasm.code_object(lib, d)
        txt = subprocess.check_output([f"{disasm.LLVM}/llvm-objdump", "-d", "--demangle", co]).decode()
    out = {}
    for f in re.split(r"\n(?=[0-9a-f]{16} <)", txt):
        if "<" not in f[:400]:
            continue
        head, _, body = f.partition("\n")
        name = head.split("<", 1)[1].rsplit(">", 1)[0]
        ins = []
        for line in body.splitlines():
            m = re.match(r"\s*([a-z_0-9]+)\b(.*?)//\s*([0-9A-F]+):\s*(.*)", line)
            if m:
                ins.append(f"{m.group(1)} {m.group(2).strip()} {m.group(4).strip()}")
        out[name] = hashlib.sha256("\n".join(ins).encode()).hexdigest()
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}")
    for title, names in (("only in the first", only_a), ("only in the second", only_b), ("different", differ)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("  " + n)
    sys.exit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
