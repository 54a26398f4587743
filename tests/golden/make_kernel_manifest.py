#!/usr/bin/env python3
"""Write tests/golden/kernel_manifest.json: the sorted names of every kernel in the built libfhespear_hip.so.

    python tests/golden/make_kernel_manifest.py

The kernels are the kernel descriptors (symbols ending in .kd) of the gfx950 code object inside the library
(tools/isa_dump.py code_object(), llvm-objdump -t -C), demangled and cut down to the spelling the launch ledger
reports (fhs_debug_launch_ledger): the kernel with its template arguments, without return type, namespace or
parameter list -- "k_modup_h<12, 3, true>".  tests/test_launch_coverage.py compares the committed file with the built
library, so an added or removed instantiation needs this script run again, and its GPU tests
then ask for an oracle-checked case that launches it."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dump  # noqa: E402

MANIFEST = os.path.join(HERE, "kernel_manifest.json")
KD = " (.kd)"   # how llvm-objdump -t -C prints the kernel descriptor symbol <mangled>.kd


def tools_present():
    return os.path.exists(isa_dump.OBJDUMP)


def normalise(demangled):
    """'void fhs::k_modup_h<12, 3, true>(fhs::DevTables, ...)' -> 'k_modup_h<12, 3, true>' (the rule of
    ledger_normalise in fhs_kernels.hip: cut the parameter list at the first '(' outside <>, then the return type
    at the last space outside <>, then the namespaces at the last '::' outside <>)."""
    def outside(s, tok, last):
        depth, found = 0, -1
        for i, c in enumerate(s):
            if c == "<":
                depth += 1
            elif c == ">":
                depth -= 1
            elif depth == 0 and s.startswith(tok, i):
                found = i
                if not last:
                    break
        return found
    s = demangled
    i = outside(s, "(", False)
    if i >= 0:
        s = s[:i]
    i = outside(s, " ", True)
    if i >= 0:
        s = s[i + 1:]
    i = outside(s, "::", True)
    if i >= 0:
        s = s[i + 2:]
    return s


def kernel_names(lib=None):
    """Sorted normalised names of the kernels in `lib` (default: the built library)."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(isa_dump.code_object(lib or isa_dump.LIB))
        f.flush()
        table = subprocess.run([isa_dump.OBJDUMP, "-t", "-C", f.name], capture_output=True, text=True,
                               check=True).stdout
    # "<address> <flags> <section>\t<size> <demangled name> (.kd)"
    full = [l.split("\t", 1)[1].split(" ", 1)[1][:-len(KD)] for l in table.splitlines() if l.endswith(KD)]
    names = [normalise(d) for d in full]
    assert len(names) == len(set(names)), "kernel names collide after normalisation"
    return sorted(names)


def main():
    names = kernel_names()
    with open(MANIFEST, "w") as f:
        json.dump({"kernels": names}, f, indent=0)
        f.write("\n")
    print(f"{len(names)} kernels -> {MANIFEST}")


if __name__ == "__main__":
    main()
