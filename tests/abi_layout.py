"""The C compiler's layout of include/aerognn.h against the ctypes structs read from it."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_struct_layouts(structs, tmp_path):
    """For every struct of {C name: ctypes class}: sizeof, and offsetof and the size of every field,
    pads included, against a program gcc compiles from the header. Returns the number of values compared."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "aerognn.h"', 'int main(void){']
    for st, cls in structs.items():
        lines.append(f'printf("{st} sizeof %zu 0\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{st} {f} %zu %zu\\n", offsetof({st}, {f}), sizeof((({st}*)0)->{f}));')
    lines.append("return 0;}")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        st, f, off, size = line.split()
        cls = structs[st]
        got = (ctypes.sizeof(cls), 0) if f == "sizeof" else (getattr(cls, f).offset, getattr(cls, f).size)
        assert got == (int(off), int(size)), (st, f, got, off, size)
        seen += 1
    return seen
