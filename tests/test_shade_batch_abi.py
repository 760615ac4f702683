"""pt_shade_batch_io (include/ptamd.h) as the C compiler lays it out against its ctypes mirror (ptamd.device.ShadeBatchIO): every member at the same offset,
the density word's two members last, so that a caller built against the record of before reads and writes the members it knew where they were.
Runs without a GPU."""
import ctypes
import os
import subprocess

from ptamd import device as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MEMBERS = [name for name, _ in D.ShadeBatchIO._fields_]

PROBE = r"""
#include "ptamd.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    printf("%zu\n", sizeof(pt_shade_batch_io));
""" + "".join(f'    printf("{m} %zu\\n", offsetof(pt_shade_batch_io, {m}));\n' for m in MEMBERS) + r"""    return 0;
}
"""


def test_shade_batch_record_matches_its_mirror(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0]) == ctypes.sizeof(D.ShadeBatchIO)
    offsets = {name: int(off) for name, off in (line.split() for line in lines[1:] if line)}
    assert offsets == {name: getattr(D.ShadeBatchIO, name).offset for name in MEMBERS}
    # the density word's two members are the last two, in this order, behind the 42 the record held before (n, 17 inputs, sample, 23 outputs)
    assert MEMBERS[-2:] == ["in_pdf", "npdf"] and len(MEMBERS) == 44
    assert offsets["in_pdf"] == max(off for name, off in offsets.items() if name not in ("in_pdf", "npdf")) + 8 and offsets["npdf"] == offsets["in_pdf"] + 8
    assert int(lines[0]) == offsets["npdf"] + 8
