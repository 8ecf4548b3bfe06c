#!/usr/bin/env python3
"""Writes tests/golden/bus_programs.txt: the message programs (AirBuilder.assemble_bus) of the restatements and the made-up table of
tests/bus_programs.py, as whitespace-separated numbers for tests/host/bus_program_check.cpp:

    <programs>  then per program:  name cols n_public block_log step n_regs  n_periodic plog..  n_values periodic values..
                                   n_consts consts..  n_code code..

usage: python tests/golden/make_bus_programs.py          (tests/test_bus_program_host.py checks that the file is current)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NAMES = ["leaf_noop", "transcript", "fri_fold", "merkle_open", "made_up"]
PATH = os.path.join(HERE, "bus_programs.txt")


def text():
    import bus_programs as BP

    out = [str(len(NAMES))]
    for name in NAMES:
        b = getattr(BP, name)()
        code, consts, n_regs = b.assemble_bus()
        vals = [v for col in b.periodic for v in col]
        out.append(" ".join(str(x) for x in [name, b.cols, b.n_public, b.bus_block_log, -1 if b.bus_step is None else b.bus_step, n_regs]))
        out.append(" ".join(str(x) for x in [len(b.periodic)] + [len(col).bit_length() - 1 for col in b.periodic]))
        out.append(" ".join(str(x) for x in [len(vals)] + vals))
        out.append(" ".join(str(int(x)) for x in [len(consts)] + list(consts)))
        out.append(" ".join(str(int(x)) for x in [len(code)] + list(code)))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(PATH, "w").write(text())
    print("wrote", PATH)
