"""Which kernel instantiation every launch runs: each pick function (csrc/mrt_pick.h) over
its whole argument domain, against tests/golden/kernel_picks.txt.  The GPU suite pins bits,
and every variant of a family gives the same bits; this pins the variant -- its occupancy
target, walk form and scene kind.  The fixture is the output of the same program built
against the parent commit's library, and is regenerated only from a parent build, and read
by hand, when a pick changes on purpose ("Kernel variants").  No GPU needed:
the program asks the dynamic linker for the returned pointers' symbol names."""
import os
import shutil
import subprocess

import pytest

from miro import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


def test_kernel_picks(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    lib = os.path.abspath(_lib.LIB_PATH)
    exe = str(tmp_path / "kernel_picks")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "kernel_picks.cpp"), lib, "-ldl",
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True, capture_output=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = open(os.path.join(HERE, "golden", "kernel_picks.txt")).read().splitlines()
    diff = ["line %d: got  %s\n%s want %s" % (i + 1, g, " " * len("line %d:" % (i + 1)), w)
            for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not diff, "%d lines (fixture %d), %d differ; the first:\n%s" % (
        len(got), len(want), len(diff), "\n".join(diff[:10]))
    assert not [g for g in got if g.endswith("-> ?")], "a pick returned a pointer that is no exported kernel"
