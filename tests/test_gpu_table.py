"""The table kernel (csrc/vrt_table_kernel.hip) on its own limits, in both of its shapes: every table size of its menu at both ends
of its band, two, three and eight segments and the decline limit, the stage and gather edges (63 .. 65, 127 .. 129, 257 survivors
for 16 waves; 63 .. 65, 127 .. 129, 511 .. 513 for 8), the four Exp / Erf pairs it takes and two it must leave to the exact kernels,
a second attempt that succeeds, and the library's defaults.  Cases, what each asserts and the runner: tests/table_cases.py; scenes
and the float64 model they are held against: tests/table_scenes.py; that the cases can see what they should:
tests/test_table_scenes.py.

Frames of 256 rays take the 16-wave shape, and the library reads VRT_HIP_TABLE_WAVES once per process: the 16-wave cases run in
this process, the 8-wave cases in ONE child started with VRT_HIP_TABLE_WAVES=8 (`table_nodes` proves which shape ran: the
multi-segment node counts differ between the shapes).  The child (python start, oracle scenes, 43 cases on contexts of their
own) has not been timed on an MI355X yet: CHILD_TIMEOUT is a provisional limit, to be sized from the first measured run (the
runner prints its time in its last line) and the figure written here.
"""
import os
import subprocess
import sys

import pytest

import table_cases as TC

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120


@pytest.mark.parametrize("group", TC.GROUPS)
def test_table_kernel_16_waves(pkg, oracle, group):
    assert "VRT_HIP_TABLE_WAVES" not in os.environ      # read once per process: the 16-wave shape is the default at this frame size
    failed = TC.run(pkg, oracle, 16, (group,), out=lambda s: print(s, flush=True))
    assert not failed, failed


def test_table_kernel_8_waves():
    child = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "table_cases.py"), "8"],
                           env={**os.environ, "VRT_HIP_TABLE_WAVES": "8"}, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    print(child.stdout, child.stderr, sep="\n", flush=True)
    assert child.returncode == 0, child.stdout[-4000:] + child.stderr[-2000:]
    assert child.stdout.count(" ok\n") == len([ln for ln in child.stdout.splitlines() if ln.startswith("waves=8 ")]) > 40
