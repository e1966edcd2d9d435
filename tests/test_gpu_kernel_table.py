"""GPU: the lazy table of fused programs (anr_capi.hip). A program's dynamic-LDS attribute is set before its own
first launch in the process; the fault this guards against is a missing attribute on a program that was not the
first of its group. Three fresh child processes (tests/_kernel_table_child.py), one after the other, each with a
different first fused launch, followed by the full 64-sample fp32 render; the children compare every output with
the oracle restatement at 1e-4."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

FIRST_CALLS = ('ns_image_x6', 'image_b16', 'alpha_x6')
LIMIT_S = 180  # per child: a few seconds of work plus the interpreter and library start-up


def test_first_launch_of_each_program_sets_its_own_attribute():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for which in FIRST_CALLS:  # a failing child ends the test: the following ones are not started
        res = subprocess.run([sys.executable, '-m', 'tests._kernel_table_child', which], cwd=root, capture_output=True,
                             text=True, timeout=LIMIT_S)
        print(res.stdout)
        assert res.returncode == 0, (which, res.stdout + res.stderr)
