"""Short runs of the three by-hand fuzzers (tests/fuzz_parity.py, tests/fuzz_state.py, tests/fuzz_extreme.py) as part of the GPU
suite: a dozen random scenes against the oracle (plus table mode, view-mode rays, packing, caller-made tiles, shards, point
queries), a few dozen random state transitions of one context against fresh contexts, and sixteen scenes of extreme values."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_random_scenes_against_the_oracle():
    out = _run("fuzz_parity.py", 3, 16)
    assert len(re.findall(r"^case \d+:", out, re.M)) == 16
    assert "FAIL" not in out and "mismatch" not in out, out[-3000:]
    worst = float(re.search(r"worst vs oracle ([0-9.e+-]+)", out).group(1))
    assert worst <= 1e-4


def test_random_state_transitions_against_fresh_contexts():
    out = _run("fuzz_state.py", 5, 40)
    assert len(re.findall(r"^step \d+:", out, re.M)) == 40
    assert "mismatches: 0" in out, out[-3000:]


def test_extreme_values_against_the_oracle():
    """Optically thick media, sigma 1e-3 .. 3, negative and zero magnitudes, albedo above 1, Gaussians behind the camera and on the
    image plane; non-finite pixels must be non-finite on both sides.  Seed 6 draws each of the eight kinds within 16 cases."""
    out = _run("fuzz_extreme.py", 6, 16)
    cases = re.findall(r"^case \d+: (\w+)", out, re.M)
    assert len(cases) == 16
    assert set(cases) == {"thick", "tiny_sigma", "huge_sigma", "behind", "negmag", "bright", "zero_mag", "near_plane"}
    assert "FAIL" not in out and "failed cases: 0" in out, out[-3000:]
    worst = float(re.search(r"^worst ([0-9.e+-]+)", out, re.M).group(1))
    assert worst <= 1e-4
