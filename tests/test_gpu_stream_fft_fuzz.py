"""GPU: randomised check of device streams on the frequency-domain engine (tests/fuzz/fuzz_stream_fft.py) — random
ratio of the schedule table, dtype, channels and chunk plan; frame counts of the default stream, the engine's bars
globally and per seam, integer streams equal to the float stream plus the host output stage."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_fft_random_cases():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_stream_fft.py"), "24", "71"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "0 failures in 24 cases" in p.stdout
