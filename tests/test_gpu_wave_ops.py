"""csrc/wave_ops.h piece by piece: tests/micro/wave_ops_probe.hip wraps the lane-spread k-list (arrival order and keyed), the block
scan and extremes, the wave folds and numpy's pairwise sum in thin kernels and compares sweeps of them with host references written
in the same file, == on bits and integers.  The probe is built once for gfx950 and run once; each test reads its section's line
"<name>: cases N, mismatches M" and asserts M == 0 and N == the count computed here — a section that ran nothing fails."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c-users-sayakdutta-self-supervised-arbitrary-scale-point-cloud-upsampling-via-snn_amd", "csrc")
PATTERNS = 7


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path_factory.mktemp("wave_ops") / "wave_ops_probe")
    subprocess.run([hipcc, "-O3", "-ffp-contract=off", "--offload-arch=gfx950", "-I", CSRC, os.path.join(ROOT, "tests", "micro", "wave_ops_probe.hip"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return run.returncode, run.stdout + run.stderr


def _section(probe, name):
    code, out = probe
    m = re.search(r"^%s: cases (\d+), mismatches (\d+)$" % re.escape(name), out, re.M)
    assert m, "no line for section %r in the probe's output (exit status %d):\n%s" % (name, code, out)
    return int(m.group(1)), int(m.group(2)), out


def _candidate_counts(k):
    return {n for n in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, k - 1, k, k + 1) if n >= 1}


def test_arrival_order_list_at_every_k(probe):
    """WaveTopK<false> at k = 1..64 and WaveTopK<true> at k = 1..128, first_slab then offer, against std::stable_sort over the finite
    distances: every entry's distance bits and index, and tau."""
    cases, mismatches, out = _section(probe, "arrival-order list")
    assert mismatches == 0, out
    assert cases == PATTERNS * (sum(len(_candidate_counts(k)) for k in range(1, 65)) + sum(len(_candidate_counts(k)) for k in range(1, 129)))


def test_keyed_list_at_every_k(probe):
    """WaveTopK<false, true> at k = 1..64 under shuffled indices and padding mid-stream, against a sort by (distance, index)."""
    cases, mismatches, out = _section(probe, "keyed list")
    assert mismatches == 0, out
    assert cases == PATTERNS * sum(len(_candidate_counts(k)) for k in range(1, 65))


def test_block_collectives(probe):
    cases, mismatches, out = _section(probe, "block collectives")
    assert mismatches == 0, out
    widths = 5                                    # 1, 2, 4, 8, 16 waves
    scans = widths * 5                            # zeros, ones, random, a non-zero at the first / at the last lane of each wave
    extremes = widths * 2 * 4 * (1 + 2 + 2)       # min and max, four places, int (finite) and float, double (finite and infinite)
    folds = 5 * 64                                # wave_min / max / sum and the two uniform ones, the large term at every lane
    assert cases == scans + extremes + folds


def test_numpy_sum(probe):
    cases, mismatches, out = _section(probe, "numpy sum")
    assert mismatches == 0, out
    lengths = 1101 + 16 + 8                       # 0..1100, 8185..8200, 16377..16384
    assert cases == 2 * 129 + 2 * 2 * lengths + 1   # leaf sums (f32, f64), plan + fold (f32, f64; 64 and 512 leaves), the guard case


def test_the_probe_ended_well(probe):
    code, out = probe
    assert code == 0 and "HIP error" not in out, out
