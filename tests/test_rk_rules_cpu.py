"""CPU: the rk_* host rules of csrc/flux_rules.h against transport.rk_controller / rk_initial_step and the tableaus' stage times, bit
for bit.  tests/c_abi/rk_rules_check.cpp (its own main) takes the cases from here, runs the rules at the buffer sizes the engine passes
under AddressSanitizer and UBSan - a stand-alone host program, run directly - and prints hex floats.  Dormand-Prince is method 0 of
the same rules; tests/test_flux_rules_cpu.py holds them at order 5 to transport.dopri5_*."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from visualcloze_amd import transport

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

NAMES = {0: "dopri5", 1: "bosh3", 2: "adaptive_heun"}
ROWS = [(0.0, 0.0), (0.0, 1e-6), (0.3721, 0.0713), (0.9, 0.25)]
RATIOS = [0.0, 0.5, 0.9, 1.0, 1.0 + 2.0 ** -23, 7.0, 32.0, 1e9, 1e-12, float("nan")]
# (d0, d1, r = rms(f(t0 + h0) - f0)): the ordinary case twice, d0 < 1e-5, d1 < 1e-5, max(d1, d2) <= 1e-15
INITIAL = [(0.5, 0.25, 2.0 ** -10), (3.0, 0.125, 2.0 ** -4), (2.0 ** -20, 0.25, 2.0 ** -12), (0.5, 2.0 ** -20, 2.0 ** -30), (0.5, 2.0 ** -60, 0.0)]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    csrc = os.path.join(REPO, "visualcloze_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("rk_rules") / "rk_rules_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I" + csrc,
           os.path.join(REPO, "tests", "c_abi", "rk_rules_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    args = (["rows"] + [float(v).hex() for p in ROWS for v in p] + ["controller"] + [float(v).hex() for v in RATIOS]
            + ["initial"] + [float(v).hex() for c in INITIAL for v in c])
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip().endswith("rk rules ok"), r.stdout + r.stderr
    return [ln.split() for ln in r.stdout.strip().split("\n")]


def _bits(values) -> list:
    return [np.float64(v).tobytes() for v in values]


def test_row_times_are_the_tableaus(lines):
    rows = [ln for ln in lines if ln[0] == "rows"]
    assert len(rows) == 3 * len(ROWS)
    for ln in rows:
        tab = transport.RK_TABLEAUS[NAMES[int(ln[1])]]
        t, dt, *tm = [float.fromhex(w) for w in ln[2:]]
        assert len(tm) == len(tab["c"])
        assert _bits(tm) == _bits([float(np.float32(1) - np.float32(t + c * dt)) for c in tab["c"]])


def test_controller_is_transports(lines):
    ctl = [ln for ln in lines if ln[0] == "controller"]
    assert len(ctl) == 3 * len(RATIOS)
    for ln, (ratio, code) in zip(ctl, ((r, c) for r in RATIOS for c in (0, 1, 2))):
        order = transport.RK_TABLEAUS[NAMES[code]]["order"]
        assert int(ln[1]) == code
        if ratio != ratio:
            assert ln[2:] == ["nan", "refused"]
            with pytest.raises(transport.Dopri5Error):
                transport.rk_controller(1.0, ratio, order)
            continue
        accepted, dt_next = transport.rk_controller(1.0, ratio, order)
        assert (float.fromhex(ln[2]), int(ln[3]), _bits([float.fromhex(ln[4])])) == (ratio, int(accepted), _bits([dt_next])), (ratio, code)


def test_initial_step_is_transports(lines):
    ini = [ln for ln in lines if ln[0] == "initial"]
    assert len(ini) == 3 * len(INITIAL)
    branches = set()
    for ln in ini:
        order = transport.RK_TABLEAUS[NAMES[int(ln[1])]]["order"]
        d0, d1, r, h0, dt = [float.fromhex(w) for w in ln[2:]]
        # atol 1, rtol 0 and one f64 element: the norms ARE d0, d1 and r (sqrt(v * v) == v, (d1 + r) - d1 == r for these values)
        y0, f0 = torch.tensor([d0], dtype=torch.float64), torch.tensor([d1], dtype=torch.float64)
        assert (d1 + r) - d1 == r
        at = []
        want = transport.rk_initial_step(lambda t, y: (at.append(t), f0 + r)[1], 0.0, y0, f0, 0.0, 1.0, order)
        assert _bits([h0, dt]) == _bits([at[0], want])
        branches.add(("small" if d0 < 1e-5 or d1 < 1e-5 else "ratio", "flat" if max(d1, r / h0) <= 1e-15 else "slope"))
    assert branches == {("ratio", "slope"), ("small", "slope"), ("small", "flat")}
