"""The Adams-Bashforth multistep solve without a GPU: the host rule (vc_ms_plan == transport.ms_plan) against exact rational
arithmetic, the torch restatement (transport.multistep_integrate) and its order of convergence, the refusals, the ABI,
Sampler.sample_ode_multistep on a foreign callable, and the static check of csrc/multistep.hip.

The pin of the coefficients is `fractions.Fraction`: an f32 grid value is a rational, the Lagrange polynomials over such nodes have
rational coefficients, and so has their integral - no tolerance but the one f32 rounding of the result is involved."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vc_ms_plan", "vc_ms_stage", "vc_flux_sample_multistep", "vc_flux_plan_count")
ORDERS = (1, 2, 3, 4)


def _grids():
    """the pinned grids of test_host_cpu.py (two time-shifted ones, one SDEdit grid from strength 0.4), and one uniform grid whose
    values and step are exact in f32"""
    from visualcloze_amd.transport import solver_time_grid
    return {"shift30": solver_time_grid(30, 3456, 0, 1, True, 1), "shift4": solver_time_grid(4, 1152, 0, 1, True, 1),
            "sdedit": solver_time_grid(10, 4096, 0.4, 1, False, 1.0), "uniform": torch.arange(9, dtype=torch.float32) / 8}


# ---------------------------------------------------------------------------------------------- exact arithmetic
def _poly_mul(p, q):
    out = [Fraction(0)] * (len(p) + len(q) - 1)
    for a, pa in enumerate(p):
        for b, qb in enumerate(q):
            out[a + b] += pa * qb
    return out


def _poly_int(p, lo, hi):
    return sum(c * (hi ** (d + 1) - lo ** (d + 1)) / (d + 1) for d, c in enumerate(p))


def _exact_rows(order, t32):
    """c_{i,j} = the integral over [t_i, t_{i+1}] of the Lagrange polynomial of node t_{i-j} among t_i .. t_{i-k+1}, as Fractions"""
    tt = [Fraction(float(v)) for v in t32]
    rows = []
    for i in range(len(tt) - 1):
        k = min(order, i + 1)
        row = []
        for j in range(k):
            p = [Fraction(1)]
            for m in range(k):
                if m != j:
                    d = tt[i - j] - tt[i - m]
                    p = _poly_mul(p, [-tt[i - m] / d, 1 / d])
            row.append(_poly_int(p, tt[i], tt[i + 1]))
        rows.append(row)
    return rows


def _ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["shift30", "shift4", "sdedit", "uniform"])
def test_coefficients_against_exact_arithmetic(name, order):
    from visualcloze_amd import transport as T
    t = _grids()[name]
    t32 = t.numpy()
    rows = T.ms_plan(order, t)["rows"]
    exact = _exact_rows(order, t32)
    assert rows.dtype == np.float32 and rows.shape == (len(t32) - 1, 4)
    worst = 0.0
    for i, ex in enumerate(exact):
        assert len(ex) == min(order, i + 1)
        assert sum(ex) == Fraction(float(t32[i + 1])) - Fraction(float(t32[i]))          # the coefficients contain the step length
        for j in range(4):
            if j >= len(ex):
                assert rows[i, j] == 0.0 and not np.signbit(rows[i, j])                   # unused: exactly +0.0
                continue
            err = abs(Fraction(float(rows[i, j])) - ex[j])
            ulp = Fraction(_ulp32(float(ex[j])))
            worst = max(worst, float(err / ulp))
            assert err <= ulp, (name, order, i, j, float(ex[j]), float(rows[i, j]))
    print(f"[ms_plan] {name} order {order}: worst |f32 row - exact| = {worst:.3f} ulp")


def test_uniform_grid_gives_the_classical_coefficients():
    from visualcloze_amd import transport as T
    t = _grids()["uniform"]
    classical = {1: [1.0], 2: [3 / 2, -1 / 2], 3: [23 / 12, -16 / 12, 5 / 12], 4: [55 / 24, -59 / 24, 37 / 24, -9 / 24]}
    for order in ORDERS:
        rows = T.ms_plan(order, t, rounded=False)["rows"]
        assert rows.dtype == np.float64
        for i in range(len(rows)):
            k = min(order, i + 1)
            want = classical[k] + [0.0] * (4 - k)
            assert np.abs(rows[i] / 0.125 - np.array(want)).max() <= 1e-12, (order, i, rows[i] / 0.125)


def test_every_step_integrates_polynomials_exactly():
    """sum_j c_{i,j} p(t_{i-j}) = the integral of p over the step for every p of degree <= k_i - 1 (here the monomials around t_i,
    scaled by the step, so that every case has values of order one): the double rows against Fractions, 1e-12 relative"""
    from visualcloze_amd import transport as T
    t = _grids()["shift30"]
    tt = [Fraction(float(v)) for v in t.numpy()]
    for order in ORDERS:
        rows = T.ms_plan(order, t, rounded=False)["rows"]
        for i in range(len(tt) - 1):
            k = min(order, i + 1)
            h = tt[i + 1] - tt[i]
            for deg in range(k):
                p = lambda x: ((x - tt[i]) / h) ** deg  # noqa: E731
                exact = h / (deg + 1)
                got = sum(Fraction(float(rows[i, j])) * p(tt[i - j]) for j in range(k))
                scale = sum(abs(Fraction(float(rows[i, j])) * p(tt[i - j])) for j in range(k))
                assert abs(got - exact) <= Fraction(1, 10 ** 12) * max(scale, abs(exact)), (order, i, deg, float(got), float(exact))


# ---------------------------------------------------------------------------------------------- order of convergence
def test_order_of_convergence():
    """y' = -y^2 (1 + sin(3t) / 2), y(0) = 1, y(t) = 1 / (1 + t + (1 - cos 3t) / 6), in f64 to t = 1 on the grid t = u^2, u uniform
    with N = 16, 32, 64, 128 steps.
    Why this grid: the rule starts at the orders 1, 2, ... without extra evaluations, so the FIRST step is Euler's, with a local error
    of h_0^2 y'' / 2 that nothing later removes.  On a grid whose first step is of the size of the others (a uniform one, the
    sampler's shifted one) that term is O(h^2) and caps the observed order of k = 3 and 4 at 2 (measured on the uniform grid, last
    halving: 1.00, 1.97, 1.99, 2.09).  t = u^2 has first steps of O(h^2) - local start errors of O(h^4) - and bounded step ratios
    (3, 5/3, 7/5, ...), so the asymptotic order is the rule's own.  Observed orders of the last halving (64 -> 128 steps):
        k = 1: 1.01    k = 2: 1.99    k = 3: 3.25    k = 4: 4.13
    (k = 3 approaches 3 from above: 3.67, 3.43, 3.25 over the three halvings; k = 4: 4.35, 4.23, 4.13.)  Errors at 128 steps: 2.3e-3,
    2.9e-5, 1.5e-7, 2.9e-8 - far above f64 rounding."""
    from visualcloze_amd import transport as T
    f = lambda t, y: -y * y * (1 + math.sin(3 * t) * 0.5)  # noqa: E731
    exact = lambda t: 1.0 / (1.0 + t + (1 - math.cos(3 * t)) / 6)  # noqa: E731
    for k in ORDERS:
        errs = []
        for N in (16, 32, 64, 128):
            u = torch.arange(N + 1, dtype=torch.float64) / N
            t = (u * u).to(torch.float32)
            out = T.multistep_integrate(f, torch.tensor([1.0], dtype=torch.float64), t, k)
            assert out.dtype == torch.float64 and out.shape == (N + 1, 1)
            errs.append(abs(out[-1].item() - exact(float(t[-1]))))
        orders = [math.log2(errs[i] / errs[i + 1]) for i in range(3)]
        print(f"[multistep order] k = {k}: errors {['%.3e' % e for e in errs]}, observed orders {['%.2f' % o for o in orders]}")
        assert abs(orders[-1] - k) <= 0.5, (k, orders)


# ---------------------------------------------------------------------------------------------- C rule == Python rule, refusals
@pytest.mark.parametrize("order", ORDERS)
def test_c_plan_equals_python_plan_bitwise(order):
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    for name, t in _grids().items():
        p, c = T.ms_plan(order, t), hip.ms_plan(order, t)
        assert p["evals"] == c["evals"] == len(t) - 1
        assert p["rows"].shape == c["rows"].shape == (len(t) - 1, hip.MS_ROW) and c["rows"].dtype == np.float32
        assert np.array_equal(p["rows"].view(np.uint32), c["rows"].view(np.uint32)), (name, order)
        assert np.array_equal(p["times"].view(np.uint32), c["times"].view(np.uint32)), (name, order)
        assert np.array_equal(p["times"], np.float32(1.0) - t.numpy()[:-1])                 # the model's time: 1 - t_i in f32
        assert np.isfinite(p["rows"]).all()
    # the counts alone
    tg = (ctypes.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    n = ctypes.c_int32(0)
    assert hip.lib().vc_ms_plan(order, tg, 4, None, None, 0, ctypes.byref(n)) == 0 and n.value == 3


def test_refusals_in_c_and_python():
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    L = hip.lib()
    t = torch.tensor([0.0, 0.25, 0.5, 1.0])

    def both(order, grid, c_match, py_match):
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*ms_plan.*" + c_match):      # VC_ERR_ARG with a message
            hip.ms_plan(order, grid)
        with pytest.raises(ValueError, match="ms_plan.*" + py_match):
            T.ms_plan(order, grid)

    for order in (0, 5, -1):
        both(order, t, "order", "order")
    both(2, torch.tensor([0.3]), "n_points", "n_points")
    for bad in (torch.tensor([0.0, 0.5, 0.5, 0.9]), torch.tensor([0.0, 0.6, 0.5]), torch.tensor([0.0, float("nan"), 0.5])):
        both(2, bad, "increase strictly", "increase strictly")
    # a non-finite coefficient: a step 2^127 times its predecessor makes c_1 = -h^2 / (2 h_prev) overflow f32
    wild = torch.tensor([0.0, 2.0 ** -126, 2.0 ** 2])
    both(2, wild, "not finite", "not finite")
    assert hip.ms_plan(1, wild)["evals"] == 2                                                # order 1 has no such term
    # a capacity that is too small
    tg = (ctypes.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    rows, times = (ctypes.c_float * 16)(), (ctypes.c_float * 4)()
    assert L.vc_ms_plan(2, tg, 4, rows, None, 2, None) == -1 and b"capacity" in L.vc_last_error()
    assert L.vc_ms_plan(2, tg, 4, None, times, 2, None) == -1 and b"capacity" in L.vc_last_error()
    assert L.vc_ms_plan(2, tg, 4, rows, times, 3, None) == 0
    assert L.vc_ms_plan(2, None, 4, None, None, 0, None) == -1 and b"t_grid" in L.vc_last_error()


def test_abi_symbols_declared_bound_exported():
    from visualcloze_amd import hip
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    declared = set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NEW_SYMBOLS:
        assert name in declared and name in hip.SYMBOLS and name in exported, name
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", hdr)
        assert len(hip.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    L = hip.lib()
    assert L.vc_abi_version() == 11 and re.search(r"#define VC_ABI_VERSION 11\b", hdr)
    assert all(L.vc_solver_evals(code) == -1 for code in (3, 100, 104))                     # no VC_SOLVER_* value was added
    assert not re.search(r"#define VC_SOLVER_\w+ [3-9]", hdr) and set(hip.SOLVERS) == {"euler", "midpoint", "rk4"}
    assert re.search(r"#define VC_MS_ROW 4\b", hdr) and re.search(r"#define VC_MS_HIST 3\b", hdr) and (hip.MS_ROW, hip.MS_HIST) == (4, 3)
    assert "look up vc_ms_plan" in hdr
    assert L.vc_flux_plan_count(None) == -1


# ---------------------------------------------------------------------------------------------- the sampler, eager, on the CPU
def test_pinned_names_keep_raising_and_the_order_is_checked():
    from visualcloze_amd import transport as T
    s = T.Sampler(T.create_transport())
    for name in ("adams", "explicit_adams", "implicit_adams", "ab2", "ab4", "multistep", "heun3", "dopri5"):
        with pytest.raises(NotImplementedError):
            s.sample_ode(sampling_method=name)
    for order in (0, 5, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="order"):
            s.sample_ode_multistep(order=order)
    with pytest.raises(ValueError, match="f32 or f64"):
        T.multistep_integrate(lambda t, y: y, torch.zeros(2, dtype=torch.bfloat16), torch.linspace(0, 1, 3), 2)


def test_sample_ode_multistep_on_a_foreign_callable():
    from visualcloze_amd import transport as T
    calls = []

    def model(xin, timesteps, scale=1.0):
        calls.append(float(timesteps[0]))
        assert xin.shape[-1] == 6 and timesteps.shape == (2,)            # x || cond
        return scale * torch.tanh(xin[..., :4]) * (0.5 + timesteps.view(-1, 1, 1))

    g = torch.Generator().manual_seed(3)
    x, cond = torch.randn(2, 3, 4, generator=g), torch.randn(2, 3, 2, generator=g)
    s = T.Sampler(T.create_transport())
    for order in ORDERS:
        for strength in (None, 0.4):
            opts = dict(order=order, num_steps=7, do_shift=True, time_shifting_factor=1, strength=strength)
            calls.clear()
            traj = s.sample_ode_multistep(return_trajectory=True, **opts)(x, model, dict(cond=cond, scale=0.5))
            assert len(calls) == 6                                            # one evaluation per step
            last = s.sample_ode_multistep(**opts)(x, model, dict(cond=cond, scale=0.5))
            assert traj.shape == (7, 2, 3, 4) and last.shape == (1, 2, 3, 4) and traj.dtype == x.dtype
            assert torch.equal(traj[0], x) and torch.equal(last[0], traj[-1])
            # ... bit for bit multistep_integrate with the drift written out
            t = T.solver_time_grid(7, 3, 0.0 if strength is None else strength, 1, True, 1)
            assert calls[0] == float(np.float32(1.0) - t.numpy()[0])

            def drift(tv, y):
                tm = np.float32(1.0) - np.float32(tv)
                return -model(torch.cat((y, cond), dim=-1), torch.ones(2) * float(tm), scale=0.5)

            want = T.multistep_integrate(drift, x, t, order)
            assert torch.equal(traj, want), (order, strength)
    # the orders differ from one another from the second step on, and order 1 is Euler's rule up to its f32 roundings
    runs = {o: s.sample_ode_multistep(order=o, num_steps=7, return_trajectory=True)(x, model, dict(cond=cond)) for o in ORDERS}
    assert torch.equal(runs[1][1], runs[4][1]) and not torch.equal(runs[1][2], runs[2][2]) and not torch.equal(runs[3][4], runs[4][4])
    euler = s.sample_ode(sampling_method="euler", num_steps=7, return_trajectory=True)(x, model, dict(cond=cond))
    assert float((runs[1] - euler).abs().max()) <= 1e-5
    # an f64 caller is stepped in f64, a bf16 caller in f32 and rounded once per output
    t64 = s.sample_ode_multistep(order=3, num_steps=5, return_trajectory=True)(x.double(), model, dict(cond=cond.double()))
    t16 = s.sample_ode_multistep(order=3, num_steps=5, return_trajectory=True)(x.bfloat16(), model, dict(cond=cond.bfloat16()))
    assert t64.dtype == torch.float64 and t16.dtype == torch.bfloat16 and t16.shape == t64.shape == (5, 2, 3, 4)


def test_pipeline_refuses_the_conflicting_combinations():
    from visualcloze_amd import pipeline
    from visualcloze_amd.transport import StepCache
    ms = dict(order=3)
    for kw, match in ((dict(use_grid_handle=True), "use_grid_handle"), (dict(adaptive=dict(rtol=1e-2, atol=1e-6)), "adaptive"),
                      (dict(sde=dict(diffusion_form="sigma")), "sde"), (dict(step_cache=StepCache(0.1)), "step_cache"),
                      (dict(monitor=1), "monitor")):
        with pytest.raises(ValueError, match=r"multistep.*" + match):
            pipeline.generate_grid(None, None, None, None, [], [], None, None, 0, multistep=ms, **kw)


# ---------------------------------------------------------------------------------------------- the static check of the kernel
def test_multistep_hip_builds_without_warnings_scratch_or_spills(tmp_path):
    """csrc/multistep.hip cross-compiled for gfx950 with the library's flags: no warning, and the stage kernel's resource usage shows
    no scratch and no spilled register"""
    from visualcloze_amd import hip
    mk = open(os.path.join(hip.CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS = (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    rules = re.search(r"^RULES_FLAGS = (.*)$", mk, re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, *flags, *rules, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(hip.CSRC, "multistep.hip"),
                        "-o", str(tmp_path / "multistep.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warning:" not in r.stderr, r.stderr[-2000:]
    block = r.stderr[r.stderr.index("ms_stage_kernel"):]
    usage = {k: int(v) for k, v in re.findall(r"remark: [^\n]*?\b(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|SGPRs|LDS Size "
                                              r"\[bytes/block\]): (\d+)", block)}
    print(f"[multistep.hip] ms_stage_kernel: {usage}")
    assert usage["ScratchSize [bytes/lane]"] == 0 and usage["VGPRs Spill"] == 0 and usage["SGPRs Spill"] == 0
    assert usage["LDS Size [bytes/block]"] == 0
