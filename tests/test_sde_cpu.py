"""The stochastic (SDE) sampler without a GPU: the host rule (vc_sde_plan == transport.sde_plan), the torch restatement
(transport.sde_integrate) pinned to the reference's own Sampler.sample_sde, the refusals, the ABI, and Sampler.sample_sde on a
foreign callable.

The pin: tests/golden/sde_golden.npz holds what the reference's Sampler.sample_sde computed in float64 (tests/golden/make_sde_golden.py)
and the draws it made.  sde_integrate is held to it at 1e-12 of max |x| over the whole trajectory - the margin covers f64 sums taken
in another order over up to 16 steps (a few 1e-16 each).  Measured: 2.9e-16 at worst over the 28 cases."""
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW_SYMBOLS = ("vc_sde_plan", "vc_sde_stage", "vc_flux_sample_sde")


@pytest.fixture(scope="module")
def gen():
    """the fixture generator as a module: the toy model, the cases and the settings are defined there, once"""
    spec = importlib.util.spec_from_file_location("make_sde_golden", os.path.join(GOLDEN, "make_sde_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sde_golden.npz"))


def _grid(form, last, n, eps=0.0, lss=0.25):
    return torch.linspace(eps if form == "SBDM" else 0.0, 1 - lss if last else 1 - eps, n)


# ---------------------------------------------------------------------------------------------- 1. the reference pin
def test_sde_integrate_equals_the_reference_sampler_in_f64(gen, golden):
    from visualcloze_amd import transport as T
    x0 = torch.from_numpy(golden["x0"])
    cases = gen.cases()
    assert len(cases) == 28 and {c[1] for c in cases} == set(gen.FORMS)
    worst = 0.0
    for name, form, method, last, n in cases:
        lss = gen.LAST_STEP_SIZE if last else 0.0
        plan = T.sde_plan(method, form, gen.NORM, last, lss, _grid(form, last, n))
        draws = torch.from_numpy(golden[name + "_draws"])
        ref = torch.from_numpy(golden[name + "_states"])
        assert draws.shape[0] == plan["draws"] == n - 1 and ref.shape == (n,) + tuple(x0.shape)
        out = T.sde_integrate(lambda tau, y: gen.toy_model(y, tau), x0, plan, lambda d, shape: draws[d])
        assert out.dtype == torch.float64 and out.shape == ref.shape
        err = float((out - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, f"{name}: {err:.3e} of max |x|"
        if last is None:
            assert torch.equal(out[-1], out[-2])                 # no last step: the final row repeats the state
    print(f"[sde pin] worst |sde_integrate - reference| / max |x| over {len(cases)} cases: {worst:.3e}")


# ---------------------------------------------------------------------------------------------- 2. the host rule
@pytest.mark.parametrize("method", ["Euler", "Heun"])
@pytest.mark.parametrize("form", ["constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing"])
def test_c_plan_equals_python_plan_bitwise(form, method):
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    for last, n, lss in (("Mean", 13, 0.25), ("Euler", 7, 0.04), ("Tweedie", 250, 0.04)) + ((((None, 9, 0.0),) if method == "Euler" else ())):
        t = _grid(form, last, n, eps=1e-3, lss=lss)
        p, c = T.sde_plan(method, form, 0.7, last, lss, t), hip.sde_plan(method, form, 0.7, last, lss, t)
        E = (n - 1) * (2 if method == "Heun" else 1) + (1 if last else 0)
        assert p["evals"] == c["evals"] == E and p["draws"] == c["draws"] == n - 1
        assert p["rows"].shape == c["rows"].shape == (E + (method == "Heun"), 5) and p["rows"].dtype == np.float32
        assert np.array_equal(p["rows"].view(np.uint32), c["rows"].view(np.uint32)), (form, method, last)
        assert np.array_equal(p["times"].view(np.uint32), c["times"].view(np.uint32))
        assert np.isfinite(p["rows"]).all()
        # the model times: 1 - t in f32 at the step's start, and for Heun's second evaluation at t + dt
        t32 = t.numpy()
        step = 2 if method == "Heun" else 1
        assert np.array_equal(p["times"][:(n - 1) * step:step], np.float32(1.0) - t32[:-1])
        if method == "Heun":
            t2 = (t32[:-1].astype(np.float64) + (t32[1:] - t32[:-1]).astype(np.float64)).astype(np.float32)
            assert np.array_equal(p["times"][1:(n - 1) * 2:2], np.float32(1.0) - t2)
            assert list(p["rows"][:2 * (n - 1):2, 0]) == [hip.SDE_HEUN1] * (n - 1) and p["rows"][-1, 0] == hip.SDE_INJECT
            assert p["rows"][2 * (n - 1) - 1, 4] == 0.0              # no noise is injected behind the last loop step
        else:
            assert list(p["rows"][:n - 1, 0]) == [hip.SDE_EM] * (n - 1)
        if last:
            assert p["times"][-1] == np.float32(1.0) - t32[-1] and p["rows"][E - 1, 0] == hip.SDE_LAST
    # the alias of the reference's misspelt key
    if form == "inccreasing-decreasing":
        t = _grid(form, "Mean", 5)
        a, b = T.sde_plan(method, "increasing-decreasing", 1.0, "Mean", 0.25, t), hip.sde_plan(method, "increasing-decreasing", 1.0, "Mean", 0.25, t)
        assert np.array_equal(a["rows"], T.sde_plan(method, form, 1.0, "Mean", 0.25, t)["rows"]) and np.array_equal(a["rows"], b["rows"])


def test_plan_coefficients_are_the_formulas():
    """one Euler-Maruyama row and the last steps against the issue's formulas, in double, rounded once"""
    from visualcloze_amd import transport as T
    t = torch.tensor([0.25, 0.5, 0.75])
    p = T.sde_plan("Euler", "sigma", 0.7, "Mean", 0.25, t)
    w = 0.7 * (1 - 0.25)
    want = np.array([0, 0.25, 1 + w * 0.25 / 0.75, w / 0.75, math.sqrt(2 * w * 0.25)]).astype(np.float32)
    assert np.array_equal(p["rows"][0], want)
    w1 = 0.7 * 0.25
    assert np.array_equal(p["rows"][2], np.array([3, 0.25, 1 + w1 * 0.75 / 0.25, w1 / 0.25, 0]).astype(np.float32))
    assert np.array_equal(T.sde_plan("Euler", "sigma", 0.7, "Euler", 0.25, t)["rows"][2], np.array([3, 0.25, 1, 0, 0], np.float32))
    assert np.array_equal(T.sde_plan("Euler", "sigma", 0.7, "Tweedie", 0.125, t)["rows"][2], np.array([3, 0.25, 1, 0, 0], np.float32))
    c = T.sde_plan("Euler", "constant", 0.7, None, 0.0, t)         # implemented: the reference's TypeError is a bug
    assert c["evals"] == 2 and np.array_equal(c["rows"][1], np.array([0, 0.25, 1 + 0.7 * 0.5 / 0.5, 0.7 / 0.5, math.sqrt(2 * 0.7 * 0.25)]).astype(np.float32))


# ---------------------------------------------------------------------------------------------- 3. the refusals
def test_refusals_in_c_and_python():
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    L = hip.lib()

    def c_refuses(method, form, last, lss, t, match):
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*" + match):          # VC_ERR_ARG with a message
            hip.sde_plan(method, form, 1.0, last, lss, t)

    t01 = torch.linspace(0, 0.96, 8)
    # SBDM at eps 0: infinite at t0 = 0; the message names the time and the form
    c_refuses("Euler", "SBDM", "Mean", 0.04, t01, r"t = 0.*SBDM")
    with pytest.raises(ValueError, match=r"t = 0\.0.*SBDM.*sample_eps"):
        T.sde_plan("Euler", "SBDM", 1.0, "Mean", 0.04, t01)
    with pytest.raises(ValueError, match="sample_eps"):
        T.Sampler(T.create_transport()).sample_sde()                                 # the reference's default: refused, never NaN
    # ... and it runs with a sample_eps
    fn = T.Sampler(T.create_transport()).sample_sde(sample_eps=1e-3, num_steps=6)
    x = torch.randn(2, 3, 4, generator=torch.Generator().manual_seed(0))
    out = fn(x, lambda xin, timesteps: -xin * timesteps.view(-1, 1, 1))
    assert out.shape == (1, 2, 3, 4) and torch.isfinite(out).all()
    assert hip.sde_plan("Heun", "SBDM", 1.0, "Mean", 0.04, torch.linspace(1e-3, 0.96, 6))["evals"] == 11
    # Heun without a last step ends at t = 1
    t1 = torch.linspace(0, 1, 5)
    c_refuses("Heun", "sigma", None, 0.0, t1, r"t = 1.*sigma")
    with pytest.raises(ValueError, match=r"t = 1\.0.*sigma"):
        T.sde_plan("Heun", "sigma", 1.0, None, 0.0, t1)
    with pytest.raises(ValueError):
        T.Sampler(T.create_transport()).sample_sde(sampling_method="Heun", diffusion_form="sigma", last_step=None, num_steps=5)
    assert T.sde_plan("Euler", "sigma", 1.0, None, 0.0, t1)["evals"] == 4            # Euler never evaluates at t = 1
    # unknown names
    for args, match in ((("RK", "sigma", "Mean"), "method"), (("Euler", "sbdm", "Mean"), "form"), (("Euler", "sigma", "mean"), "last step")):
        c_refuses(args[0], args[1], args[2], 0.04, t01, match)
        with pytest.raises(NotImplementedError, match=match):
            T.sde_plan(args[0], args[1], 1.0, args[2], 0.04, t01)
    # a grid that does not increase strictly
    for bad in (torch.tensor([0.0, 0.5, 0.5, 0.9]), torch.tensor([0.0, 0.6, 0.5]), torch.tensor([0.3])):
        c_refuses("Euler", "sigma", "Mean", 0.04, bad, "t_grid|n_points")
        with pytest.raises(ValueError, match="increasing"):
            T.sde_plan("Euler", "sigma", 1.0, "Mean", 0.04, bad)
    # a capacity that is too small
    tg = (C_float * 4)(0.0, 0.25, 0.5, 0.75)
    rows = (C_float * 10)()
    assert L.vc_sde_plan(b"Euler", b"sigma", 1.0, b"Mean", 0.25, tg, 4, rows, None, 2, None, None) == -1
    assert b"capacity" in L.vc_last_error()


import ctypes  # noqa: E402

C_float = ctypes.c_float


# ---------------------------------------------------------------------------------------------- 4. the ABI
def test_abi_symbols_declared_bound_exported():
    from visualcloze_amd import hip
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    declared = set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NEW_SYMBOLS:
        assert name in declared and name in hip.SYMBOLS and name in exported, name
    L = hip.lib()
    assert L.vc_abi_version() == 11 and re.search(r"#define VC_ABI_VERSION 11\b", hdr)
    assert L.vc_solver_evals(3) == -1 and L.vc_solver_evals(100) == -1 and L.vc_solver_evals(101) == -1      # no VC_SOLVER_* value was added
    assert not re.search(r"#define VC_SOLVER_\w+ [3-9]", hdr) and set(hip.SOLVERS) == {"euler", "midpoint", "rk4"}
    for name, val in (("EM", 0), ("HEUN1", 1), ("HEUN2", 2), ("LAST", 3), ("INJECT", 4), ("ROW", 5)):
        assert re.search(rf"#define VC_SDE_{name} {val}\b", hdr) and getattr(hip, "SDE_" + name) == val
    assert "look up vc_sde_stage" in hdr


# ---------------------------------------------------------------------------------------------- 5. Sampler.sample_sde, eager, on the CPU
def test_sample_sde_on_a_foreign_callable():
    from visualcloze_amd import transport as T
    calls = []

    def model(xin, timesteps, scale=1.0):
        calls.append(float(timesteps[0]))
        assert xin.shape[-1] == 6 and timesteps.shape == (2,)            # x || cond
        return scale * torch.tanh(xin[..., :4]) * (0.5 + timesteps.view(-1, 1, 1))

    g = torch.Generator().manual_seed(3)
    x, cond = torch.randn(2, 3, 4, generator=g), torch.randn(2, 3, 2, generator=g)
    s = T.Sampler(T.create_transport())
    for method, evals in (("Euler", 5), ("Heun", 9)):
        opts = dict(sampling_method=method, diffusion_form="sigma", last_step="Mean", last_step_size=0.25, num_steps=5)
        torch.manual_seed(11)
        calls.clear()
        traj = s.sample_sde(return_trajectory=True, **opts)(x, model, cond=cond, scale=0.5)
        assert len(calls) == evals and calls[0] == 1.0 and calls[-1] == 0.25
        torch.manual_seed(11)
        last = s.sample_sde(**opts)(x, model, cond=cond, scale=0.5)
        assert traj.shape == (5, 2, 3, 4) and last.shape == (1, 2, 3, 4) and traj.dtype == x.dtype
        assert torch.equal(last[-1], traj[-1])                            # [-1] is the sample, as with the reference's list
        torch.manual_seed(12)
        other = s.sample_sde(**opts)(x, model, cond=cond, scale=0.5)
        assert not torch.equal(other, last) and torch.isfinite(traj).all()
    # an f64 caller is stepped in f64, a bf16 caller in f32 and rounded once per output
    torch.manual_seed(5)
    t64 = s.sample_sde(diffusion_form="linear", num_steps=4, return_trajectory=True)(x.double(), model, cond=cond.double())
    torch.manual_seed(5)
    t16 = s.sample_sde(diffusion_form="linear", num_steps=4, return_trajectory=True)(x.bfloat16(), model, cond=cond.bfloat16())
    assert t64.dtype == torch.float64 and t16.dtype == torch.bfloat16 and t16.shape == t64.shape == (4, 2, 3, 4)
    # a NoiseStream draws on the device: refused for a CPU state, never ignored
    class Stream:
        seed, offset = 1, 0
    with pytest.raises(ValueError, match="NoiseStream"):
        s.sample_sde(diffusion_form="linear", num_steps=4, rng=Stream())(x, model, cond=cond)
    # sample_ode is untouched: what it refused, it keeps refusing
    for m in ("dopri5", "Euler", "Heun", "sde"):
        with pytest.raises(NotImplementedError):
            s.sample_ode(sampling_method=m)
    assert s.transport.check_interval() == (0, 1)
    assert s.transport.check_interval(sde=True, diffusion_form="SBDM", last_step_size=0.04, sample_eps=1e-3) == (1e-3, 1 - 0.04)
    assert s.transport.check_interval(sde=True, diffusion_form="sigma", last_step_size=0.0) == (0, 1)
