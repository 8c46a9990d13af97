"""CPU: the adaptive Dormand-Prince 5(4) solve in plain torch (transport.dopri5_integrate, the eager twin of vc_flux_sample_dopri5).

  * the tableau and ONE forced step - end state and dense output - against SciPy's RK45, to 1e-12 in f64.  SciPy's controller differs
    (safety factor, growth limits, steps clamped to the end time), so step SEQUENCES are not compared: the controller is
    torchdiffeq's as recalled, unpinned against real torchdiffeq;
  * accuracy against exact solutions, and more attempts at a tighter tolerance;
  * the controller's cases one by one;
  * the pinned names keep raising, and the new name exists and integrates a foreign callable."""
import math
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampler():
    from visualcloze_amd.transport import Sampler, create_transport
    return Sampler(create_transport("Linear", "velocity", do_shift=True))


# ---------------------------------------------------------------------------------------------- 1. SciPy
def test_tableau_equals_scipys():
    pytest.importorskip("scipy")
    import numpy as np
    from scipy.integrate._ivp.rk import RK45
    from visualcloze_amd import transport as T
    assert np.array_equal(np.array(T.DOPRI5_C), RK45.C)
    A = np.zeros((6, 5))
    for i, row in enumerate(T.DOPRI5_A):
        A[i + 1, :len(row)] = row
    assert np.array_equal(A, RK45.A)
    assert np.array_equal(np.array(T.DOPRI5_B), RK45.B)
    assert np.array_equal(np.array(T.DOPRI5_E), RK45.E)
    # the midpoint row is SciPy's dense-output polynomial at 1/2 (two ways to the same rationals: rounding apart)
    mid = np.array([sum(RK45.P[i, j] * 0.5 ** (j + 1) for j in range(4)) for i in range(7)])
    assert np.abs(mid - np.array(T.DOPRI5_C_MID)).max() < 1e-15


def test_one_forced_step_and_its_dense_output_equal_scipys():
    pytest.importorskip("scipy")
    import numpy as np
    from scipy.integrate._ivp.rk import RK45
    from visualcloze_amd import transport as T
    t0, h = 0.3, 0.17
    y0 = np.array([1.0, -0.5, 2.25])
    solver = RK45(lambda t, y: -2 * t * y + np.sin(t), t0, y0, t_bound=10.0, first_step=h, rtol=1e-1, atol=1e-1)   # loose: h is accepted
    assert solver.step() is None and solver.t == t0 + h, "SciPy rejected the forced step: the comparison would be of another step"
    dense = solver.dense_output()

    f = lambda t, y: -2 * t * y + math.sin(t)  # noqa: E731
    ty0 = torch.tensor(y0, dtype=torch.float64)
    y1, ks = T.dopri5_step(f, t0, h, ty0, f(t0, ty0))
    assert np.abs(y1.numpy() - solver.y).max() < 1e-12
    for theta in (0.1, 0.5, 0.9):
        got = T.dopri5_interp(ty0, y1, ks, h, theta).numpy()
        assert np.abs(got - dense(t0 + theta * h)).max() < 1e-12, theta
    assert torch.equal(T.dopri5_interp(ty0, y1, ks, h, 0.0), ty0) and torch.equal(T.dopri5_interp(ty0, y1, ks, h, 1.0), y1)
    # the error estimate is SciPy's too: its norm over scale = atol + rtol * max(|y0|, |y1|)
    rtol, atol = 1e-3, 1e-6
    K = np.stack([k.numpy() for k in ks])
    want = np.linalg.norm((K.T @ RK45.E) * h / (atol + rtol * np.maximum(np.abs(y0), np.abs(solver.y)))) / 3 ** 0.5
    assert abs(T.dopri5_error_ratio(ty0, y1, ks, h, rtol, atol) - want) < 1e-12 * want


# ---------------------------------------------------------------------------------------------- 2. exact solutions
ODES = {"decay": (lambda t, y: -y, lambda y0, t: y0 * math.exp(-t)),
        "logistic": (lambda t, y: y * (1 - y), lambda y0, t: y0 * math.exp(t) / (1 - y0 + y0 * math.exp(t)))}
GRID = [0.0, 0.5, 1.0, 1.5, 2.0]
Y0 = [0.1, 0.5, 0.9]
ATOL = 1e-6


def test_scipy_itself_stays_inside_the_allowance():
    """the allowance of the next test - global error <= 10 (atol + rtol |y|) - holds for SciPy's own RK45 on these inputs"""
    pytest.importorskip("scipy")
    import numpy as np
    from scipy.integrate import solve_ivp
    for name, (f, exact) in ODES.items():
        for rtol in (1e-3, 1e-6):
            sol = solve_ivp(f, (GRID[0], GRID[-1]), np.array(Y0), method="RK45", t_eval=GRID, rtol=rtol, atol=ATOL)
            for i, t in enumerate(GRID):
                ex = np.array([exact(y, t) for y in Y0])
                assert (np.abs(sol.y[:, i] - ex) <= 10 * (ATOL + rtol * np.abs(ex))).all(), (name, rtol, t)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", sorted(ODES))
def test_global_error_against_the_exact_solution(name, dtype):
    from visualcloze_amd.transport import dopri5_integrate
    f, exact = ODES[name]
    y0 = torch.tensor(Y0, dtype=dtype)
    # an f32 state resolves 6e-8 |y|: rtol = 1e-6 is sixteen of its ulps, and the allowance ten times that
    attempts = {}
    for rtol in (1e-3, 1e-6):
        log = []
        out = dopri5_integrate(f, y0, GRID, rtol=rtol, atol=ATOL, log=log)
        assert out.dtype == dtype and out.shape == (len(GRID), len(Y0)) and torch.equal(out[0], y0)
        ex = torch.tensor([[exact(float(y), t) for y in y0] for t in GRID], dtype=torch.float64)
        err = (out.double() - ex).abs()
        worst = (err / (10 * (ATOL + rtol * ex.abs()))).max().item()
        print(f"\n{name} {dtype} rtol {rtol:g}: {len(log)} attempts, {sum(1 for a in log if not a[3])} rejected, error / allowance {worst:.3f}")
        assert worst <= 1.0
        attempts[rtol] = len(log)
        assert all(a[3] == (a[2] <= 1.0) for a in log)
        t_end = [a[0] + a[1] for a in log if a[3]][-1]
        assert t_end >= GRID[-1]                      # not clamped: the last step may run past the last output time
    assert attempts[1e-6] > attempts[1e-3]


def test_outputs_inside_one_step_come_from_the_dense_output():
    from visualcloze_amd.transport import dopri5_integrate
    grid = [0.0, 0.01, 0.02, 0.03, 1.0]
    log, calls = [], []
    out = dopri5_integrate(lambda t, y: (calls.append(t), -y)[1], torch.tensor([1.0], dtype=torch.float64), grid, rtol=1e-6, atol=1e-9, log=log)
    assert len(calls) == 2 + 6 * len(log)                                  # k1, the probe of the first step size, six per attempt
    assert sum(1 for a in log if a[3]) < 20                                # far fewer steps than a clamp at every output would need
    ex = torch.tensor([[math.exp(-t)] for t in grid], dtype=torch.float64)
    assert ((out - ex).abs() <= 10 * (1e-9 + 1e-6 * ex)).all()


# ---------------------------------------------------------------------------------------------- 3. the controller
def test_controller_cases():
    from visualcloze_amd.transport import Dopri5Error, dopri5_controller, dopri5_integrate
    dt = 0.125
    assert dopri5_controller(dt, 0.0) == (True, 1.25)                                      # ratio 0: the largest growth
    acc, nxt = dopri5_controller(dt, 0.5)                                                  # ratio < 1: accepted, never shrinks
    assert acc and nxt == dt * (0.9 / math.pow(0.5, 0.2)) and nxt > dt
    acc, nxt = dopri5_controller(dt, 0.9)
    assert acc and nxt == dt * 1.0                                                         # 0.9 / 0.9^(1/5) < 1: held at 1
    assert dopri5_controller(dt, 1e-12) == (True, dt * 10.0)                               # growth capped at 10
    assert dopri5_controller(dt, 1.0) == (True, dt * 0.9)                                  # ratio = 1: accepted, the safety factor
    acc, nxt = dopri5_controller(dt, 32.0)                                                 # ratio > 1: rejected
    assert not acc and nxt == dt * (0.9 / math.pow(32.0, 0.2))
    assert dopri5_controller(dt, 1e9) == (False, dt * 0.2)                                 # shrink capped at 0.2
    with pytest.raises(Dopri5Error, match="NaN"):
        dopri5_controller(dt, float("nan"))
    y0 = torch.tensor([1.0], dtype=torch.float64)
    with pytest.raises(Dopri5Error, match="NaN"):
        dopri5_integrate(lambda t, y: y * float("nan") if t > 0.5 else -y, y0, [0.0, 1.0], forced_dts=[0.9])
    with pytest.raises(Dopri5Error, match="max_attempts"):
        dopri5_integrate(lambda t, y: -50 * y, y0, [0.0, 1.0], rtol=1e-8, atol=1e-10, max_attempts=3)
    with pytest.raises(Dopri5Error, match="underflowed"):
        dopri5_integrate(lambda t, y: -y, y0, [1e20, 2e20], forced_dts=[1.0])


def test_forced_attempts_replay_a_run():
    from visualcloze_amd.transport import dopri5_integrate
    f = lambda t, y: -2 * t * y + math.sin(t)  # noqa: E731
    y0 = torch.tensor([1.0, -0.5, 2.25], dtype=torch.float32)
    grid = [0.0, 0.4, 1.1, 2.0]
    log = []
    out = dopri5_integrate(f, y0, grid, rtol=1e-5, atol=1e-7, log=log)
    for forced in ([a[1] for a in log], [(a[1], a[3]) for a in log]):
        log2 = []
        again = dopri5_integrate(f, y0, grid, rtol=1e-5, atol=1e-7, forced_dts=forced, log=log2)
        assert torch.equal(again, out) and log2 == log
    # every logged dt is the controller's answer to the attempt before it
    from visualcloze_amd.transport import dopri5_controller
    for a, b in zip(log, log[1:]):
        assert dopri5_controller(a[1], a[2]) == (a[3], b[1])


# ---------------------------------------------------------------------------------------------- 4. the names
def test_pinned_names_keep_raising_and_the_new_name_integrates():
    from visualcloze_amd import hip
    s = _sampler()
    with pytest.raises(NotImplementedError):
        s.sample_ode(sampling_method="dopri5")
    with pytest.raises(NotImplementedError):
        s.sample_ode()                                                     # the reference's default IS dopri5
    if os.path.exists(hip.LIB_PATH):
        with pytest.raises(hip.VclozeHipError):
            hip.solver_evals("dopri5")
        assert "dopri5" not in hip.SOLVERS
    # the new name: a foreign callable, y' = -(1 + t) y through the sampler's drift f = -model(y, 1 - t)
    assert s.last_adaptive_log is None
    y0 = torch.linspace(0.5, 2.0, 16, dtype=torch.float64).reshape(1, 8, 2)

    def model(y, timesteps, **kw):
        t = (1 - timesteps.double())[:, None, None]
        return (1 + t) * y
    fn = s.sample_ode_adaptive(num_steps=5, rtol=1e-6, atol=1e-9, do_shift=False, time_shifting_factor=None, return_trajectory=True)
    out = fn(y0, model, {})
    assert out.dtype == torch.float64 and out.shape == (5, 1, 8, 2) and torch.equal(out[0], y0)
    for i, t in enumerate((0.25, 0.5, 0.75, 1.0)):
        ex = y0 * math.exp(-(t + t * t / 2))
        # the model sees 1 - f32(t): ~1e-7 of perturbation in t on top of the tolerance's allowance
        assert ((out[i + 1] - ex).abs() <= 10 * (1e-9 + 1e-6 * ex.abs()) + 1e-6 * ex.abs()).all(), t
    (log,) = s.last_adaptive_log
    assert log["evaluations"] == 2 + 6 * len(log["attempts"]) and log["rejected"] == sum(1 for a in log["attempts"] if not a[3])
    last = s.sample_ode_adaptive(num_steps=5, rtol=1e-6, atol=1e-9, do_shift=False, time_shifting_factor=None)(y0, model, {})
    assert last.shape == (1, 1, 8, 2) and torch.equal(last[0], out[-1])
    # a bf16 caller: stepped in f32, rounded once per output (the model is handed the state in the CALLER's dtype; one that rounds
    # its input to bf16 itself, as Flux's img_in does, cannot tell the two callers apart)
    rounding = lambda y, timesteps, **kw: model(y.to(torch.bfloat16).float(), timesteps)  # noqa: E731
    o16 = fn(y0.to(torch.bfloat16), rounding, {})
    o32 = fn(y0.to(torch.bfloat16).float(), rounding, {})
    assert o16.dtype == torch.bfloat16 and torch.equal(o16, o32.to(torch.bfloat16))
