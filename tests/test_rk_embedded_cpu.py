"""CPU: the embedded Runge-Kutta pairs bosh3 and adaptive_heun in plain torch (transport.rk_integrate, the eager twin of
vc_flux_sample_rk).

  * bosh3: the tableau and ONE forced step - end state, error ratio and dense output - against SciPy's RK23, to 1e-12 in f64;
  * adaptive_heun: one step against the closed form, and a whole run against a numpy adaptive Heun written here, independent of
    transport.py;
  * the step-size rules at order 5 return what the dopri5_* rules return;
  * global error against exact solutions inside an allowance SciPy's own RK23 is first shown to keep;
  * forced replays, the error cases, the names.
SciPy's controller differs (safety factor, growth limits, steps clamped to the end time), so step SEQUENCES are not compared with it:
the controller is torchdiffeq's as recalled, unpinned against real torchdiffeq."""
import math

import pytest
import torch

from tests.test_dopri5_cpu import ATOL, GRID, ODES, Y0

PAIRS = ["bosh3", "adaptive_heun"]
RTOLS = (1e-3, 1e-5)


def _sampler():
    from visualcloze_amd.transport import Sampler, create_transport
    return Sampler(create_transport("Linear", "velocity", do_shift=True))


# ---------------------------------------------------------------------------------------------- 1. bosh3 against SciPy
def test_bosh3_tableau_equals_scipys():
    pytest.importorskip("scipy")
    import numpy as np
    from scipy.integrate._ivp.rk import RK23
    from visualcloze_amd import transport as T
    tab = T.RK_TABLEAUS["bosh3"]
    assert tab["order"] == 3 and len(tab["c"]) == 4 and tab["c"][3] == 1.0
    assert np.array_equal(np.array(tab["c"][:3]), RK23.C)
    A = np.zeros((3, 3))
    for i, row in enumerate(tab["a"]):
        A[i + 1, :len(row)] = row
    assert np.array_equal(A, RK23.A)
    assert np.array_equal(np.array(tab["b"]), RK23.B)
    assert np.array_equal(np.array(tab["e"]), RK23.E)
    heun = T.RK_TABLEAUS["adaptive_heun"]
    assert (heun["order"], heun["c"], heun["a"], heun["b"], heun["e"]) == (2, (0.0, 1.0, 1.0), ((1.0,),), (0.5, 0.5), (0.5, -0.5, 0.0))
    assert T.RK_TABLEAUS["dopri5"]["a"] == T.DOPRI5_A and T.RK_TABLEAUS["dopri5"]["e"] == T.DOPRI5_E


def test_one_forced_bosh3_step_and_its_dense_output_equal_scipys():
    pytest.importorskip("scipy")
    import numpy as np
    from scipy.integrate._ivp.rk import RK23
    from visualcloze_amd import transport as T
    t0, h = 0.3, 0.17
    y0 = np.array([1.0, -0.5, 2.25])
    solver = RK23(lambda t, y: -2 * t * y + np.sin(t), t0, y0, t_bound=10.0, first_step=h, rtol=1e-1, atol=1e-1)   # loose: h is accepted
    assert solver.step() is None and solver.t == t0 + h, "SciPy rejected the forced step: the comparison would be of another step"
    dense = solver.dense_output()

    f = lambda t, y: -2 * t * y + math.sin(t)  # noqa: E731
    ty0 = torch.tensor(y0, dtype=torch.float64)
    y1, ks = T.rk_step(f, t0, h, ty0, f(t0, ty0), "bosh3")
    assert len(ks) == 4 and np.abs(y1.numpy() - solver.y).max() < 1e-12
    for theta in (0.1, 0.5, 0.9):
        got = T.rk_hermite(ty0, y1, ks, h, theta).numpy()
        assert np.abs(got - dense(t0 + theta * h)).max() < 1e-12, theta
    assert torch.equal(T.rk_hermite(ty0, y1, ks, h, 0.0), ty0) and torch.equal(T.rk_hermite(ty0, y1, ks, h, 1.0), y1)
    # the error estimate is SciPy's too: its norm over scale = atol + rtol * max(|y0|, |y1|)
    rtol, atol = 1e-3, 1e-6
    K = np.stack([k.numpy() for k in ks])
    want = np.linalg.norm((K.T @ RK23.E) * h / (atol + rtol * np.maximum(np.abs(y0), np.abs(solver.y)))) / 3 ** 0.5
    assert abs(T.rk_error_ratio(ty0, y1, ks, h, rtol, atol, "bosh3") - want) < 1e-12 * want


# ---------------------------------------------------------------------------------------------- 2. adaptive_heun against the closed form
def test_one_adaptive_heun_step_equals_the_closed_form():
    from visualcloze_amd import transport as T
    t0, h = 0.3, 0.17
    f = lambda t, y: -2 * t * y + math.sin(t)  # noqa: E731
    y0 = torch.tensor([1.0, -0.5, 2.25], dtype=torch.float64)
    k1 = f(t0, y0)
    k2 = f(t0 + h, y0 + h * k1)
    y1, ks = T.rk_step(f, t0, h, y0, k1, "adaptive_heun")
    want = y0 + h / 2 * (k1 + k2)
    assert len(ks) == 3 and (y1 - want).abs().max() < 1e-12
    assert (ks[1] - k2).abs().max() < 1e-12 and (ks[2] - f(t0 + h, want)).abs().max() < 1e-12
    rtol, atol = 1e-3, 1e-6
    err = h / 2 * (k1 - k2)
    ratio = float(((err / (atol + rtol * torch.maximum(y0.abs(), want.abs()))) ** 2).mean().sqrt())
    assert abs(T.rk_error_ratio(y0, y1, ks, h, rtol, atol, "adaptive_heun") - ratio) < 1e-12 * ratio
    mid = T.rk_hermite(y0, y1, ks, h, 0.5)
    assert (mid - ((y0 + y1) / 2 + h / 8 * (ks[0] - ks[2]))).abs().max() < 1e-12
    assert torch.equal(T.rk_hermite(y0, y1, ks, h, 0.0), y0) and torch.equal(T.rk_hermite(y0, y1, ks, h, 1.0), y1)
    # the f32 expression is the same cubic (to f32's resolution), and its ends are the ends
    y32, y132, k32 = y0.float(), y1.float(), [k.float() for k in ks]
    assert (T.rk_hermite(y32, y132, k32, h, 0.5).double() - mid).abs().max() < 1e-6
    assert torch.equal(T.rk_hermite(y32, y132, k32, h, 1.0), y132)


def _numpy_adaptive_heun(f, y0, grid, rtol, atol):
    """adaptive Heun-Euler 2(1) with the first-step search and the controller vcloze_hip.h states (exponent 1/2), in numpy f64:
    -> (outputs at grid, attempts [(t, dt, accepted)])"""
    import numpy as np
    rms = lambda a: float(np.sqrt(np.mean(a * a)))  # noqa: E731
    t, y, k1 = grid[0], np.array(y0, dtype=np.float64), None
    k1 = f(t, y)
    scale = atol + rtol * np.abs(y)
    d0, d1 = rms(y / scale), rms(k1 / scale)
    h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    d2 = rms((f(t + h0, y + h0 * k1) - k1) / scale) / h0
    dt = min(100 * h0, max(1e-6, h0 * 1e-3) if max(d1, d2) <= 1e-15 else (0.01 / max(d1, d2)) ** 0.5)
    outs, att, nxt = [y.copy()], [], 1
    while nxt < len(grid):
        k2 = f(t + dt, y + dt * k1)
        y1 = y + dt * (0.5 * k1 + 0.5 * k2)
        k3 = f(t + dt, y1)
        ratio = rms(dt * (0.5 * k1 - 0.5 * k2) / (atol + rtol * np.maximum(np.abs(y), np.abs(y1))))
        att.append((t, dt, ratio <= 1.0))
        if ratio <= 1.0:
            while nxt < len(grid) and grid[nxt] <= t + dt:
                x = min(1.0, max(0.0, (grid[nxt] - t) / dt))
                outs.append((1 - x) * y + x * y1 + x * (x - 1) * ((1 - 2 * x) * (y1 - y) + (x - 1) * dt * k1 + x * dt * k3))
                nxt += 1
            t, y, k1 = t + dt, y1, k3
        dt *= 10.0 if ratio == 0.0 else min(10.0, max(0.9 / ratio ** 0.5, 1.0 if ratio < 1.0 else 0.2))
    return np.stack(outs), att


# ---------------------------------------------------------------------------------------------- 3. the order-5 rules
def test_order_5_rules_return_what_the_dopri5_rules_return():
    from visualcloze_amd import transport as T
    dt = 0.125
    for ratio in (0.0, 0.5, 0.9, 1e-12, 1.0, 32.0, 1e9):                                   # the case list of test_controller_cases
        assert T.rk_controller(dt, ratio, 5) == T.dopri5_controller(dt, ratio), ratio
    with pytest.raises(T.Dopri5Error, match="NaN"):
        T.rk_controller(dt, float("nan"), 5)
    # order 3 and 2: the same clamps, the exponent 1 / order
    assert T.rk_controller(dt, 0.5, 3) == (True, dt * (0.9 / math.pow(0.5, 1 / 3))) and T.rk_controller(dt, 0.9, 2) == (True, dt)
    assert T.rk_controller(dt, 32.0, 2) == (False, dt * 0.2) and T.rk_controller(dt, 4.0, 2) == (False, dt * 0.45)
    assert T.rk_controller(dt, 1.0, 3) == (True, dt * 0.9) and T.rk_controller(dt, 0.0, 2) == (True, 1.25)
    # five (d0, d1, d2 h0) triples through atol 1, rtol 0 and one f64 element, where the norms ARE the values
    for d0, d1, r in ((0.5, 0.25, 2.0 ** -10), (3.0, 0.125, 2.0 ** -4), (2.0 ** -20, 0.25, 2.0 ** -12), (0.5, 2.0 ** -20, 2.0 ** -30),
                      (0.5, 2.0 ** -60, 0.0)):
        y0, f0 = torch.tensor([d0], dtype=torch.float64), torch.tensor([d1], dtype=torch.float64)
        a, b = [], []
        got = T.rk_initial_step(lambda t, y: (a.append(t), f0 + r)[1], 0.0, y0, f0, 0.0, 1.0, 5)
        want = T.dopri5_initial_step(lambda t, y: (b.append(t), f0 + r)[1], 0.0, y0, f0, 0.0, 1.0)
        assert (got, a) == (want, b), (d0, d1, r)


# ---------------------------------------------------------------------------------------------- 4. global error
def test_scipys_rk23_itself_stays_inside_the_allowance():
    """the allowance of the bosh3 test - global error <= 10 (atol + rtol |y|) - holds for SciPy's own RK23 on these inputs"""
    pytest.importorskip("scipy")
    import numpy as np
    from scipy.integrate import solve_ivp
    for name, (f, exact) in ODES.items():
        for rtol in RTOLS:
            sol = solve_ivp(f, (GRID[0], GRID[-1]), np.array(Y0), method="RK23", t_eval=GRID, rtol=rtol, atol=ATOL)
            for i, t in enumerate(GRID):
                ex = np.array([exact(y, t) for y in Y0])
                worst = (np.abs(sol.y[:, i] - ex) / (10 * (ATOL + rtol * np.abs(ex)))).max()
                print(f"\nRK23 {name} rtol {rtol:g} t {t}: error / allowance {worst:.3f}")
                assert worst <= 1.0, (name, rtol, t)


def _solve(method, name, dtype, rtol):
    from visualcloze_amd.transport import rk_integrate
    f, exact = ODES[name]
    y0 = torch.tensor(Y0, dtype=dtype)
    log, calls = [], []
    out = rk_integrate(lambda t, y: (calls.append(t), f(t, y))[1], y0, GRID, method, rtol=rtol, atol=ATOL, log=log)
    assert out.dtype == dtype and out.shape == (len(GRID), len(Y0)) and torch.equal(out[0], y0)
    ex = torch.tensor([[exact(float(y), t) for y in y0] for t in GRID], dtype=torch.float64)
    worst = ((out.double() - ex).abs() / (ATOL + rtol * ex.abs())).max().item()
    assert all(a[3] == (a[2] <= 1.0) for a in log)
    assert [a[0] + a[1] for a in log if a[3]][-1] >= GRID[-1]              # not clamped: the last step may run past the last output time
    return out, log, len(calls), worst


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", sorted(ODES))
def test_bosh3_global_error_against_the_exact_solution(name, dtype):
    attempts = {}
    for rtol in RTOLS:
        _, log, calls, worst = _solve("bosh3", name, dtype, rtol)
        print(f"\nbosh3 {name} {dtype} rtol {rtol:g}: {len(log)} attempts, {sum(1 for a in log if not a[3])} rejected, error / allowance "
              f"{worst / 10:.3f}")
        assert worst <= 10.0                                               # global error <= 10 (atol + rtol |y|)
        assert calls == 2 + 3 * len(log)                                   # k1, the probe of the first step size, three per attempt
        attempts[rtol] = len(log)
    assert attempts[1e-5] > attempts[1e-3]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", sorted(ODES))
def test_adaptive_heun_against_a_numpy_twin_and_the_exact_solution(name, dtype):
    import numpy as np
    f, exact = ODES[name]
    attempts = {}
    for rtol in RTOLS:
        ref, ref_att = _numpy_adaptive_heun(f, Y0, GRID, rtol, ATOL)
        ex = np.array([[exact(y, t) for y in Y0] for t in GRID])
        twin_worst = (np.abs(ref - ex) / (ATOL + rtol * np.abs(ex))).max()
        out, log, calls, worst = _solve("adaptive_heun", name, dtype, rtol)
        print(f"\nadaptive_heun {name} {dtype} rtol {rtol:g}: {len(log)} attempts, {sum(1 for a in log if not a[3])} rejected, error / "
              f"(atol + rtol |y|) {worst:.3f}; the numpy twin's {twin_worst:.3f} in {len(ref_att)} attempts")
        if dtype == torch.float64:                                         # the same attempt sequence, the same states
            assert [a[3] for a in log] == [a[2] for a in ref_att]
            assert all(abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12 * b[1] for a, b in zip(log, ref_att))
            assert np.abs(out.numpy() - ref).max() < 1e-12
        assert worst <= 2 * twin_worst                                     # at most twice the twin's worst error over allowance
        assert calls == 2 + 2 * len(log)                                   # k1, the probe, two per attempt
        attempts[rtol] = len(log)
    assert attempts[1e-5] > attempts[1e-3]


# ---------------------------------------------------------------------------------------------- 5. replays, errors, names
@pytest.mark.parametrize("method", PAIRS)
def test_forced_attempts_replay_a_run(method):
    from visualcloze_amd import transport as T
    f = lambda t, y: -2 * t * y + math.sin(t)  # noqa: E731
    y0 = torch.tensor([1.0, -0.5, 2.25], dtype=torch.float32)
    grid = [0.0, 0.4, 1.1, 2.0]
    log = []
    out = T.rk_integrate(f, y0, grid, method, rtol=1e-4, atol=1e-7, log=log)
    assert any(not a[3] for a in log)
    for forced in ([a[1] for a in log], [(a[1], a[3]) for a in log]):
        log2 = []
        again = T.rk_integrate(f, y0, grid, method, rtol=1e-4, atol=1e-7, forced_dts=forced, log=log2)
        assert torch.equal(again, out) and log2 == log
    # every logged dt is the controller's answer to the attempt before it
    order = T.RK_TABLEAUS[method]["order"]
    for a, b in zip(log, log[1:]):
        assert T.rk_controller(a[1], a[2], order) == (a[3], b[1])


@pytest.mark.parametrize("method", PAIRS)
def test_error_cases(method):
    from visualcloze_amd.transport import Dopri5Error, rk_integrate
    y0 = torch.tensor([1.0], dtype=torch.float64)
    with pytest.raises(Dopri5Error, match="NaN"):
        rk_integrate(lambda t, y: y * float("nan") if t > 0.5 else -y, y0, [0.0, 1.0], method, forced_dts=[0.9])
    with pytest.raises(Dopri5Error, match="max_attempts"):
        rk_integrate(lambda t, y: -50 * y, y0, [0.0, 1.0], method, rtol=1e-8, atol=1e-10, max_attempts=3)
    with pytest.raises(Dopri5Error, match="underflowed"):
        rk_integrate(lambda t, y: -y, y0, [1e20, 2e20], method, forced_dts=[1.0])
    with pytest.raises(ValueError, match="increasing"):
        rk_integrate(lambda t, y: -y, y0, [0.0, 0.0], method)
    with pytest.raises(TypeError):
        rk_integrate(lambda t, y: -y, y0.to(torch.bfloat16), [0.0, 1.0], method)


def test_names():
    from visualcloze_amd import transport as T
    s = _sampler()
    for name in PAIRS:
        with pytest.raises(NotImplementedError):
            s.sample_ode(sampling_method=name)                             # the fixed-grid entry point keeps refusing them
    with pytest.raises(ValueError, match=r"dopri5.*bosh3.*adaptive_heun"):
        s.sample_ode_adaptive(method="fehlberg2")
    with pytest.raises(ValueError, match="dopri5_integrate"):
        T.rk_integrate(lambda t, y: -y, torch.ones(1), [0.0, 1.0], "dopri5")   # one route to Dormand-Prince
    with pytest.raises(ValueError):
        T.rk_integrate(lambda t, y: -y, torch.ones(1), [0.0, 1.0], "heun3")
    assert T.ADAPTIVE_METHODS == ("dopri5", "bosh3", "adaptive_heun")


@pytest.mark.parametrize("method", PAIRS)
def test_sample_ode_adaptive_integrates_a_foreign_callable(method):
    s = _sampler()
    y0 = torch.linspace(0.5, 2.0, 16, dtype=torch.float64).reshape(1, 8, 2)
    stages = {"bosh3": 4, "adaptive_heun": 3}[method]

    def model(y, timesteps, **kw):                                         # y' = -(1 + t) y through the sampler's drift f = -model(y, 1 - t)
        t = (1 - timesteps.double())[:, None, None]
        return (1 + t) * y
    rtol, atol = 1e-4, 1e-9
    fn = s.sample_ode_adaptive(method=method, num_steps=5, rtol=rtol, atol=atol, do_shift=False, time_shifting_factor=None,
                               return_trajectory=True)
    out = fn(y0, model, {})
    assert out.dtype == torch.float64 and out.shape == (5, 1, 8, 2) and torch.equal(out[0], y0)
    for i, t in enumerate((0.25, 0.5, 0.75, 1.0)):
        ex = y0 * math.exp(-(t + t * t / 2))
        # the model sees 1 - f32(t): ~1e-7 of perturbation in t on top of the tolerance's allowance
        assert ((out[i + 1] - ex).abs() <= 10 * (atol + rtol * ex.abs()) + 1e-6 * ex.abs()).all(), t
    (log,) = s.last_adaptive_log
    assert log["evaluations"] == 2 + (stages - 1) * len(log["attempts"]) and log["rejected"] == sum(1 for a in log["attempts"] if not a[3])
    last = s.sample_ode_adaptive(method=method, num_steps=5, rtol=rtol, atol=atol, do_shift=False, time_shifting_factor=None)(y0, model, {})
    assert last.shape == (1, 1, 8, 2) and torch.equal(last[0], out[-1])
    # the default is Dormand-Prince, as before
    s.sample_ode_adaptive(num_steps=5, rtol=rtol, atol=atol, do_shift=False, time_shifting_factor=None)(y0, model, {})
    (log,) = s.last_adaptive_log
    assert log["evaluations"] == 2 + 6 * len(log["attempts"])
