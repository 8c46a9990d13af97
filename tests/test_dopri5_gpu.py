"""-m gpu: the adaptive Dormand-Prince 5(4) solve in the fused loop (vc_dopri5_*, vc_flux_sample_dopri5).

  * vc_dopri5_stage and vc_dopri5_interp against the torch f32 expressions of transport.py, bit for bit;
  * vc_dopri5_error_ratio against fp64 inside the budget of its f32 arithmetic (tests/budget.py), the same bits on a second run, and a
    huge element in the last partial block moves it;
  * replay parity: the fused solve's log replayed by transport.dopri5_integrate (forced_dts) through Flux.forward - every ratio inside
    the norm's budget, every decision and every next dt the controller formula of the logged ratio, every output bit-equal;
  * bf16 callers, trajectory shapes, true CFG, the option off, the refusals.
The controller is unpinned against real torchdiffeq (tests/test_dopri5_cpu.py pins the tableau and single steps to SciPy)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()


def _kw(inp, guidance_dtype=torch.float32):
    return dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                cond=inp["cond"].to(DEV, torch.bfloat16), guidance=inp["guidance"].to(DEV, guidance_dtype))


def _sampler():
    from visualcloze_amd.transport import Sampler, create_transport
    return Sampler(create_transport())


def _step_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    y0 = (torch.randn(n, generator=g) * 2).to(DEV)
    vs = [torch.randn(n, generator=g).to(DEV, torch.bfloat16) for _ in range(7)]
    return y0, vs


# ---------------------------------------------------------------------------------------------- 1. the stage combination
@pytest.mark.parametrize("dt", [0.0371234, 0.25])
@pytest.mark.parametrize("n", [7, 1003, 8 * 1024])
def test_stage_equals_the_torch_expressions_bitwise(n, dt):
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    y0, vs = _step_inputs(n, n)
    dt_dev = torch.tensor([dt], dtype=torch.float32, device=DEV)
    h = T._f32(dt)
    k = torch.zeros(7, n, dtype=torch.bfloat16, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    ks = []
    for s in range(7):
        y_stage = torch.full((n,), 7.0, device=DEV)
        y_in = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
        counter.fill_(s)
        if s % 2:
            hip.dopri5_stage(-1, y0, k, vs[s], dt_dev, counter, y_stage, y_in)       # stage from the device-side counter
        else:
            hip.dopri5_stage(s, y0, k, vs[s], dt_dev, None, y_stage, y_in)           # explicit stage
        torch.cuda.synchronize()
        ks.append((-vs[s]).float())
        assert torch.equal(k[s], -vs[s]) and not k[s + 1:].any(), f"stage {s}: k"
        if s == 6:                                                                   # k7 only: nothing else is written
            assert (y_stage == 7.0).all() and (y_in.float() == 7.0).all()
            break
        want = y0 + h * T._dopri5_combine(T.DOPRI5_A[s] if s < 5 else T.DOPRI5_B, ks)
        assert torch.equal(y_stage, want), f"stage {s}: {(y_stage != want).float().mean().item():.4f} of the states differ"
        assert torch.equal(y_in, want.to(torch.bfloat16)), f"stage {s}: y_in"
    # v None: k[stage] stays, the same state is formed (k1 of a step is the last step's k7); stage 7: the probe state y0 + dt k1
    y_stage = torch.empty(n, device=DEV)
    before = k.clone()
    hip.dopri5_stage(0, y0, k, None, dt_dev, None, y_stage, None)
    assert torch.equal(k, before) and torch.equal(y_stage, y0 + h * T._dopri5_combine(T.DOPRI5_A[0], ks))
    y_in = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    hip.dopri5_stage(7, y0, k, None, dt_dev, None, None, y_in)
    assert torch.equal(k, before) and torch.equal(y_in, (y0 + h * ks[0]).to(torch.bfloat16))
    with pytest.raises(hip.VclozeHipError, match="dopri5_stage"):
        hip.dopri5_stage(8, y0, k, None, dt_dev, None, y_stage, None)
    with pytest.raises(hip.VclozeHipError, match="dopri5_stage"):
        hip.dopri5_stage(-1, y0, k, vs[0], dt_dev, None, y_stage, None)              # the device-side stage needs the counter


# ---------------------------------------------------------------------------------------------- 2. the dense output
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [7, 1003, 8 * 1024])
def test_interp_equals_the_torch_expressions_bitwise(n, out_dtype):
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    y0, vs = _step_inputs(n, n + 1)
    dt = 0.0371234
    dt_dev = torch.tensor([dt], dtype=torch.float32, device=DEV)
    k = torch.stack([-v for v in vs]).contiguous()
    ks = [r.float() for r in k]
    y1 = y0 + T._f32(dt) * T._dopri5_combine(T.DOPRI5_B, ks)
    for theta in (0.0, 0.37, 1.0):
        got = hip.dopri5_interp(y0, y1, k, dt_dev, theta, dtype=out_dtype)
        want = T.dopri5_interp(y0, y1, ks, dt, theta).to(out_dtype)
        assert got.dtype == out_dtype and torch.equal(got, want), f"theta {theta}: {(got != want).float().mean().item():.4f} differ"
    assert torch.equal(hip.dopri5_interp(y0, y1, k, dt_dev, 0.0), y0)                # the ends themselves
    assert torch.equal(hip.dopri5_interp(y0, y1, k, dt_dev, 1.0), y1)
    assert not torch.equal(hip.dopri5_interp(y0, y1, k, dt_dev, 0.37), y0 + 0.37 * (y1 - y0))   # and no chord in between
    with pytest.raises(hip.VclozeHipError, match="theta"):
        hip.dopri5_interp(y0, y1, k, dt_dev, 1.5)


# ---------------------------------------------------------------------------------------------- 3. the norm
def _norm_chain(n):
    """longest chain of f32 additions of the two-pass reduction: a thread's own elements, then two 256-wide trees of 8 levels"""
    nblk = min((n + 255) // 256, 256)
    return -(-n // (nblk * 256)) + 16


def _ratio64(y0, y1, ks, dt32, rtol, atol):
    """(the fp64 value of the norm over the f32 / bf16 operands the kernel reads, the budget of the kernel's f32 arithmetic).
    Per element: 6 products and 5 additions of the e row (each half an ulp of the running |sum| <= sum |e_i k_i|), the product with
    dt, the three operations of the tolerance, the division, the square; then the additions of the reduction, each half an ulp of
    the running sum <= sum q^2; then the division by n and the square root."""
    from visualcloze_amd import transport as T
    d = torch.float64
    e = [float(torch.tensor(c, dtype=d).to(torch.float32)) for c in T.DOPRI5_E]
    rt, at = T._f32(rtol), T._f32(atol)
    terms = [c * k.to(d) for c, k in zip(e, ks) if c != 0.0]
    acc = sum(terms)
    mag = sum(t.abs() for t in terms)
    err = dt32 * acc
    tol = at + rt * torch.maximum(y0.to(d).abs(), y1.to(d).abs())
    q = err / tol
    d_err = abs(dt32) * 11 * EPS24 * mag + EPS24 * err.abs()
    d_q = d_err / tol + 4 * EPS24 * q.abs()
    d_q2 = 2 * q.abs() * d_q + d_q * d_q + EPS24 * q * q
    S = float((q * q).sum())
    d_S = float(d_q2.sum()) + _norm_chain(q.numel()) * EPS24 * S
    n = q.numel()
    ratio = math.sqrt(S / n)
    return ratio, (d_S / (2 * math.sqrt(S * n)) if S > 0 else math.sqrt(d_S / n)) + 2 * EPS24 * ratio


@pytest.mark.parametrize("n", [1, 7, 1003, 256 * 1024 + 5])
def test_error_ratio_within_its_f32_budget_and_reproducible(n):
    from tests.budget import assert_within_budget
    from visualcloze_amd import hip
    y0, vs = _step_inputs(n, n + 2)
    dt, rtol, atol = 0.0371234, 1e-3, 1e-6
    dt_dev = torch.tensor([dt], dtype=torch.float32, device=DEV)
    k = torch.stack([-v for v in vs]).contiguous()
    y1 = y0 + 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(5)).to(DEV)
    got = hip.dopri5_error_ratio(y0, y1, k, dt_dev, rtol, atol)
    again = hip.dopri5_error_ratio(y0, y1, k, dt_dev, rtol, atol)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))               # fixed order: the same bits
    ref, bud = _ratio64(y0.cpu(), y1.cpu(), [r.cpu() for r in k], float(dt_dev.cpu()[0]), rtol, atol)
    print(f"\nerror_ratio n={n}: {got.item():.9g} vs fp64 {ref:.9g}, |diff| {abs(got.item() - ref):.3e}, budget {bud:.3e}")
    assert_within_budget(got.cpu(), torch.tensor([ref], dtype=torch.float64), roundings=0, f32_terms=torch.tensor([bud]), what=f"n={n}")
    # one huge element at the very end - the last, partial block of a ragged n - must move the result: a dropped tail would not
    k2 = k.clone()
    k2[6, n - 1] = 3e6                                                               # (k7 alone: the e row sums to zero)
    moved = hip.dopri5_error_ratio(y0, y1, k2, dt_dev, rtol, atol)
    ref2, bud2 = _ratio64(y0.cpu(), y1.cpu(), [r.cpu() for r in k2], float(dt_dev.cpu()[0]), rtol, atol)
    assert ref2 > 2 * ref
    assert_within_budget(moved.cpu(), torch.tensor([ref2], dtype=torch.float64), roundings=0, f32_terms=torch.tensor([bud2]), what=f"tail n={n}")
    # the initial-step norms: rms(a / (atol + rtol |y0|)) of y0, k1, k2 - k1
    scale = atol + rtol * y0.double().abs()
    for mode, a in ((1, y0.double()), (2, k[0].double()), (3, k[1].double() - k[0].double())):
        want = float(((a / scale) ** 2).mean().sqrt())
        g = hip.dopri5_error_ratio(y0, None, None if mode == 1 else k, None, rtol, atol, mode=mode).item()
        assert abs(g - want) <= (8 + _norm_chain(n)) * EPS24 * want, (mode, g, want)
    with pytest.raises(hip.VclozeHipError, match="rtol"):
        hip.dopri5_error_ratio(y0, y1, k, dt_dev, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------- 4. replay parity
@pytest.mark.parametrize("case", ["b1", "b2_ragged"])
def test_replay_parity_tiny(model, case):
    from tests.helpers import parity_log
    from tests.procedural import tiny_inputs
    from visualcloze_amd import transport as T
    m, _ = model
    inp = tiny_inputs(B=2, seed=7) if case == "b2_ragged" else tiny_inputs(B=1)
    if case == "b2_ragged":
        inp["img_mask"][1, -12:] = 0
        inp["txt_mask"][0, -5:] = 0
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.float32)
    rtol, atol = 1e-2, 1e-6
    s = _sampler()
    fused = s.sample_ode_adaptive(num_steps=4, rtol=rtol, atol=atol, do_shift=True, time_shifting_factor=1, return_trajectory=True)(
        x, m.forward, kw)
    torch.cuda.synchronize()
    (log,) = s.last_adaptive_log
    att = log["attempts"]
    assert fused.dtype == torch.float32 and fused.shape == (4,) + tuple(x.shape) and torch.equal(fused[0], x)
    assert log["evaluations"] == 2 + 6 * len(att) and att[-1][3]
    parity_log(f"[tiny, dopri5, {case}, rtol {rtol:g}] fused adaptive solve: {len(att)} attempts, {log['evaluations']} evaluations, "
               f"{log['rejected']} rejected; dt {['%.3g' % a[1] for a in att]}, ratio {['%.3g' % a[2] for a in att]}")
    # every decision and every next dt is the controller formula of the LOGGED ratio, exactly, in double
    for a, b in zip(att, att[1:]):
        assert T.dopri5_controller(a[1], a[2]) == (a[3], b[1])
        assert b[0] == (a[0] + a[1] if a[3] else a[0])
    assert all(a[3] == (a[2] <= 1.0) for a in att)
    # the eager twin on the same attempt sequence, through Flux.forward
    t = T.solver_time_grid(4, x.shape[1], 0, 1, True, 1)
    worst = [0.0]

    def on_attempt(tc, dt, y0, y1, ks):
        i = on_attempt.i
        on_attempt.i += 1
        ref, bud = _ratio64(y0.cpu(), y1.cpu(), [k.cpu() for k in ks], T._f32(dt), rtol, atol)
        worst[0] = max(worst[0], abs(att[i][2] - ref) / bud)
        assert abs(att[i][2] - ref) <= bud, f"attempt {i}: fused ratio {att[i][2]!r} vs fp64 of the eager step {ref!r} (budget {bud:.3e})"
    on_attempt.i = 0
    fwd = lambda xin, **k: m.forward(xin, **k)  # noqa: E731  (a foreign callable: stepped eagerly)
    eager, elog = T._sample_adaptive_foreign(fwd, x, dict(kw), t, True, rtol, atol, 1000, bf16_out=True,
                                             forced_dts=[(a[1], a[3]) for a in att], on_attempt=on_attempt)
    torch.cuda.synchronize()
    assert on_attempt.i == len(att) and [a[:2] for a in elog["attempts"]] == [a[:2] for a in att]
    parity_log(f"[tiny, dopri5, {case}] fused ratios vs fp64 of the eager twin's steps: worst |diff| / budget {worst[0]:.3f}")
    for i in range(4):
        assert torch.equal(fused[i], eager[i]), f"output {i}: {(fused[i] != eager[i]).float().mean().item():.4f} of the elements differ"


# ---------------------------------------------------------------------------------------------- 5. other cases
def test_bf16_caller_trajectory_shapes_and_the_pipeline(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import pipeline
    m, _ = model
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    xb = inp["x"].to(DEV, torch.bfloat16)
    opts = dict(num_steps=4, rtol=1e-2, atol=1e-6, do_shift=True, time_shifting_factor=1)
    s = _sampler()
    t16 = s.sample_ode_adaptive(return_trajectory=True, **opts)(xb, m.forward, kw)
    t32 = s.sample_ode_adaptive(return_trajectory=True, **opts)(xb.float(), m.forward, kw)
    last = s.sample_ode_adaptive(**opts)(xb, m.forward, kw)
    torch.cuda.synchronize()
    assert t16.dtype == torch.bfloat16 and t16.shape == (4,) + tuple(xb.shape) and t32.dtype == torch.float32
    assert torch.equal(t16, t32.to(torch.bfloat16))                       # widened on entry, rounded once per output
    assert not torch.equal(t32[-1].to(torch.bfloat16).float(), t32[-1])   # ... and stepped IN f32
    assert last.shape == (1,) + tuple(xb.shape) and torch.equal(last[0], t16[-1])
    # the pipeline passes it through; the grid handle does not know it
    noise = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16) for _ in range(2)]
    lat = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16) for _ in range(2)]
    masks = [torch.ones(1, 1, 64, 192, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    txt, vec = inp["txt"].to(DEV, torch.bfloat16), inp["y"].to(DEV, torch.bfloat16)
    rows = pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=3, adaptive=dict(rtol=1e-2, atol=1e-6))
    euler = pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=3)
    assert all(torch.isfinite(r.float()).all() for r in rows) and not torch.equal(rows[0], euler[0])
    assert m.last_adaptive_log[0]["evaluations"] == 2 + 6 * len(m.last_adaptive_log[0]["attempts"])
    with pytest.raises(ValueError, match="use_grid_handle"):
        pipeline.generate_grid(m, None, None, None, [], [], None, None, 0, adaptive=dict(rtol=1e-2, atol=1e-6), use_grid_handle=True)
    with pytest.raises(NotImplementedError):
        pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=3, solver="dopri5")


def test_true_cfg_steps_both_halves(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import transport as T
    m, _ = model
    inp = tiny_inputs(B=2, seed=7)
    kw = dict(_kw(inp), cfg_scale=2.5)
    x = inp["x"].to(DEV, torch.float32)
    rtol, atol = 1e-2, 1e-6
    s = _sampler()
    fused = s.sample_ode_adaptive(num_steps=3, rtol=rtol, atol=atol, do_shift=True, time_shifting_factor=1, return_trajectory=True)(
        x, m.forward_with_cfg, kw)
    torch.cuda.synchronize()
    (log,) = s.last_adaptive_log
    att = log["attempts"]
    # the eager twin through Flux.forward_with_cfg on the same attempts: both halves advance, bit for bit
    t = T.solver_time_grid(3, x.shape[1], 0, 1, True, 1)
    kw2 = dict(_kw(inp))
    fwd = lambda xin, **k: m.forward_with_cfg(xin, cfg_scale=2.5, **k)  # noqa: E731
    eager, _ = T._sample_adaptive_foreign(fwd, x, kw2, t, True, rtol, atol, 1000, bf16_out=True, forced_dts=[(a[1], a[3]) for a in att])
    assert torch.equal(fused, eager)
    assert not torch.equal(fused[-1][0], x[0]) and not torch.equal(fused[-1][1], x[1])
    plain = s.sample_ode_adaptive(num_steps=3, rtol=rtol, atol=atol, do_shift=True, time_shifting_factor=1)(x, m.forward, _kw(inp))
    assert not torch.equal(plain[-1][0], fused[-1][0])                    # the combine reached the conditional half


def test_option_off_changes_nothing_and_the_refusals(model):
    from tests.helpers import tiny_model
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import StepCache, solver_time_grid
    m, _ = tiny_model()                                                   # a handle that never heard of the option
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.bfloat16)
    h = m.handle()
    L = hip.lib()
    B, T_, N = 1, kw["txt"].shape[1], x.shape[1]
    euler = lambda: _sampler().sample_ode(sampling_method="euler", num_steps=5, do_shift=True, time_shifting_factor=1,  # noqa: E731
                                          return_trajectory=True)(x, m.forward, kw)
    before = [L.vc_flux_workspace_bytes(h.h, B, T_, N, S) for S in (4, 7, 30)]
    e0 = euler()
    h.set_adaptive(True)
    on = [L.vc_flux_workspace_bytes(h.h, B, T_, N, S) for S in (4, 7, 30)]
    n = B * N * x.shape[2]
    assert all(o - b >= 7 * n * 2 + 2 * n * 4 for o, b in zip(on, before))     # k[7] bf16, y0 and y1 f32
    h.set_adaptive(False)
    assert [L.vc_flux_workspace_bytes(h.h, B, T_, N, S) for S in (4, 7, 30)] == before
    fn = _sampler().sample_ode_adaptive(num_steps=4, rtol=1e-2, atol=1e-6, do_shift=True, time_shifting_factor=1)
    a0 = fn(x, m.forward, kw)
    assert h.ws_options["adaptive"] == 0                                                # the sampler leaves the option off behind it
    assert [L.vc_flux_workspace_bytes(h.h, B, T_, N, S) for S in (4, 7, 30)] == before
    assert torch.equal(euler(), e0)                                       # the same Euler bits after an adaptive run on the handle
    # the refusals, on the handle directly
    t = solver_time_grid(4, N, 0, 1, True, 1)
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        prep = lambda S=7: h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S, stream=s)  # noqa: E731
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*adaptive"):                 # VC_ERR_STATE: the option is off
            h.sample_dopri5(x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        h.set_adaptive(True)
        h.set_step_cache(StepCache(0.1))
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*step cache"):               # VC_ERR_ARG
            h.sample_dopri5(x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        h.set_step_cache(None)
        prep(6)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*max_steps"):
            h.sample_dopri5(x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*max_attempts"):             # VC_ERR_STATE
            h.sample_dopri5(x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6, max_attempts=1)
        assert len(h.dopri5_log()["attempts"]) == 1
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\)"):
            h.sample_dopri5(x.clone(), kw["cond"], t, True, s, float("nan"), 1e-6)
        x1 = x.clone()                                                                     # ... and the handle is usable afterwards
        h.sample_dopri5(x1, kw["cond"], t, True, s, 1e-2, 1e-6)
        h.set_adaptive(False)
    torch.cuda.synchronize()
    assert torch.equal(x1[None], a0)
    assert torch.equal(euler(), e0)
