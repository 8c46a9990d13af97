"""-m gpu: the embedded Runge-Kutta pairs bosh3 and adaptive_heun in the fused loop (vc_rk_*, vc_flux_sample_rk).

  * vc_rk_stage and vc_rk_interp against the torch f32 expressions of transport.py (rk_step, rk_hermite), bit for bit, at sizes that
    take the 16-byte body, the scalar tail, more than 256 blocks x 256 threads and a base 2 bytes off alignment;
  * VC_RK_DOPRI5 against vc_dopri5_stage / vc_dopri5_error_ratio, bit for bit: the vc_dopri5_* entries are the same kernels under
    their own names (what pins Dormand-Prince itself are the stage and norm tests, which run every method);
  * vc_rk_error_ratio, Dormand-Prince included, against fp64 inside the budget of its f32 arithmetic, reproducible, moved by its
    last element - and bit-equal to transport.rk_error_ratio, which restates the kernel's summation order;
  * the fused solve against transport.rk_integrate through Flux.forward: every output bit and an identical log;
  * the refusals, the workspace bytes, and Dormand-Prince and Euler on the same handle before and after.
The controller is torchdiffeq's as recalled, unpinned against real torchdiffeq (tests/test_rk_embedded_cpu.py pins the tableaus and
single steps to SciPy and to the closed form)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS24 = 2.0 ** -24
SIZES = [1, 7, 255, 2051, 131077]
METHODS = ["dopri5", "bosh3", "adaptive_heun"]
PAIRS = ["bosh3", "adaptive_heun"]
# the fused solve's tolerances on the tiny procedural model, chosen (from the step sizes a run logs, not from its results) so that an
# attempt is rejected and an output time falls strictly inside a step; the test asserts both
SOLVE_TOL = {"bosh3": (1e-2, 1e-6), "adaptive_heun": (5e-2, 1e-6)}
SOLVE_OUTPUTS = 8


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()


def _kw(inp):
    return dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                cond=inp["cond"].to(DEV, torch.bfloat16), guidance=inp["guidance"].to(DEV, torch.float32))


def _sampler():
    from visualcloze_amd.transport import Sampler, create_transport
    return Sampler(create_transport())


def _stages(method):
    from visualcloze_amd import transport as T
    return len(T.RK_TABLEAUS[method]["c"])


def _buf(n, dtype, off, fill=None):
    """n elements on the device; off: the base sits `off` elements past a 256-byte aligned allocation (a bf16 base 2 bytes off
    16-byte alignment, an f32 base 4 bytes off)"""
    t = torch.empty(n + off, dtype=dtype, device=DEV)[off:]
    assert t.data_ptr() % 16 == (off * t.element_size()) % 16 and t.is_contiguous()
    return t if fill is None else t.fill_(fill)


def _inputs(n, seed, off, planes=7):
    g = torch.Generator().manual_seed(seed)
    y0 = _buf(n, torch.float32, off).copy_(torch.randn(n, generator=g) * 2)
    vs = [_buf(n, torch.bfloat16, off).copy_(torch.randn(n, generator=g)) for _ in range(planes)]
    return y0, vs


def _rows(method):
    """the row of the tableau behind stage s = 0..S-2: a2.., then b"""
    from visualcloze_amd import transport as T
    tab = T.RK_TABLEAUS[method]
    return list(tab["a"]) + [tab["b"]]


# ---------------------------------------------------------------------------------------------- 1. the stage combination
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", METHODS)
def test_stage_equals_the_torch_expressions_bitwise(method, n, off):
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    S, dt = _stages(method), 0.0371234
    y0, vs = _inputs(n, n + off, off, S)
    dt_dev = torch.tensor([dt], dtype=torch.float32, device=DEV)
    h = T._f32(dt)
    k = _buf(S * n, torch.bfloat16, off, 0.0).view(S, n)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    ks, rows = [], _rows(method)
    for s in range(S):
        y_stage, y_in = _buf(n, torch.float32, off, 7.0), _buf(n, torch.bfloat16, off, 7.0)
        counter.fill_(s)
        if s % 2:
            hip.rk_stage(method, -1, y0, k, vs[s], dt_dev, counter, y_stage, y_in)    # stage from the device-side counter
        else:
            hip.rk_stage(method, s, y0, k, vs[s], dt_dev, None, y_stage, y_in)        # explicit stage
        ks.append((-vs[s]).float())
        assert torch.equal(k[s], -vs[s]) and not k[s + 1:].any(), f"stage {s}: k"
        if s == S - 1:                                                                # the last stage stores k alone
            assert (y_stage == 7.0).all() and (y_in.float() == 7.0).all()
            break
        want = y0 + h * T._dopri5_combine(rows[s], ks)
        assert torch.equal(y_stage, want), f"stage {s}: {(y_stage != want).float().mean().item():.4f} of the states differ"
        assert torch.equal(y_in, want.to(torch.bfloat16)), f"stage {s}: y_in"
    # the torch expression above IS transport.rk_step's: the same states from the same evaluations
    it = iter(vs[1:])
    y1, ks2 = T.rk_step(lambda t, y: (-next(it)).float(), 0.0, dt, y0, ks[0], method)
    assert torch.equal(y1, y0 + h * T._dopri5_combine(rows[-1], ks)) and all(torch.equal(a, b) for a, b in zip(ks, ks2))
    # a counter outside the method's stages: nothing is written
    before = k.clone()
    for outside in [-1, 8, 1000] + list(range(S, 7)):
        y_stage, y_in = _buf(n, torch.float32, off, 7.0), _buf(n, torch.bfloat16, off, 7.0)
        counter.fill_(outside)
        hip.rk_stage(method, -1, y0, k, vs[0], dt_dev, counter, y_stage, y_in)
        assert torch.equal(k, before) and (y_stage == 7.0).all() and (y_in.float() == 7.0).all(), outside
    # v None: k[stage] stays and the same state is formed; stage 7: the probe state y0 + dt k1
    y_stage = _buf(n, torch.float32, off)
    hip.rk_stage(method, 0, y0, k, None, dt_dev, None, y_stage, None)
    assert torch.equal(k, before) and torch.equal(y_stage, y0 + h * T._dopri5_combine(rows[0], ks))
    y_in = _buf(n, torch.bfloat16, off)
    hip.rk_stage(method, 7, y0, k, None, dt_dev, None, None, y_in)
    assert torch.equal(k, before) and torch.equal(y_in, (y0 + h * ks[0]).to(torch.bfloat16))
    if n == 7 and not off:
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*rk_stage"):
            hip.rk_stage(method, S if S < 7 else 8, y0, k, None, dt_dev, None, y_stage, None)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*rk_stage"):
            hip.rk_stage(method, -1, y0, k, vs[0], dt_dev, None, y_stage, None)       # the device-side stage needs the counter
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*unknown method"):
            hip.rk_stage(3, 0, y0, k, vs[0], dt_dev, None, y_stage, None)


# ---------------------------------------------------------------------------------------------- 2. the vc_dopri5_* entries are aliases
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_dopri5_method_returns_the_bits_of_the_dopri5_kernels(n, off):
    from visualcloze_amd import hip
    y0, vs = _inputs(n, n + 3, off)
    dt_dev = torch.tensor([0.0371234], dtype=torch.float32, device=DEV)
    ka, kb = (_buf(7 * n, torch.bfloat16, off, 0.0).view(7, n) for _ in range(2))
    for s in range(8):                                                                # 0..6, and the probe
        v = None if s == 7 else vs[s]
        outs = []
        for fn, k in ((lambda *a: hip.rk_stage("dopri5", *a), ka), (hip.dopri5_stage, kb)):
            y_stage, y_in = _buf(n, torch.float32, off, 7.0), _buf(n, torch.bfloat16, off, 7.0)
            fn(s, y0, k, v, dt_dev, None, y_stage, y_in)
            outs.append((y_stage, y_in))
        assert torch.equal(ka, kb) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"stage {s}"
    y1 = y0 + 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(5)).to(DEV)
    for mode in range(4):
        args = (y0, y1 if mode == 0 else None, None if mode == 1 else ka, dt_dev if mode == 0 else None, 1e-3, 1e-6)
        a, b = hip.rk_error_ratio("dopri5", *args, mode=mode), hip.dopri5_error_ratio(*args, mode=mode)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and a.item() > 0, f"mode {mode}: {a.item()!r} vs {b.item()!r}"


# ---------------------------------------------------------------------------------------------- 3. the norm
def _norm_chain(n):
    """longest chain of f32 additions of the two-pass reduction: a thread's own elements, then two 256-wide trees of 8 levels"""
    nblk = min((n + 255) // 256, 256)
    return -(-n // (nblk * 256)) + 16


def _ratio64(method, y0, y1, ks, dt32, rtol, atol):
    """(the fp64 value of the norm over the f32 / bf16 operands the kernel reads, the budget of the kernel's f32 arithmetic): the
    derivation of tests/test_dopri5_gpu.py with the method's e row - per element at most 2 S - 1 roundings of the row (each half an
    ulp of the running |sum| <= sum |e_i k_i|), the product with dt, the three operations of the tolerance, the division, the
    square; then the additions of the reduction; then the division by n and the square root."""
    from visualcloze_amd import transport as T
    d = torch.float64
    e = [float(torch.tensor(c, dtype=d).to(torch.float32)) for c in T.RK_TABLEAUS[method]["e"]]
    rt, at = T._f32(rtol), T._f32(atol)
    terms = [c * k.to(d) for c, k in zip(e, ks) if c != 0.0]
    acc = sum(terms)
    mag = sum(t.abs() for t in terms)
    err = dt32 * acc
    tol = at + rt * torch.maximum(y0.to(d).abs(), y1.to(d).abs())
    q = err / tol
    d_err = abs(dt32) * (2 * len(terms) - 1) * EPS24 * mag + EPS24 * err.abs()
    d_q = d_err / tol + 4 * EPS24 * q.abs()
    d_q2 = 2 * q.abs() * d_q + d_q * d_q + EPS24 * q * q
    S = float((q * q).sum())
    d_S = float(d_q2.sum()) + _norm_chain(q.numel()) * EPS24 * S
    n = q.numel()
    ratio = math.sqrt(S / n)
    return ratio, (d_S / (2 * math.sqrt(S * n)) if S > 0 else math.sqrt(d_S / n)) + 2 * EPS24 * ratio


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", METHODS)
def test_error_ratio_within_its_f32_budget_reproducible_and_the_twins_bits(method, n, off):
    from tests.budget import assert_within_budget
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    S = _stages(method)
    y0, vs = _inputs(n, n + 2, off, S)
    dt, rtol, atol = 0.0371234, 1e-3, 1e-6
    dt_dev = torch.tensor([dt], dtype=torch.float32, device=DEV)
    k = _buf(S * n, torch.bfloat16, off).view(S, n).copy_(torch.stack([-v for v in vs]))
    y1 = _buf(n, torch.float32, off).copy_(y0 + 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(5)).to(DEV))
    got = hip.rk_error_ratio(method, y0, y1, k, dt_dev, rtol, atol)
    again = hip.rk_error_ratio(method, y0, y1, k, dt_dev, rtol, atol)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))               # fixed order: the same bits
    ks = [r.float() for r in k]
    ref, bud = _ratio64(method, y0.cpu(), y1.cpu(), [r.cpu() for r in k], float(dt_dev.cpu()[0]), rtol, atol)
    print(f"\nrk_error_ratio {method} n={n}: {got.item():.9g} vs fp64 {ref:.9g}, |diff| {abs(got.item() - ref):.3e}, budget {bud:.3e}")
    assert_within_budget(got.cpu(), torch.tensor([ref], dtype=torch.float64), roundings=0, f32_terms=torch.tensor([bud]), what=f"n={n}")
    assert got.item() == T.rk_error_ratio(y0, y1, ks, dt, rtol, atol, method)          # the twin sums in the kernel's order
    # one huge element at the very end - the last, partial block of a ragged n - must move the result: a dropped tail would not
    k2 = k.clone()
    k2[0, n - 1] = 3e6
    moved = hip.rk_error_ratio(method, y0, y1, k2, dt_dev, rtol, atol)
    ref2, bud2 = _ratio64(method, y0.cpu(), y1.cpu(), [r.cpu() for r in k2], float(dt_dev.cpu()[0]), rtol, atol)
    assert ref2 > 2 * ref
    assert_within_budget(moved.cpu(), torch.tensor([ref2], dtype=torch.float64), roundings=0, f32_terms=torch.tensor([bud2]), what=f"tail n={n}")
    # the initial-step norms: rms(a / (atol + rtol |y0|)) of y0, k1, k2 - k1
    scale = atol + rtol * y0.double().abs()
    scale32 = T._f32(atol) + T._f32(rtol) * y0.cpu().abs()
    for mode, a, a32 in ((1, y0.double(), y0.cpu()), (2, k[0].double(), ks[0].cpu()),
                         (3, k[1].double() - k[0].double(), ks[1].cpu() - ks[0].cpu())):
        want = float(((a / scale) ** 2).mean().sqrt())
        g = hip.rk_error_ratio(method, y0, None, None if mode == 1 else k, None, rtol, atol, mode=mode).item()
        assert abs(g - want) <= (8 + _norm_chain(n)) * EPS24 * want, (mode, g, want)
        assert g == T._rk_norm(a32, scale32), mode
    if n == 7 and not off:
        with pytest.raises(hip.VclozeHipError, match="rtol"):
            hip.rk_error_ratio(method, y0, y1, k, dt_dev, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------- 4. the dense output
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", PAIRS)
def test_interp_equals_the_torch_expression_bitwise(method, n, out_dtype, off):
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    S, dt = _stages(method), 0.0371234
    y0, vs = _inputs(n, n + 1, off, S)
    dt_dev = torch.tensor([dt], dtype=torch.float32, device=DEV)
    k = _buf(S * n, torch.bfloat16, off).view(S, n).copy_(torch.stack([-v for v in vs]))
    ks = [r.float() for r in k]
    y1 = _buf(n, torch.float32, off).copy_(y0 + T._f32(dt) * T._dopri5_combine(T.RK_TABLEAUS[method]["b"], ks))
    for theta in (0.0, 0.25, 0.5, 1.0):
        got = hip.rk_interp(method, y0, y1, k, dt_dev, theta, out=_buf(n, out_dtype, off))
        want = T.rk_hermite(y0, y1, ks, dt, theta).to(out_dtype)
        assert got.dtype == out_dtype and torch.equal(got, want), f"theta {theta}: {(got != want).float().mean().item():.4f} differ"
    assert torch.equal(hip.rk_interp(method, y0, y1, k, dt_dev, 0.0), y0)              # the ends themselves
    assert torch.equal(hip.rk_interp(method, y0, y1, k, dt_dev, 1.0), y1)
    if n > 1:
        assert not torch.equal(hip.rk_interp(method, y0, y1, k, dt_dev, 0.25), y0 + 0.25 * (y1 - y0))   # and no chord in between
    if n == 7 and not off:
        with pytest.raises(hip.VclozeHipError, match="theta"):
            hip.rk_interp(method, y0, y1, k, dt_dev, 1.5)
        k7 = torch.zeros(7, n, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*vc_dopri5_interp"):     # VC_ERR_ARG: one route to Dormand-Prince
            hip.rk_interp("dopri5", y0, y1, k7, dt_dev, 0.5)


# ---------------------------------------------------------------------------------------------- 5. the fused solve
CASES = {"f32_b1": (torch.float32, 1, False), "bf16_b1": (torch.bfloat16, 1, False), "f32_b2": (torch.float32, 2, False),
         "bf16_b2": (torch.bfloat16, 2, False), "f32_b2_cfg": (torch.float32, 2, True), "bf16_b2_cfg": (torch.bfloat16, 2, True)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("method", PAIRS)
def test_fused_solve_equals_the_eager_twin_bitwise(model, method, case):
    from tests.helpers import parity_log
    from tests.procedural import tiny_inputs
    from visualcloze_amd import transport as T
    m, _ = model
    dtype, B, cfg = CASES[case]
    inp = tiny_inputs(B=2, seed=7) if B == 2 else tiny_inputs(B=1)
    kw = _kw(inp)
    x = inp["x"].to(DEV, dtype)
    rtol, atol = SOLVE_TOL[method]
    S = _stages(method)
    s = _sampler()
    opts = dict(num_steps=SOLVE_OUTPUTS, rtol=rtol, atol=atol, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    call, kwf = (m.forward_with_cfg, dict(kw, cfg_scale=2.5)) if cfg else (m.forward, kw)
    fused = s.sample_ode_adaptive(method=method, **opts)(x, call, kwf)
    torch.cuda.synchronize()
    (log,) = s.last_adaptive_log
    att = log["attempts"]
    assert fused.dtype == dtype and fused.shape == (SOLVE_OUTPUTS,) + tuple(x.shape) and torch.equal(fused[0], x)
    assert log["evaluations"] == 2 + (S - 1) * len(att) and att[-1][3]
    parity_log(f"[tiny, {method}, {case}, rtol {rtol:g}] fused solve: {len(att)} attempts, {log['evaluations']} evaluations, "
               f"{log['rejected']} rejected; dt {['%.3g' % a[1] for a in att]}, ratio {['%.3g' % a[2] for a in att]}")
    # no empty case: an attempt was rejected, and an output time lies strictly inside an accepted step
    t = T.solver_time_grid(SOLVE_OUTPUTS, x.shape[1], 0, 1, True, 1)
    ts = [float(v) for v in t.to(torch.float32).tolist()]
    assert log["rejected"] >= 1
    assert any(a[3] and any(a[0] < v < a[0] + a[1] for v in ts[1:]) for a in att)
    # the eager twin with ITS OWN controller, through the same model's forward (a foreign callable: stepped eagerly)
    if cfg:
        fwd = lambda xin, **k: m.forward_with_cfg(xin, cfg_scale=2.5, **k)  # noqa: E731
    else:
        fwd = lambda xin, **k: m.forward(xin, **k)  # noqa: E731
    eager, elog = T._sample_adaptive_foreign(fwd, x, dict(kw), t, True, rtol, atol, 1000, bf16_out=True, method=method)
    torch.cuda.synchronize()
    assert elog["attempts"] == att, "the logs (t, dt, ratio, accepted) differ"
    assert elog["evaluations"] == log["evaluations"]
    for i in range(SOLVE_OUTPUTS):
        assert torch.equal(fused[i], eager[i]), f"output {i}: {(fused[i] != eager[i]).float().mean().item():.4f} of the elements differ"
    if cfg:
        assert not torch.equal(fused[-1][0], x[0]) and not torch.equal(fused[-1][1], x[1])      # both halves advance


def test_refusals_workspace_bytes_and_coexistence(model):
    from tests.helpers import tiny_model
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import solver_time_grid
    m, _ = tiny_model()
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.bfloat16)
    h, L = m.handle(), hip.lib()
    B, T_, N = 1, kw["txt"].shape[1], x.shape[1]
    t = solver_time_grid(4, N, 0, 1, True, 1)
    t6 = solver_time_grid(6, N, 0, 1, True, 1)
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        prep = lambda S=7: h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S, stream=s)  # noqa: E731
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*adaptive"):                 # VC_ERR_STATE: the option is off
            h.sample_rk("bosh3", x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        off_bytes = L.vc_flux_workspace_bytes(h.h, B, T_, N, 7)
        h.set_adaptive(True)
        on_bytes = L.vc_flux_workspace_bytes(h.h, B, T_, N, 7)
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*vc_flux_sample_dopri5"):    # VC_ERR_ARG: one route to Dormand-Prince
            h.sample_rk("dopri5", x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\)"):
            h.sample_rk("bosh3", x.clone(), kw["cond"], t, True, s, float("nan"), 1e-6)
        h.set_monitor(1, 8)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*monitor"):                  # VC_ERR_ARG
            h.sample_rk("bosh3", x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        h.set_monitor(0)
        prep(3)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*max_steps"):
            h.sample_rk("bosh3", x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6)
        xh = x.clone()
        h.sample_rk("adaptive_heun", xh, kw["cond"], t, True, s, 5e-2, 1e-6)               # three rows are enough for S = 3
        assert h.rk_log()["evaluations"] == 2 + 2 * len(h.rk_log()["attempts"])
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*max_attempts"):             # VC_ERR_STATE
            h.sample_rk("bosh3", x.clone(), kw["cond"], t, True, s, 1e-2, 1e-6, max_attempts=1)
        assert len(h.rk_log()["attempts"]) == 1
        # coexistence on ONE handle: dopri5, bosh3, dopri5 again, then a fixed-grid Euler trajectory
        d1, b1, d2, e1 = x.clone(), x.clone(), x.clone(), x.clone()
        h.sample_dopri5(d1, kw["cond"], t, True, s, 1e-2, 1e-6)
        h.sample_rk("bosh3", b1, kw["cond"], t, True, s, 1e-2, 1e-6)
        assert L.vc_flux_workspace_bytes(h.h, B, T_, N, 7) == on_bytes > off_bytes         # bosh3 ran in dopri5's workspace
        h.sample_dopri5(d2, kw["cond"], t, True, s, 1e-2, 1e-6)
        h.sample_ode("euler", e1, kw["cond"], t6, True, s)
        nodes = h.step_nodes()
        h.set_adaptive(False)
        assert L.vc_flux_workspace_bytes(h.h, B, T_, N, 7) == off_bytes
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(d1, d2) and not torch.equal(d1, b1) and not torch.equal(b1, x)
    # a fresh handle that never ran an adaptive solve: the same Euler bits from a step of the same nodes
    m2, _ = tiny_model()
    h2 = m2.handle()
    st2 = m2.engine().stream
    st2.wait_stream(torch.cuda.current_stream())
    e2 = x.clone()
    with torch.cuda.stream(st2):
        h2.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 7, stream=st2.cuda_stream)
        h2.sample_ode("euler", e2, kw["cond"], t6, True, st2.cuda_stream)
        nodes2 = h2.step_nodes()
    torch.cuda.current_stream().wait_stream(st2)
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and nodes == nodes2 and nodes[0] > 0
