"""-m gpu: the fixed-grid "midpoint" and "rk4" solvers in the fused sampling loop.

  * vc_ode_stage alone - and vc_euler_step / vc_euler_step_f32, the same kernel - against the literal torch expressions
    (transport.STEP_RULES), bit for bit;
  * the fused loop (vc_flux_sample_ode: graph replays, device-side evaluation counter) == host-driven stepping through Flux.forward
    with those expressions, bit for bit, whole trajectories;
  * against the reference's own runs (tests/golden/solver_golden.npz).  Bound: 4 x floor_<method>, the reference's own bf16-vs-fp32
    distance as recorded by the generator (the standing rule of tests/test_model_gpu.py) - CAPPED at 6e-2, the loosest bound any
    trajectory test of this suite uses, because on the tiny procedural model the recorded floors (2.05e-1: four steps of a model
    whose single evaluation already moves by 5e-2 with the bf16 guidance and times) would make 4 x floor meaningless;
  * piecewise stepping, argument errors, and no leakage between methods on one handle.
The step functions are unpinned against real torchdiffeq (tests/golden/make_solver_golden.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METHODS = ("midpoint", "rk4")
EVALS = {"euler": 1, "midpoint": 2, "rk4": 4}
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 6e-2


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def sg():
    return np.load(os.path.join(REPO, "tests", "golden", "solver_golden.npz"))


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()


def _kw(inp, guidance_dtype=torch.float32):
    return dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                cond=inp["cond"].to(DEV, torch.bfloat16), guidance=inp["guidance"].to(DEV, guidance_dtype))


def _fn(method, **over):
    from visualcloze_amd.transport import Sampler, create_transport
    opts = dict(sampling_method=method, num_steps=5, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    opts.update(over)
    return Sampler(create_transport()).sample_ode(**opts)


def _eager(m):
    """a foreign callable: host-driven stepping, one Flux.forward per stage + the torch expressions.  Under autocast the reference
    model's output is bf16 whatever the dtype of its input (visualcloze.py:363), hence the cast."""
    return lambda x, **k: m.forward(x, **k).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- 1. the op alone
@pytest.mark.parametrize("dt", [0.0371234, -0.21347, 0.25])          # inexact in bf16, negative, exact
@pytest.mark.parametrize("n", [8 * 1024, 24 * 64, 1003, 7])          # multiples of 8 and not
@pytest.mark.parametrize("state", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("method", METHODS)
def test_ode_stage_equals_the_torch_expressions_bitwise(method, state, n, dt):
    from visualcloze_amd import hip
    from visualcloze_amd.transport import STEP_RULES
    E = EVALS[method]
    g = torch.Generator().manual_seed(n + E)
    y0 = (torch.randn(n, generator=g) * 2).to(DEV, state)
    vs = [torch.randn(n, generator=g).to(DEV, torch.bfloat16) for _ in range(E)]
    step = 2                                                          # dt sits at index 2 of the table: the device picks it
    dts = torch.tensor([9.0, -7.0, dt, 5.0], dtype=torch.float32, device=DEV)
    t0 = torch.tensor(0.25, device=DEV)
    dt_t = dts[step]
    # the literal rule; its drift hands back -v_j and records the state each stage is evaluated at
    ins, it = [], iter(vs)
    y1 = STEP_RULES[method](lambda t, y: (ins.append(y), -next(it))[1], t0, t0 + dt_t, dt_t, y0)
    assert y1.dtype == state and all(i.dtype == state for i in ins)
    want_in = [i.to(torch.bfloat16) for i in ins[1:]] + [y1.to(torch.bfloat16)]     # what img_in reads before evaluation j + 1
    y = y0.clone()
    k = torch.zeros(3, n, dtype=torch.bfloat16, device=DEV) if method == "rk4" else None
    y_in = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for j in range(E):
        counter.fill_(step * E + j)
        if j % 2:
            hip.ode_stage(method, -1, y, vs[j], k, y_in, dts, counter)          # stage from the device-side evaluation counter
        else:
            hip.ode_stage(method, j, y, vs[j], k, y_in, dts, counter)           # explicit stage
        torch.cuda.synchronize()
        bad = (y_in.view(torch.int16) != want_in[j].view(torch.int16)).float().mean().item()
        assert bad == 0.0, f"{method} stage {j}: {bad:.4f} of the next-evaluation inputs differ"
        if j < E - 1:
            assert torch.equal(y, y0), f"{method} stage {j} touched the state"
            if k is not None:
                assert torch.equal(k[j], -vs[j])
    assert torch.equal(y, y1), f"{method}: {(y != y1).float().mean().item():.4f} of the states differ"


# vc_euler_step / vc_euler_step_f32 run the same kernel as the Euler method: the literal rule again.  n = 1024 takes the 16-byte
# path; n = 1027, and a state that starts one element into its allocation (an unaligned base), the element path.  The device
# counter stands at 2 of a 3-entry dt table (Euler: one evaluation per step, dt = dts[counter]); without one, dt = dts[0].
@pytest.mark.parametrize("counter", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1024, 1027])
@pytest.mark.parametrize("state", ["bf16", "f32", "f32_shadow_only"])
def test_euler_step_equals_the_torch_expression_bitwise(state, n, offset, counter):
    from visualcloze_amd import hip
    from visualcloze_amd.transport import STEP_RULES
    dtype = torch.bfloat16 if state == "bf16" else torch.float32
    g = torch.Generator().manual_seed(n + offset)
    y0 = (torch.randn(n, generator=g) * 2).to(DEV, dtype)
    v = torch.randn(n, generator=g).to(DEV, torch.bfloat16)
    dts = torch.tensor([0.0371234, 9.0, -0.21347], dtype=torch.float32, device=DEV)
    step = torch.tensor([2], dtype=torch.int32, device=DEV) if counter else None
    dt_t = dts[2 if counter else 0]
    y1 = y0 if state == "f32_shadow_only" else STEP_RULES["euler"](lambda t, y: -v, None, None, dt_t, y0)
    assert y1.dtype == dtype
    buf = torch.zeros(n + 8, dtype=dtype, device=DEV)                 # the state is a view; the elements around it stay zero
    y = buf[offset:offset + n]
    y.copy_(y0)
    if state == "bf16":
        hip.euler_step(y, v, dts, step)
    else:
        shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        hip.euler_step_f32(y, shadow, None if state == "f32_shadow_only" else v, dts, step)      # v None: shadow = bf16(x32) only
    torch.cuda.synchronize()
    assert torch.equal(y, y1), f"{(y != y1).float().mean().item():.4f} of the states differ"
    assert not buf[:offset].any() and not buf[offset + n:].any()
    if state != "bf16":
        assert torch.equal(shadow, y1.to(torch.bfloat16))             # what img_in reads next


def test_ode_stage_argument_errors():
    from visualcloze_amd import hip
    y = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    v, y_in, dts = torch.zeros_like(y), torch.zeros_like(y), torch.zeros(1, device=DEV)
    with pytest.raises(hip.VclozeHipError, match="not VC_SOLVER_MIDPOINT"):
        hip.ode_stage(hip.SOLVER_EULER, 0, y, v, None, y_in, dts)
    with pytest.raises(hip.VclozeHipError):
        hip.ode_stage("midpoint", 2, y, v, None, y_in, dts)                  # stage out of range
    with pytest.raises(hip.VclozeHipError):
        hip.ode_stage("midpoint", -1, y, v, None, y_in, dts)                 # device-side stage needs the counter
    with pytest.raises(hip.VclozeHipError):
        hip.ode_stage("rk4", 0, y, v, None, y_in, dts)                       # rk4 needs k


# ---------------------------------------------------------------------------------------------- 2. fused == eager
@pytest.mark.parametrize("case", ["bf16", "f32", "b2_ragged", "guidance_bf16"])
@pytest.mark.parametrize("method", METHODS)
def test_fused_equals_eager_bitwise_tiny(model, method, case):
    from tests.procedural import tiny_inputs
    m, _ = model
    inp = tiny_inputs(B=2, seed=7) if case == "b2_ragged" else tiny_inputs(B=1)
    if case == "b2_ragged":
        inp["img_mask"][1, -12:] = 0
        inp["txt_mask"][0, -5:] = 0
    kw = _kw(inp, torch.bfloat16 if case == "guidance_bf16" else torch.float32)
    x = inp["x"].to(DEV, torch.float32 if case == "f32" else torch.bfloat16)
    x_before = x.clone()
    fn = _fn(method)
    fused = fn(x, m.forward, kw)
    eager = fn(x, _eager(m), kw)
    torch.cuda.synchronize()
    assert torch.equal(x, x_before) and "cond" in kw
    assert fused.dtype == x.dtype and fused.shape == eager.shape == (5,) + tuple(x.shape)
    for i in range(5):
        assert torch.equal(fused[i], eager[i]), f"state {i}: rel-L2 {rel_l2(fused[i], eager[i]):.3e}"
    if case == "f32":
        assert not torch.equal(fused[-1].to(torch.bfloat16).float(), fused[-1])     # stepped IN f32
    last = _fn(method, return_trajectory=False)(x, m.forward, kw)                  # and without the trajectory buffer
    assert last.shape[0] == 1 and torch.equal(last[-1], fused[-1])


@pytest.mark.parametrize("method", METHODS)
def test_fused_equals_eager_bitwise_full_width(method):
    """cfg 2 (512 text + 3456 image tokens), full width, 1 + 1 blocks, 3 intervals: the 2S / 4S-row modulation table and the
    256-row GEMM tiles."""
    from tests.test_fullsize_gpu import _build, _inputs
    m = _build(1, 1)
    inp = _inputs("cfg2", seed=3)
    kw = _kw(inp, torch.bfloat16)
    x = inp["x"].to(DEV, torch.bfloat16)
    fn = _fn(method, num_steps=4)
    fused = fn(x, m.forward, kw)
    eager = fn(x, _eager(m), kw)
    torch.cuda.synchronize()
    assert fused.shape == (4, 1, 3456, 64) and torch.isfinite(fused.float()).all()
    for i in range(4):
        assert torch.equal(fused[i], eager[i]), f"state {i}: rel-L2 {rel_l2(fused[i], eager[i]):.3e}"


# ---------------------------------------------------------------------------------------------- 3. the reference's own runs
@pytest.mark.parametrize("method", METHODS)
def test_fused_vs_the_reference_runs(model, sg, method):
    from tests.helpers import parity_log
    from tests.procedural import tiny_inputs
    m, _ = model
    inp = tiny_inputs(B=1)
    floor = float(sg[f"floor_{method}"])
    bound = min(4 * floor, CAP)
    fn = _fn(method)
    xb, x32 = inp["x"].to(DEV, torch.bfloat16), inp["x"].to(DEV, torch.float32)
    # fp32 reference run: f32 guidance; the reference's bf16 runs carry a bf16 guidance tensor (visualcloze.py:413)
    runs = {"fp32": (fn(xb, m.forward, _kw(inp)), sg[f"traj_{method}_states"]),
            "bf16": (fn(xb, m.forward, _kw(inp, torch.bfloat16)), sg[f"traj_{method}_bf16_states"]),
            "f32state": (fn(x32, m.forward, _kw(inp, torch.bfloat16)), sg[f"traj_{method}_f32state_states"])}
    worst = 0.0
    for name, (got, ref) in runs.items():
        assert tuple(got.shape) == ref.shape
        errs = [rel_l2(got[i], ref[i]) for i in range(1, ref.shape[0])]
        parity_log(f"[tiny, {method}] fused sampler vs the reference's {name} run, per step {['%.2e' % e for e in errs]} "
                   f"(bound {bound:.1e} = min(4 x floor {floor:.3e}, {CAP:.0e}))")
        worst = max(worst, max(errs))
    assert worst < bound


# ---------------------------------------------------------------------------------------------- 4. piecewise, errors
@pytest.mark.parametrize("method", METHODS)
def test_piecewise_steps_trajectory_and_table_bound(model, method):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import solver_time_grid
    m, _ = model
    inp = tiny_inputs(B=1)
    h = m.handle()
    kw = _kw(inp)
    S, E = 4, EVALS[method]
    t = solver_time_grid(S + 1, inp["x"].shape[1], 0.0, 1, True, 1)
    x0 = inp["x"].to(DEV, torch.bfloat16)
    eager = _fn(method)(x0, _eager(m), kw)                           # [S + 1, 1, N, C]
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S * E, stream=s)
        x1 = x0.clone()
        traj = torch.empty((S,) + tuple(x1.shape), dtype=torch.bfloat16, device=DEV)
        h.sample_ode(method, x1, kw["cond"], t, True, s, trajectory=traj)
        x2 = x0.clone()
        h.sample_begin(x2, kw["cond"], t, True, s, method=method)
        h.sample_steps(1, s)
        mid = torch.empty_like(x2)
        h.sample_end(mid, s)
        h.sample_steps(S - 1, s)
        out = torch.empty_like(x2)
        h.sample_end(out, s)
    torch.cuda.synchronize()
    assert torch.equal(out, x1) and torch.equal(traj[-1], x1) and torch.equal(mid, traj[0])
    assert torch.equal(x2, x0)                                        # begin / steps never write the caller's x
    for i in range(S):
        assert torch.equal(traj[i], eager[i + 1]), f"trajectory[{i}] is not the state after step {i}"
    with pytest.raises(hip.VclozeHipError, match="more steps"):
        h.sample_steps(1, st.cuda_stream)
    # S * E evaluations must fit the prepared tables: refused before the device is touched
    with torch.cuda.stream(st):
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S * E - 1, stream=st.cuda_stream)
        with pytest.raises(hip.VclozeHipError, match="evaluations"):
            h.sample_ode(method, x0.clone(), kw["cond"], t, True, st.cuda_stream)
        with pytest.raises(hip.VclozeHipError, match="unknown solver method"):
            h.sample_ode(7, x0.clone(), kw["cond"], t, True, st.cuda_stream)
        h.sample_ode("euler", x0.clone(), kw["cond"], t, True, st.cuda_stream)       # S <= S * E - 1 evaluations: Euler fits
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. no leakage between methods
def test_methods_alternate_on_one_handle_without_leakage(model):
    from tests.helpers import tiny_model
    from tests.procedural import tiny_inputs
    m, _ = model
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.bfloat16)
    e1 = _fn("euler")(x, m.forward, kw)
    r1 = _fn("rk4")(x, m.forward, kw)
    e2 = _fn("euler")(x, m.forward, kw)
    r2 = _fn("rk4")(x, m.forward, kw)
    m1 = _fn("midpoint")(x, m.forward, kw)
    e3 = _fn("euler")(x, m.forward, kw)
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and torch.equal(e1, e3) and torch.equal(r1, r2)
    assert not torch.equal(e1[-1], r1[-1]) and not torch.equal(m1[-1], r1[-1])
    fresh, _ = tiny_model()
    assert torch.equal(_fn("euler")(x, fresh.forward, kw), e1)        # ... and to a handle that never ran another method
    assert torch.equal(_fn("rk4")(x, fresh.forward, kw), r1)
    # the captured step is kept per (geometry, method): with three methods and a second geometry on one handle - four entries,
    # what the handle keeps - every repeat above replays its own graph; the results stay bit-identical after a fifth entry
    # evicted the oldest
    inp2 = tiny_inputs(B=2, seed=7)
    x2 = inp2["x"].to(DEV, torch.bfloat16)
    a = _fn("midpoint")(x2, m.forward, _kw(inp2))
    b = _fn("rk4")(x2, m.forward, _kw(inp2))
    assert torch.equal(_fn("euler")(x, m.forward, kw), e1) and torch.equal(_fn("rk4")(x, m.forward, kw), r1)
    assert torch.equal(_fn("midpoint")(x2, m.forward, _kw(inp2)), a) and torch.equal(_fn("rk4")(x2, m.forward, _kw(inp2)), b)


def test_every_sampler_in_turn_on_one_handle_equals_a_fresh_handle(model):
    """One handle, one stream, one workspace (options adaptive and sde on, max_steps 16): Euler, Dormand-Prince, rk4, SDE-Heun, Euler
    with true CFG, a REFUSED sample_sde, a REFUSED sample_dopri5, midpoint, Euler.  A trajectory latches its solver once where it
    begins (csrc/flux_sample.hip begin_trajectory): every successful result, and the captured step's node counts after every
    fixed-grid run, are those of a handle over the same weights that ran nothing else; the last Euler is the first."""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import solver_time_grid
    m, _ = model
    inp = tiny_inputs(B=2)
    kw = _kw(inp)
    x0 = inp["x"].to(DEV, torch.bfloat16)
    assert (x0.shape[0], kw["txt"].shape[1], x0.shape[1]) == (2, 16, 24)
    t = solver_time_grid(5, 24, 0, 1, True, None)                         # 4 steps: 16 evaluations of rk4
    t_sde = torch.linspace(0, 0.75, 4)                                    # Heun: 7 evaluations
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    kept = []

    def new_handle(s):
        m._handle = None                                                   # m.handle() builds another one over the same prepared weights
        h = m.handle()
        kept.append(h)
        h.set_adaptive(True)
        h.set_sde(True)
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 16, stream=s)
        return h

    def run(h, mode, s):
        x = x0.clone()
        if mode == "dopri5":
            h.sample_dopri5(x, kw["cond"], t, True, s, rtol=1e-2, atol=1e-3, max_attempts=200)
        elif mode == "sde_heun":
            h.sample_sde("Heun", x, kw["cond"], t_sde, True, s, form="sigma", norm=0.7, last_step="Mean", last_step_size=0.25, seed=3)
        elif mode == "cfg":
            h.set_cfg(2.5)
            h.sample_ode("euler", x, kw["cond"], t, True, s)
            h.set_cfg(None)
        else:
            h.sample_ode(mode, x, kw["cond"], t, True, s)
        return x, (None if mode in ("dopri5", "sde_heun") else h.step_nodes())

    try:
        with torch.cuda.stream(st):
            s = st.cuda_stream
            one = new_handle(s)
            got = {}
            for i, mode in enumerate(("euler", "dopri5", "rk4", "sde_heun", "cfg", "refused_sde", "refused_dopri5", "midpoint", "euler")):
                if mode == "refused_sde":
                    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*evaluations"):   # 19 evaluations, 16 prepared
                        one.sample_sde("Heun", x0.clone(), kw["cond"], torch.linspace(0, 0.75, 10), True, s, form="sigma", norm=0.7,
                                       last_step="Mean", last_step_size=0.25, seed=3)
                elif mode == "refused_dopri5":
                    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*increase strictly"):
                        one.sample_dopri5(x0.clone(), kw["cond"], torch.tensor([0.0, 0.5, 0.5, 1.0]), True, s)
                else:
                    got[i, mode] = run(one, mode, s)
            want = {mode: run(new_handle(s), mode, s) for mode in ("euler", "dopri5", "rk4", "sde_heun", "cfg", "midpoint")}
        torch.cuda.synchronize()
    finally:
        m._handle = None                                                   # the module's model builds its own handle again
    for (i, mode), (x, nodes) in got.items():
        assert torch.isfinite(x.float()).all() and not torch.equal(x, x0), mode
        assert torch.equal(x, want[mode][0]), (i, mode)
        assert nodes == want[mode][1], (i, mode, nodes, want[mode][1])
    assert torch.equal(got[8, "euler"][0], got[0, "euler"][0])
    finals = [want[mode][0] for mode in ("euler", "dopri5", "rk4", "sde_heun", "cfg", "midpoint")]
    assert all(not torch.equal(a, b) for i, a in enumerate(finals) for b in finals[i + 1:])       # six different samplers


def test_every_sampler_method_in_turn_on_one_model_leaves_the_handle_as_it_found_it(model):
    """The same at the Sampler level, where every method sets the handle's options and takes them back: Euler, adaptive bosh3, SDE-Heun,
    multistep of order 3, rk4 with true CFG, an adaptive solve that FAILS inside the fused loop (max_attempts = 1), Euler.  After every
    call, the failed one too, the workspace options and true CFG are off; every successful result is bit-equal to the same call on a
    model whose handle ran nothing else; the last Euler is the first."""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.pipeline import NoiseStream
    from visualcloze_amd.transport import Sampler, create_transport
    m, _ = model
    inp = tiny_inputs(B=2)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.bfloat16)
    assert (x.shape[0], kw["txt"].shape[1], x.shape[1]) == (2, 16, 24)
    S = Sampler(create_transport())
    grid = dict(num_steps=5, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    calls = {
        "euler": lambda: S.sample_ode(sampling_method="euler", **grid)(x, m.forward, kw),
        "bosh3": lambda: S.sample_ode_adaptive(method="bosh3", rtol=1e-2, atol=1e-3, **grid)(x, m.forward, kw),
        "sde_heun": lambda: S.sample_sde(sampling_method="Heun", diffusion_form="sigma", diffusion_norm=0.7, last_step="Mean", last_step_size=0.25,
                                         num_steps=4, sample_eps=1e-3, rng=NoiseStream(3), return_trajectory=True)(x, m.forward, **kw),
        "multistep": lambda: S.sample_ode_multistep(order=3, **grid)(x, m.forward, kw),
        "cfg_rk4": lambda: S.sample_ode(sampling_method="rk4", **grid)(x, m.forward_with_cfg, dict(kw, cfg_scale=2.5)),
        "failing": lambda: S.sample_ode_adaptive(method="bosh3", rtol=1e-2, atol=1e-3, max_attempts=1, **grid)(x, m.forward, kw),
    }

    def all_off():
        h = m.handle()
        return {k: h.ws_options[k] for k in ("adaptive", "sde", "multistep")} == dict(adaptive=0, sde=0, multistep=0) and h._cfg is None

    kept = []                                                              # every handle lives until the device is idle
    try:
        m._handle = None
        got = []
        for name in ("euler", "bosh3", "sde_heun", "multistep", "cfg_rk4", "failing", "euler"):
            if name == "failing":
                with pytest.raises(hip.VclozeHipError, match="max_attempts = 1"):
                    calls[name]()
            else:
                got.append((name, calls[name]()))
            assert all_off(), name
        want = {}
        for name in ("euler", "bosh3", "sde_heun", "multistep", "cfg_rk4"):
            kept.append(m.handle())
            m._handle = None                                               # m.handle() builds another one over the same prepared weights
            want[name] = calls[name]()
        kept.append(m.handle())
        torch.cuda.synchronize()
    finally:
        m._handle = None                                                   # the module's model builds its own handle again
    for name, out in got:
        assert torch.isfinite(out.float()).all() and not torch.equal(out[-1], x), name
        assert torch.equal(out, want[name]), name
    assert torch.equal(got[-1][1], got[0][1])
    finals = [want[name][-1] for name in want]
    assert all(not torch.equal(a, b) for i, a in enumerate(finals) for b in finals[i + 1:])       # five different samplers


def test_pipeline_passes_the_solver_through(model):
    """generate_grid(..., solver=) reaches Sampler.sample_ode through denoise_grid: rk4 runs end to end and is not Euler."""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import pipeline
    m, _ = model
    inp = tiny_inputs(B=1)
    noise = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16) for _ in range(2)]
    lat = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16) for _ in range(2)]
    masks = [torch.ones(1, 1, 64, 192, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    outs = {}
    for solver in ("euler", "rk4"):
        rows = pipeline.denoise_grid(m, noise, lat, masks, inp["txt"].to(DEV, torch.bfloat16), inp["y"].to(DEV, torch.bfloat16),
                                     cfg=30.0, steps=3, solver=solver)
        outs[solver] = torch.cat([r.float().flatten() for r in rows])
        assert torch.isfinite(outs[solver]).all()
    assert not torch.equal(outs["euler"], outs["rk4"])
    with pytest.raises(NotImplementedError):
        pipeline.denoise_grid(m, noise, lat, masks, inp["txt"].to(DEV, torch.bfloat16), inp["y"].to(DEV, torch.bfloat16),
                              cfg=30.0, steps=3, solver="dopri5")
