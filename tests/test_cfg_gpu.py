"""-m gpu: true classifier-free guidance (Flux.forward_with_cfg, models/model.py:126-145) in the fused sampling loop.

  * vc_cfg_combine alone against the literal torch expression `u + s * (c - u)` on bf16 tensors, bit for bit;
  * Flux.forward_with_cfg == that expression over Flux.forward's bf16 output, bit for bit, and against the reference's own run
    (tests/golden/cfg_golden.npz) within TOL_GOLDEN x (1 + |s|): the bound tests/test_model_gpu.py holds the tiny `flux_b2` forward
    to, times the factor by which the combine can amplify a difference of the two halves;
  * the fused loop (vc_flux_set_cfg: one more node in the captured step, samples chunked by pairs) == host-driven stepping through
    forward_with_cfg, bit for bit, every state, and against the reference's own trajectories at the per-step bound of
    tests/test_solvers_gpu.py (min(4 x floor, 6e-2), floor = the reference's own bf16-vs-fp32 distance recorded by the generator);
  * piecewise stepping, the unconditional half against a plain trajectory, no leakage on one handle, argument errors, full width."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_GOLDEN = 3e-2          # tests/test_model_gpu.py
CAP = 6e-2                 # tests/test_solvers_gpu.py
METHODS = ("euler", "midpoint", "rk4")
EVALS = {"euler": 1, "midpoint": 2, "rk4": 4}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def cg():
    return np.load(os.path.join(REPO, "tests", "golden", "cfg_golden.npz"))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_cfg_golden", os.path.join(REPO, "tests", "golden", "make_cfg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()[0]


def _kw(inp, guidance_dtype=torch.float32, cfg_scale=None, rows=slice(None)):
    kw = dict(txt=inp["txt"][rows].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"][rows].to(DEV), txt_mask=inp["txt_mask"][rows].to(DEV),
              y=inp["y"][rows].to(DEV, torch.bfloat16), img_ids=inp["img_ids"][rows].to(DEV), img_mask=inp["img_mask"][rows].to(DEV),
              cond=inp["cond"][rows].to(DEV, torch.bfloat16), guidance=inp["guidance"][rows].to(DEV, guidance_dtype))
    if cfg_scale is not None:
        kw["cfg_scale"] = cfg_scale
    return kw


def _fn(method, **over):
    from visualcloze_amd.transport import Sampler, create_transport
    opts = dict(sampling_method=method, num_steps=4, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    opts.update(over)
    return Sampler(create_transport()).sample_ode(**opts)


def _eager(m):
    """a foreign callable (no __self__): host-driven stepping, one forward_with_cfg per evaluation + the torch expressions"""
    return lambda x, **k: m.forward_with_cfg(x, **k).to(torch.bfloat16)


def _eager_plain(m):
    return lambda x, **k: m.forward(x, **k).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- 1. the op alone
@pytest.mark.parametrize("scale", [1.0, 3.7, 0.0, -1.5])
@pytest.mark.parametrize("n", [8 * 1024, 24 * 64, 1003, 7])          # 1003, 7: the 16-byte path must not be taken
def test_cfg_combine_equals_the_torch_expression_bitwise(n, scale):
    from visualcloze_amd import hip
    g = torch.Generator().manual_seed(n)
    c = (torch.randn(n, generator=g) * 2).to(DEV, torch.bfloat16)
    u = (torch.randn(n, generator=g) * 2).to(DEV, torch.bfloat16)
    want = u + scale * (c - u)
    assert want.dtype == torch.bfloat16
    c0, u0 = c.clone(), u.clone()
    out = hip.cfg_combine(c, u, scale)                                # out of place
    torch.cuda.synchronize()
    assert torch.equal(out, want), f"{(out != want).float().mean().item():.4f} of the elements differ"
    assert torch.equal(c, c0) and torch.equal(u, u0)
    assert hip.cfg_combine(c, u, scale, out=c) is c                   # in place on cond
    torch.cuda.synchronize()
    assert torch.equal(c, want) and torch.equal(u, u0)
    hip.cfg_combine(c0, u, scale, out=u)                              # in place on uncond
    torch.cuda.synchronize()
    assert torch.equal(u, want)
    if scale == 1.0:
        assert not torch.equal(want, c0)                              # c - u is rounded: s = 1 is not the identity


def test_cfg_combine_with_unaligned_bases_and_argument_errors():
    from visualcloze_amd import hip
    n = 1024                                                          # a multiple of 8: only the bases keep it off the 16-byte path
    g = torch.Generator().manual_seed(5)
    bufs = [torch.zeros(n + 8, dtype=torch.bfloat16, device=DEV) for _ in range(3)]
    c, u, out = (b[1:1 + n] for b in bufs)
    c.copy_((torch.randn(n, generator=g) * 2).to(torch.bfloat16))
    u.copy_((torch.randn(n, generator=g) * 2).to(torch.bfloat16))
    hip.cfg_combine(c, u, 3.7, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, u + 3.7 * (c - u))
    assert not bufs[2][:1].any() and not bufs[2][1 + n:].any()        # the elements around the view stay zero
    with pytest.raises(hip.VclozeHipError, match="overlap"):
        hip.cfg_combine(bufs[0][0:n], u, 1.0, out=bufs[0][4:4 + n])
    with pytest.raises(hip.VclozeHipError, match="finite"):
        hip.cfg_combine(c, u, float("nan"), out=out)
    with pytest.raises(hip.VclozeHipError, match="same number"):
        hip.cfg_combine(c, u[:-1], 1.0)


# ---------------------------------------------------------------------------------------------- 2. forward_with_cfg
@pytest.mark.parametrize("B", [2, 4])
def test_forward_with_cfg_is_forward_plus_the_expression_and_tracks_the_reference(model, cg, gen, B):
    from tests.helpers import parity_log
    m = model
    inp, t, s = gen.cfg_inputs(B), torch.tensor(cg[f"fwd_b{B}_t"]).to(DEV), float(cg["cfg_scale"])
    h = B // 2
    img = torch.cat((inp["x"], inp["cond"]), -1)
    for in_dtype, gdt, ref, name in ((torch.bfloat16, torch.float32, cg[f"fwd_b{B}"], "fp32"),
                                     (torch.float32, torch.bfloat16, cg[f"fwd_b{B}_bf16"], "bf16")):
        kw = _kw(inp, gdt)
        kw.pop("cond")
        v = m.forward(img.to(DEV, torch.bfloat16), timesteps=t, **kw)                 # the kernels' bf16 output
        assert v.dtype == torch.bfloat16
        want = torch.cat([v[h:] + s * (v[:h] - v[h:]), v[h:]], dim=0)
        got = m.forward_with_cfg(img.to(DEV, in_dtype), timesteps=t, cfg_scale=s, **kw)
        torch.cuda.synchronize()
        assert got.dtype == in_dtype and got.shape == v.shape
        assert torch.equal(got, want.to(in_dtype)), f"{(got != want.to(in_dtype)).float().mean().item():.4f} of the elements differ"
        err = rel_l2(got, ref)
        bound = TOL_GOLDEN * (1 + abs(s))
        parity_log(f"[tiny, B={B}] forward_with_cfg (cfg_scale {s}) vs the reference's {name} run: rel-L2 {err:.3e} "
                   f"(bound {bound:.3e} = {TOL_GOLDEN:.0e} x (1 + |s|)); unconditional half alone {rel_l2(got[h:], ref[h:]):.3e}")
        assert err < bound
    kw1 = {k: v for k, v in _kw(inp, rows=slice(0, 1)).items() if k != "cond"}
    with pytest.raises(ValueError, match="odd batch"):                # the reference dies with an unpack error there
        m.forward_with_cfg(img[:1].to(DEV, torch.bfloat16), timesteps=t[:1], cfg_scale=s, **kw1)


# ---------------------------------------------------------------------------------------------- 3. fused == eager
def _inputs(gen, B):
    """cfg_inputs for any even B: text masks differ within every pair (the negative prompt is shorter); from B = 4 on the second pair
    is a shorter, padded grid.  B = 6 needs two chunks - pairs (0, 3), (1, 4), then (2, 5) - and the way back to the caller's order."""
    return gen.cfg_inputs(B)


@pytest.mark.parametrize("B", [2, 4, 6])
@pytest.mark.parametrize("state", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("method", METHODS)
def test_fused_equals_eager_bitwise(model, gen, monkeypatch, method, state, B):
    from visualcloze_amd import transport
    m = model
    inp = _inputs(gen, B)
    assert not torch.equal(inp["txt_mask"][0], inp["txt_mask"][B // 2])              # a pair with different text-mask lengths
    kw = _kw(inp, cfg_scale=3.5)
    x = inp["x"].to(DEV, state)
    x_before = x.clone()
    fused_calls = []
    real = transport._sample_fused
    monkeypatch.setattr(transport, "_sample_fused", lambda *a, **k: (fused_calls.append(k.get("cfg_scale")), real(*a, **k))[1])
    fn = _fn(method)
    fused = fn(x, m.forward_with_cfg, kw)
    eager = fn(x, _eager(m), kw)
    torch.cuda.synchronize()
    assert fused_calls == [3.5]                                        # the fused loop ran, once, with the scale
    assert torch.equal(x, x_before) and kw["cfg_scale"] == 3.5 and "cond" in kw
    assert fused.dtype == state and fused.shape == eager.shape == (4,) + tuple(x.shape)
    for i in range(4):
        assert torch.equal(fused[i], eager[i]), f"state {i}: rel-L2 {rel_l2(fused[i], eager[i]):.3e}"
    assert not torch.equal(fused[-1][:B // 2], fused[-1][B // 2:])     # the halves carry their own state
    last = _fn(method, return_trajectory=False)(x, m.forward_with_cfg, kw)
    assert last.shape[0] == 1 and torch.equal(last[-1], fused[-1])


def test_unequal_image_masks_in_a_pair_are_stepped_eagerly(model, gen, monkeypatch):
    from visualcloze_amd import transport
    m = model
    inp = gen.cfg_inputs(2)
    inp["img_mask"][1, -12:] = 0                                       # the unconditional sample alone is a shorter grid
    kw = _kw(inp, cfg_scale=3.5)
    x = inp["x"].to(DEV, torch.bfloat16)
    assert not transport._cfg_fusable(m, x, "euler", kw)
    want = transport._sample_foreign(_eager(m), x, dict(kw), transport.solver_time_grid(4, x.shape[1], 0, 1, True, 1), True, "euler")
    monkeypatch.setattr(transport, "_sample_fused", lambda *a, **k: pytest.fail("the fused loop must not run"))
    got = _fn("euler")(x, m.forward_with_cfg, kw)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # so are an f16 state and a model without the C handle
    x16 = inp["x"].to(DEV, torch.float16)
    kw_eq = _kw(gen.cfg_inputs(2), cfg_scale=3.5)
    assert not transport._cfg_fusable(m, x16, "euler", kw_eq) and transport._cfg_fusable(m, x, "euler", kw_eq)
    m.use_handle = False
    try:
        assert not transport._cfg_fusable(m, x, "euler", kw_eq)
        a = _fn("euler")(x, m.forward_with_cfg, kw_eq)
    finally:
        m.use_handle = True
    monkeypatch.undo()
    assert torch.equal(a, _fn("euler")(x, m.forward_with_cfg, kw_eq))  # and the Python-ordered plan's eager steps == the fused loop


@pytest.mark.parametrize("B", [2, 4])
def test_fused_vs_the_reference_runs(model, cg, gen, B):
    from tests.helpers import parity_log
    m = model
    inp = gen.cfg_inputs(B)
    s = float(cg["cfg_scale"])
    floor = float(cg[f"floor_b{B}"])
    bound = min(4 * floor, CAP)
    fn = _fn("euler")
    xb, x32 = inp["x"].to(DEV, torch.bfloat16), inp["x"].to(DEV, torch.float32)
    runs = {"fp32": (fn(xb, m.forward_with_cfg, _kw(inp, cfg_scale=s)), cg[f"traj_b{B}_states"]),
            "bf16": (fn(xb, m.forward_with_cfg, _kw(inp, torch.bfloat16, cfg_scale=s)), cg[f"traj_b{B}_bf16_states"])}
    if B == 2:
        runs["f32state"] = (fn(x32, m.forward_with_cfg, _kw(inp, torch.bfloat16, cfg_scale=s)), cg["traj_b2_f32state_states"])
    worst = 0.0
    for name, (got, ref) in runs.items():
        assert tuple(got.shape) == ref.shape
        errs = [rel_l2(got[i], ref[i]) for i in range(1, ref.shape[0])]
        parity_log(f"[tiny, euler, true CFG {s}, B={B}] fused sampler vs the reference's {name} run, per step {['%.2e' % e for e in errs]} "
                   f"(bound {bound:.1e} = min(4 x floor {floor:.3e}, {CAP:.0e}))")
        worst = max(worst, max(errs))
    assert worst < bound


# ---------------------------------------------------------------------------------------------- 4. piecewise
@pytest.mark.parametrize("method", METHODS)
def test_piecewise_steps_with_cfg_and_the_unconditional_half(model, gen, method):
    from visualcloze_amd.transport import solver_time_grid
    m = model
    inp = gen.cfg_inputs(2)
    h = m.handle()
    kw = _kw(inp)
    S, E = 3, EVALS[method]
    t = solver_time_grid(S + 1, inp["x"].shape[1], 0.0, 1, True, 1)
    x0 = inp["x"].to(DEV, torch.bfloat16)
    eager = _fn(method)(x0, _eager(m), dict(kw, cfg_scale=2.5))       # [S + 1, 2, N, C]
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(st):
            s = st.cuda_stream
            h.set_cfg(2.5)
            h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S * E, [40, 40], [(0, 0), (11, 16)],
                      stream=s)
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
    finally:
        h.set_cfg(None)
    torch.cuda.synchronize()
    assert torch.equal(out, x1) and torch.equal(traj[-1], x1) and torch.equal(mid, traj[0]) and torch.equal(x2, x0)
    for i in range(S):                                                # trajectory[i]: the state after step i, both halves
        assert torch.equal(traj[i], eager[i + 1]), f"trajectory[{i}] is not the state after step {i}"
    # the unconditional half is a plain trajectory of that sample alone: nothing of the conditional half leaks into it
    plain = _fn(method)(x0[1:], m.forward, _kw(inp, rows=slice(1, 2)))
    torch.cuda.synchronize()
    for i in range(S + 1):
        assert torch.equal(eager[i][1:], plain[i]), f"state {i}: rel-L2 {rel_l2(eager[i][1:], plain[i]):.3e}"
    assert not torch.equal(eager[-1][:1], _fn(method)(x0[:1], m.forward, _kw(inp, rows=slice(0, 1)))[-1])   # the conditional half IS guided


# ---------------------------------------------------------------------------------------------- 5. no leakage, errors
def test_no_leakage_on_one_handle_and_argument_errors(model, gen):
    from tests.helpers import tiny_model
    from visualcloze_amd import hip
    from visualcloze_amd.transport import StepCache, solver_time_grid
    m = model
    inp = gen.cfg_inputs(2)
    x = inp["x"].to(DEV, torch.bfloat16)
    fn = _fn("euler")
    a = fn(x, m.forward_with_cfg, _kw(inp, cfg_scale=2.0))
    b = fn(x, m.forward_with_cfg, _kw(inp, cfg_scale=3.5))
    p = fn(x, m.forward, _kw(inp))
    a2 = fn(x, m.forward_with_cfg, _kw(inp, cfg_scale=2.0))
    torch.cuda.synchronize()
    assert torch.equal(a, fn(x, _eager(m), _kw(inp, cfg_scale=2.0))) and torch.equal(b, fn(x, _eager(m), _kw(inp, cfg_scale=3.5)))
    assert torch.equal(p, fn(x, _eager_plain(m), _kw(inp))) and torch.equal(a, a2)
    assert not torch.equal(a[-1], b[-1]) and not torch.equal(a[-1], p[-1])
    assert m.handle()._cfg is None                                    # set back to off behind every CFG trajectory
    fresh = tiny_model()[0]
    assert torch.equal(fn(x, fresh.forward, _kw(inp)), p)             # a handle that never ran CFG gives the same bits
    # cfg_scale defaults to 1.0, which is not the plain trajectory (c - u is rounded) but is forward_with_cfg's default
    d = fn(x, m.forward_with_cfg, _kw(inp))
    assert torch.equal(d, fn(x, _eager(m), _kw(inp, cfg_scale=1.0)))
    # at the C level: odd B, or the step cache, with CFG on are refused at sample_begin
    h = m.handle()
    kw1, kw2 = _kw(inp, rows=slice(0, 1)), _kw(inp)
    t = solver_time_grid(4, x.shape[1], 0.0, 1, True, 1)
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(st):
            s = st.cuda_stream
            h.set_cfg(2.0)
            h.prepare(kw1["txt"], kw1["y"], kw1["guidance"], False, kw1["img_ids"], kw1["txt_ids"], 3, stream=s)
            with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*odd"):
                h.sample_begin(x[:1].clone(), kw1["cond"], t, True, s)
            h.set_step_cache(StepCache(0.1))
            h.prepare(kw2["txt"], kw2["y"], kw2["guidance"], False, kw2["img_ids"], kw2["txt_ids"], 3, stream=s)
            with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*step cache"):
                h.sample_begin(x.clone(), kw2["cond"], t, True, s)
            h.set_step_cache(None)
            h.set_cfg(float("inf"))
            h.prepare(kw2["txt"], kw2["y"], kw2["guidance"], False, kw2["img_ids"], kw2["txt_ids"], 3, stream=s)
            with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*finite"):
                h.sample_begin(x.clone(), kw2["cond"], t, True, s)
    finally:
        h.set_step_cache(None)
        h.set_cfg(None)
    torch.cuda.synchronize()
    assert torch.equal(fn(x, m.forward, _kw(inp)), p)                 # and the handle is a plain one again


# ---------------------------------------------------------------------------------------------- 6. full width
def test_fused_equals_eager_bitwise_full_width():
    """cfg 2 geometry (512 text + 3456 image tokens), full width (hidden 3072, 24 heads), 1 + 1 blocks, B = 2, euler, 2 steps."""
    from tests.test_fullsize_gpu import _build, _inputs as full_inputs
    m = _build(1, 1)
    c, u = full_inputs("cfg2", seed=3), full_inputs("cfg2", seed=4)
    inp = {k: torch.cat((c[k], u[k]), 0) for k in c}
    inp["x"][1], inp["cond"][1] = inp["x"][0], inp["cond"][0]
    inp["txt_mask"][1, -200:] = 0
    kw = _kw(inp, torch.bfloat16, cfg_scale=3.5)
    x = inp["x"].to(DEV, torch.bfloat16)
    fn = _fn("euler", num_steps=3)
    fused = fn(x, m.forward_with_cfg, kw)
    eager = fn(x, _eager(m), kw)
    torch.cuda.synchronize()
    assert fused.shape == (3, 2, 3456, 64) and torch.isfinite(fused.float()).all()
    for i in range(3):
        assert torch.equal(fused[i], eager[i]), f"state {i}: rel-L2 {rel_l2(fused[i], eager[i]):.3e}"
