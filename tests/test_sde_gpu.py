"""-m gpu: the stochastic (SDE) sampler in the fused loop (vc_sde_stage, vc_flux_sample_sde).

  * vc_sde_stage against the torch f32 expressions, bit for bit, the noise taken from hip.randn(F32) at the stated stream positions:
    every mode, the 16-byte path, its tail and the element-wise path, stream phases 0 and 3, a block counter that carries into its high
    word, the device-side counter, the grid-stride loop past the capped grid;
  * the fused sampler == the eager twin (transport.sde_integrate through Flux.forward with hip.randn draws), bit for bit: B = 1 and a
    ragged B = 2, Euler-Maruyama with Mean and Heun with Tweedie, f32 and bf16 callers, true CFG;
  * replays and seeds, the option off, the node count, the refusals, the pipeline's pass-through.
Image quality under any diffusion form and the throughput of the step are not measured here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15


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


# ---------------------------------------------------------------------------------------------- 1. the update kernel
ROW = (0.0371234, 1.2345678, 0.4567891, 0.6180339)          # h, A, Bc, g


def _f32s(vals):
    return [float(v) for v in np.asarray(vals, dtype=np.float32)]


def _expect(mode, e, n, offset, y, xhat, k1, v, coef):
    """the torch f32 expressions of one row -> the buffers afterwards (None: left as it was)"""
    from visualcloze_amd import hip
    h, A, Bc, g = coef
    d = {hip.SDE_EM: e, hip.SDE_HEUN2: (e + 1) // 2, hip.SDE_INJECT: 0}.get(mode)
    z = hip.randn((n,), SEED, offset + d * n, dtype=torch.float32, device=DEV) if d is not None and g != 0.0 else None
    vel = (-v).float() if v is not None else None
    if mode == hip.SDE_EM:
        yn = y + h * (A * vel - Bc * y)
        yn = yn + g * z if z is not None else yn
        return dict(y=yn, y_in=yn)
    if mode == hip.SDE_LAST:
        yn = y + h * (A * vel - Bc * y)
        return dict(y=yn, y_in=yn)
    if mode == hip.SDE_HEUN1:
        K1 = A * vel - Bc * xhat
        xp = xhat + h * K1
        return dict(k1=K1, y=xp, y_in=xp)
    if mode == hip.SDE_HEUN2:
        xn = xhat + h * (k1 + (A * vel - Bc * y))
        xh = xn + g * z if z is not None else xn
        return dict(y=xn, xhat=xh, y_in=xh)
    xh = y + g * z if z is not None else y
    return dict(xhat=xh, y_in=xh)


def _run_stage(mode, e, n, offset, coef, shift, use_counter, gen_seed):
    """one launch on fresh buffers (shift 1: every base one element off its 16-byte boundary) -> (got, want) dicts"""
    from visualcloze_amd import hip
    g = torch.Generator().manual_seed(gen_seed)
    buf = lambda dt: torch.empty(n + 8, dtype=dt, device=DEV)[shift:shift + n]  # noqa: E731
    src = {k: (torch.randn(n, generator=g) * 2).to(DEV) for k in ("y", "xhat", "k1")}
    v0 = torch.randn(n, generator=g).to(DEV, torch.bfloat16)
    t = {k: buf(torch.float32).copy_(src[k]) for k in src}
    v = buf(torch.bfloat16).copy_(v0)
    y_in = buf(torch.bfloat16).fill_(7.0)
    table = torch.zeros(8, 5, dtype=torch.float32, device=DEV)
    table[:, 0] = -1.0                                          # every other row: no mode, nothing written
    table[e] = torch.tensor([float(mode)] + list(coef))
    rng = hip.rng_words(SEED, offset, DEV)
    counter = torch.tensor([e], dtype=torch.int32, device=DEV)
    vv = None if mode == hip.SDE_INJECT else v
    hip.sde_stage(-1 if use_counter else e, table, t["y"], vv, y_in, rng, xhat=t["xhat"], k1=t["k1"], eval_ptr=counter if use_counter else None)
    torch.cuda.synchronize()
    want = _expect(mode, e, n, offset, src["y"], src["xhat"], src["k1"], vv, _f32s(coef))
    got = dict(y=t["y"], xhat=t["xhat"], k1=t["k1"], y_in=y_in)
    full = {k: want.get(k, src[k]) for k in src}
    full["y_in"] = want["y_in"].to(torch.bfloat16)
    assert torch.equal(v, v0)
    return got, full


@pytest.mark.parametrize("n,shift", [(8, 0), (1031, 0), (1031, 1), (8 * 520, 0), (8 * 520 + 5, 0)])
def test_stage_equals_the_torch_expressions_bitwise(n, shift):
    """n = 8: one 16-byte work item; 1031 = 128 chunks + a tail of 7, and with every base shifted the element-wise path; 8 * 520 chunks
    over more than one block, and with a tail.  Offsets: phase 0, phase 3, one just below 2^32 and one whose block counter
    (position >> 2) carries into its high word.  The counter at 0, 1 and 5."""
    from visualcloze_amd import hip
    modes = (hip.SDE_EM, hip.SDE_HEUN1, hip.SDE_HEUN2, hip.SDE_LAST, hip.SDE_INJECT)
    offsets = (0, 3, (1 << 32) - 5, (1 << 34) - 5)
    for mode in modes:
        for oi, offset in enumerate(offsets):
            for e in (0, 1, 5):
                if oi >= 2 and e != 1:
                    continue                                    # the large offsets: one counter each
                got, want = _run_stage(mode, e, n, offset, ROW, shift, use_counter=(e != 0), gen_seed=n + mode)
                for k in want:
                    assert torch.equal(got[k], want[k]), (f"mode {mode}, offset {offset}, counter {e}: {k} differs in "
                                                          f"{(got[k] != want[k]).float().mean().item():.4f} of the elements")


def test_stage_counters_draw_different_noise_and_the_guards():
    from visualcloze_amd import hip
    n = 1031
    runs = {e: _run_stage(hip.SDE_EM, e, n, 3, ROW, 0, True, 99)[0]["y"].clone() for e in (0, 1, 5)}
    again = _run_stage(hip.SDE_EM, 5, n, 3, ROW, 0, True, 99)[0]["y"]
    assert torch.equal(again, runs[5])                                            # the same counter: the same bits
    assert not torch.equal(runs[0], runs[1]) and not torch.equal(runs[1], runs[5])  # another counter: another draw
    # Heun's second stage draws the NEXT step's noise: counters 1 and 2 share draw 1, counter 3 takes draw 2
    h2 = {e: _run_stage(hip.SDE_HEUN2, e, n, 3, ROW, 0, True, 98)[0]["xhat"].clone() for e in (1, 2, 3)}
    assert torch.equal(h2[1], h2[2]) and not torch.equal(h2[2], h2[3])
    # g == 0: no noise term, not even a signed zero
    got, want = _run_stage(hip.SDE_EM, 1, n, 3, ROW[:3] + (0.0,), 0, True, 97)
    assert torch.equal(got["y"], want["y"])
    # a counter outside the table, a row without a mode, a Heun row without its buffers: nothing is written
    table = torch.zeros(4, 5, dtype=torch.float32, device=DEV)
    table[:, 0] = float(hip.SDE_EM)
    table[2, 0] = 9.0
    table[3, 0] = float(hip.SDE_HEUN2)
    y = torch.ones(n, device=DEV)
    v = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    y_in = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    rng = hip.rng_words(SEED, 0, DEV)
    for e in (-3, 4, 2, 3):
        hip.sde_stage(-1, table, y, v, y_in, rng, eval_ptr=torch.tensor([e], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert (y == 1.0).all() and (y_in.float() == 7.0).all()
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*sde_stage"):
        hip.sde_stage(4, table, y, v, y_in, rng)                                  # an explicit row outside the table
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*sde_stage"):
        hip.sde_stage(-1, table, y, v, y_in, rng)                                 # the device-side row needs the counter


def test_stage_grid_stride_loop_past_the_capped_grid():
    """2048 blocks x 256 threads x 8 elements + 24: every thread takes a second work item (16 MB of state)"""
    from visualcloze_amd import hip
    n = 2048 * 256 * 8 + 24
    got, want = _run_stage(hip.SDE_EM, 5, n, 3, ROW, 0, True, 5)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------- 2. fused == eager twin
def _twin(m, x, kw, opts, seed, offset, cfg_scale=None):
    """the eager restatement: transport.sde_integrate through Flux.forward as a foreign callable, hip.randn draws for the whole batch"""
    from visualcloze_amd import transport as T
    lss = opts["last_step_size"] if opts["last_step"] else 0.0
    t = torch.linspace(0.0, 1 - lss, opts["num_steps"])
    plan = T.sde_plan(opts["sampling_method"], opts["diffusion_form"], opts["diffusion_norm"], opts["last_step"], lss, t)
    if cfg_scale is None:
        fwd = lambda xin, **k: m.forward(xin, **k)  # noqa: E731
    else:
        fwd = lambda xin, **k: m.forward_with_cfg(xin, cfg_scale=cfg_scale, **k)  # noqa: E731
    return T._sample_sde_foreign(fwd, x, dict(kw), plan, seed, offset, True, bf16_out=True), plan


SETTINGS = {
    "euler_mean": dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=0.7, last_step="Mean", last_step_size=0.25, num_steps=4),
    "heun_tweedie": dict(sampling_method="Heun", diffusion_form="decreasing", diffusion_norm=0.7, last_step="Tweedie", last_step_size=0.25,
                         num_steps=4),
}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("case", ["b1", "b2_ragged"])
def test_fused_equals_the_eager_twin_bitwise(model, case, setting):
    from tests.procedural import tiny_inputs
    from visualcloze_amd.pipeline import NoiseStream
    m, _ = model
    inp = tiny_inputs(B=2, seed=7) if case == "b2_ragged" else tiny_inputs(B=1)
    if case == "b2_ragged":
        inp["img_mask"][1, -12:] = 0
        inp["txt_mask"][0, -5:] = 0
    kw = _kw(inp)
    opts = SETTINGS[setting]
    x = inp["x"].to(DEV, torch.float32)
    rng = NoiseStream(SEED, 1003, device=DEV)
    fused = _sampler().sample_sde(rng=rng, return_trajectory=True, **opts)(x, m.forward, **kw)
    torch.cuda.synchronize()
    eager, plan = _twin(m, x, kw, opts, SEED, 1003)
    assert fused.dtype == torch.float32 and fused.shape == (4,) + tuple(x.shape) and torch.isfinite(fused).all()
    for i in range(4):
        assert torch.equal(fused[i], eager[i]), f"row {i}: {(fused[i] != eager[i]).float().mean().item():.4f} of the elements differ"
    assert rng.offset == 1003 + plan["draws"] * x.numel()
    assert not torch.equal(fused[0], x) and not torch.equal(fused[-1], fused[-2])        # x' of step 0, and a last step that moved
    # a bf16 caller: widened on entry, stepped in f32, rounded once per output
    xb = x.to(torch.bfloat16)
    f16 = _sampler().sample_sde(rng=NoiseStream(SEED, 1003, device=DEV), return_trajectory=True, **opts)(xb, m.forward, **kw)
    f32 = _sampler().sample_sde(rng=NoiseStream(SEED, 1003, device=DEV), return_trajectory=True, **opts)(xb.float(), m.forward, **kw)
    last = _sampler().sample_sde(rng=NoiseStream(SEED, 1003, device=DEV), **opts)(xb, m.forward, **kw)
    assert f16.dtype == torch.bfloat16 and torch.equal(f16, f32.to(torch.bfloat16))
    assert not torch.equal(f32[-1].to(torch.bfloat16).float(), f32[-1])
    assert last.shape == (1,) + tuple(x.shape) and torch.equal(last[0], f16[-1])


def test_true_cfg_steps_both_halves(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd.pipeline import NoiseStream
    m, _ = model
    inp = tiny_inputs(B=2, seed=7)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.float32)
    for setting in sorted(SETTINGS):
        opts = SETTINGS[setting]
        fused = _sampler().sample_sde(rng=NoiseStream(SEED, 8, device=DEV), return_trajectory=True, **opts)(
            x, m.forward_with_cfg, cfg_scale=2.5, **kw)
        eager, _ = _twin(m, x, kw, opts, SEED, 8, cfg_scale=2.5)
        assert torch.equal(fused, eager), setting
        assert not torch.equal(fused[-1][0], x[0]) and not torch.equal(fused[-1][1], x[1])      # both halves move
        plain = _sampler().sample_sde(rng=NoiseStream(SEED, 8, device=DEV), **opts)(x, m.forward, **kw)
        assert not torch.equal(plain[-1][0], fused[-1][0])                                        # the combine reached the conditional half


def test_replays_and_seeds(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd.pipeline import NoiseStream
    m, _ = model
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.bfloat16)
    opts = SETTINGS["euler_mean"]
    run = lambda seed, off: _sampler().sample_sde(rng=NoiseStream(seed, off, device=DEV), return_trajectory=True, **opts)(x, m.forward, **kw)  # noqa: E731
    a, b = run(5, 64), run(5, 64)
    assert torch.equal(a, b)                                                      # one captured step, replayed: the same noise again
    assert not torch.equal(run(6, 64), a) and not torch.equal(run(5, 65), a)      # another seed; the stream shifted by one
    rng = NoiseStream(5, 64, device=DEV)
    _sampler().sample_sde(rng=rng, **opts)(x, m.forward, **kw)
    assert rng.offset == 64 + 3 * x.numel()
    # rng=None: the seed comes from torch's default generator
    torch.manual_seed(21)
    c = _sampler().sample_sde(**opts)(x, m.forward, **kw)
    torch.manual_seed(21)
    d = _sampler().sample_sde(**opts)(x, m.forward, **kw)
    torch.manual_seed(22)
    e = _sampler().sample_sde(**opts)(x, m.forward, **kw)
    assert torch.equal(c, d) and not torch.equal(c, e)


def test_option_off_changes_nothing_the_node_count_and_the_refusals():
    from tests.helpers import tiny_model
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.pipeline import NoiseStream
    from visualcloze_amd.transport import StepCache
    m, _ = tiny_model()                                                   # a handle that never heard of the option
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    x = inp["x"].to(DEV, torch.bfloat16)
    h = m.handle()
    L = hip.lib()
    B, T_, N = 1, kw["txt"].shape[1], x.shape[1]
    euler = lambda: _sampler().sample_ode(sampling_method="euler", num_steps=5, do_shift=True, time_shifting_factor=1,  # noqa: E731
                                          return_trajectory=True)(x, m.forward, kw)
    sizes = lambda: [L.vc_flux_workspace_bytes(h.h, B, T_, N, S) for S in (4, 7, 30)]  # noqa: E731
    before = sizes()
    e0 = euler()
    ode_nodes = h.step_nodes()
    h.set_sde(True)
    n = B * N * x.shape[2]
    assert all(o - b >= 3 * n * 4 + (S + 1) * 5 * 4 + 16 for o, b, S in zip(sizes(), before, (4, 7, 30)))     # y, xhat, K1, table, words
    h.set_sde(False)
    assert sizes() == before
    opts = SETTINGS["euler_mean"]
    s0 = _sampler().sample_sde(rng=NoiseStream(3, device=DEV), **opts)(x, m.forward, **kw)
    assert h.step_nodes() == ode_nodes                                    # the Euler-Maruyama step: the nodes of the ODE Euler step
    assert h.ws_options["sde"] == 0 and sizes() == before                               # the sampler leaves the option off behind it
    assert torch.equal(euler(), e0) and h.step_nodes() == ode_nodes       # the same Euler bits and nodes after an SDE run on the handle
    # the refusals, on the handle directly
    t = torch.linspace(0, 0.75, 4)
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        prep = lambda S=4: h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S, stream=s)  # noqa: E731
        sde = lambda xs, **k: h.sample_sde(k.pop("method", "Euler"), xs, kw["cond"], t, True, s, form=k.pop("form", "sigma"), norm=0.7,  # noqa: E731
                                           last_step="Mean", last_step_size=0.25, seed=3, offset=0, **k)
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*sde"):                      # VC_ERR_STATE: the option is off
            sde(x.clone())
        h.set_sde(True)
        h.set_step_cache(StepCache(0.1))
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*step cache"):               # VC_ERR_ARG
            sde(x.clone())
        h.set_step_cache(None)
        prep()
        h.set_monitor(1, 8)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*monitor"):
            sde(x.clone())
        h.set_monitor(0)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*max_steps|\(-1\).*evaluations"):
            sde(x.clone(), method="Heun")                                                  # 7 evaluations, 4 prepared
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*SBDM"):
            sde(x.clone(), form="SBDM")                                                    # the plan's refusal, before the device
        x1 = x.clone()                                                                     # ... and the handle is usable afterwards
        sde(x1)
        h.set_sde(False)
    torch.cuda.synchronize()
    assert torch.equal(x1[None], s0)
    assert torch.equal(euler(), e0)


def test_the_pipeline_passes_it_through(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import pipeline
    m, _ = model
    inp = tiny_inputs(B=1)
    noise = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16) for _ in range(2)]
    lat = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16) for _ in range(2)]
    masks = [torch.ones(1, 1, 64, 192, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    txt, vec = inp["txt"].to(DEV, torch.bfloat16), inp["y"].to(DEV, torch.bfloat16)
    sde = dict(diffusion_form="sigma", last_step_size=0.25)
    rng = pipeline.NoiseStream(9, device=DEV)
    rows = pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=3, sde=sde, rng=rng)
    euler = pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=3)
    assert all(torch.isfinite(r.float()).all() for r in rows) and not torch.equal(rows[0], euler[0])
    assert rng.offset == 2 * sum(r.numel() for r in noise)
    with pytest.raises(ValueError, match="NoiseStream"):
        pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=3, sde=sde)
    with pytest.raises(ValueError, match="use_grid_handle"):
        pipeline.generate_grid(m, None, None, None, [], [], None, None, 0, sde=sde, rng=rng, use_grid_handle=True)
    with pytest.raises(ValueError, match="NoiseStream"):
        pipeline.generate_grid(m, None, None, None, [], [], None, None, 0, sde=sde)
