"""-m gpu: the Adams-Bashforth multistep solve in the fused loop (vc_ms_stage, vc_flux_sample_multistep).

  * vc_ms_stage against the torch f32 expression, bit for bit in the f32 state and the bf16 y_in: orders 1 to 4, evaluations 0 .. 7 (the
    ring wraps twice), the row given explicitly and through the device-side counter, the element-wise path (a size that is no multiple
    of 8; every base off its 16-byte boundary), the 16-byte path, and the grid-stride loop past the capped grid; a row outside the
    table writes nothing;
  * the start reads nothing it did not write: a ring and a y_in full of NaN give the bits of a zero-filled ring - the kernel alone
    and a fresh handle whose whole workspace is poisoned;
  * the fused solve == the eager twin (transport.multistep_integrate through Flux.forward), bit for bit: orders 2, 3, 4, f32 and bf16
    callers, true CFG on two pairs, an SDEdit grid;
  * one captured step serves every order, the node count, the option off, the refusals, the pipeline's pass-through.
Image quality at any order and the throughput of the step are not measured here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID = [0.0, 0.05, 0.13, 0.22, 0.34, 0.47, 0.63, 0.80, 1.0]          # 8 steps of growing size: every row of every order differs


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
def _buffers(n, shift, fill=None):
    """y f32 [n], v / y_in bf16 [n], hist bf16 [3 n]; shift 1: every base one element off its 16-byte boundary (2 bytes for bf16)"""
    def buf(dt, count):
        t = torch.empty(count + 8, dtype=dt, device=DEV)
        if fill is not None:
            t.fill_(fill)
        return t[shift:shift + count]
    return buf(torch.float32, n), buf(torch.bfloat16, n), buf(torch.bfloat16, 3 * n), buf(torch.bfloat16, n)


def _expect(row, y, past):
    """the torch f32 expression of one row; past[j] = v_{e-j} (bf16)"""
    c0, c1, c2, c3 = (float(c) for c in row)
    f = [(-p).float() for p in past]
    z = c0 * f[0]
    if c1 != 0.0:
        z = z + c1 * f[1]
    if c2 != 0.0:
        z = z + c2 * f[2]
    y = y + z
    if c3 != 0.0:
        y = y + c3 * f[3]
    return y


def _run_sequence(order, n, shift, evals, counter_from=4, seed=0, hist_fill=0.0):
    """evaluations 0 .. evals - 1 of one trajectory on fresh buffers, each checked against the torch expression; -> the final y"""
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    rows = T.ms_plan(order, torch.tensor(GRID))["rows"]
    table = torch.from_numpy(rows).to(DEV)
    g = torch.Generator().manual_seed(seed + n)
    y, v, hist, y_in = _buffers(n, shift)
    y.copy_((torch.randn(n, generator=g) * 2).to(DEV))
    hist.fill_(hist_fill)
    y_in.fill_(7.0)
    want, past = y.clone(), []
    ring = hist.clone().view(3, n)
    for e in range(evals):
        v.copy_(torch.randn(n, generator=g).to(DEV, torch.bfloat16))
        past.insert(0, v.clone())
        use_counter = e >= counter_from                       # the first rows explicitly, the others through the device-side counter
        counter = torch.tensor([e], dtype=torch.int32, device=DEV) if use_counter else None
        hip.ms_stage(-1 if use_counter else e, table, y, v, hist, y_in, eval_ptr=counter)
        want = _expect(rows[e], want, past[:4])
        ring[e % 3] = past[0]
        assert torch.equal(y, want), f"order {order}, n {n}, evaluation {e}: y differs in {(y != want).float().mean().item():.4f} of the elements"
        assert torch.equal(y_in, want.to(torch.bfloat16)), f"order {order}, n {n}, evaluation {e}: y_in"
        assert torch.equal(hist.view(3, n), ring), f"order {order}, n {n}, evaluation {e}: the ring"
        assert torch.equal(v, past[0])
    return y.clone()


@pytest.mark.parametrize("counter_from", [0, 4])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("n,shift", [(8 * 5 + 3, 0), (8 * 64, 1), (8 * 64, 0), (8 * 300, 0)])
def test_stage_equals_the_torch_expression_bitwise(n, shift, order, counter_from):
    """8 * 5 + 3: no multiple of 8, element-wise (the ring's planes are not 16-byte aligned); 8 * 64 with every base shifted by one
    element: element-wise again; 8 * 64 and 8 * 300 (more than one block) aligned: 16-byte accesses.  Evaluations 0 .. 7.
    counter_from 0: every row - the start's rows with their zero coefficients included - through the device-side counter; 4: the
    first four rows through the explicit argument, the others through the counter."""
    _run_sequence(order, n, shift, evals=8, counter_from=counter_from)


def test_stage_grid_stride_loop_past_the_capped_grid():
    """1024 blocks x 256 threads x 8 elements + 8: the smallest n at which a thread takes a second work item on the 16-byte path
    (8 MB of state); order 4, evaluations 0 .. 4, so every ring slot is read once"""
    _run_sequence(4, 1024 * 256 * 8 + 8, 0, evals=5, counter_from=0)


def test_stage_row_outside_the_table_and_argument_errors():
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    n = 8 * 64
    table = torch.from_numpy(T.ms_plan(4, torch.tensor(GRID))["rows"]).to(DEV)
    y, v, hist, y_in = _buffers(n, 0, fill=3.0)
    v.fill_(1.0)
    for e in (-3, 8, 1 << 20):
        hip.ms_stage(-1, table, y, v, hist, y_in, eval_ptr=torch.tensor([e], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert (y == 3.0).all() and (hist.float() == 3.0).all() and (y_in.float() == 3.0).all()
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*ms_stage"):
        hip.ms_stage(8, table, y, v, hist, y_in)                                  # an explicit row outside the table
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*ms_stage"):
        hip.ms_stage(-1, table, y, v, hist, y_in)                                 # the device-side row needs the counter
    torch.cuda.synchronize()
    assert (y == 3.0).all()


# ---------------------------------------------------------------------------------------------- 2. the start reads nothing it did not write
def test_stage_start_ignores_a_poisoned_ring():
    """order 4, 7 steps: the ring and y_in allocated inside poisoned_empty(0xFF) hold NaN (and 0 * NaN would be NaN)"""
    from tests.poison import holds, poisoned_empty
    from visualcloze_amd import hip
    from visualcloze_amd import transport as T
    n = 8 * 64
    table = torch.from_numpy(T.ms_plan(4, torch.tensor(GRID[:8]))["rows"]).to(DEV)
    g = torch.Generator().manual_seed(11)
    y0 = (torch.randn(n, generator=g) * 2).to(DEV)
    vs = [torch.randn(n, generator=g).to(DEV, torch.bfloat16) for _ in range(7)]
    out = {}
    for byte in (0x00, 0xFF):
        with poisoned_empty(byte) as p:
            hist, y_in = torch.empty(3 * n, dtype=torch.bfloat16, device=DEV), torch.empty(n, dtype=torch.bfloat16, device=DEV)
        assert p.count == 2 and holds(hist, byte) and holds(y_in, byte)
        assert byte == 0x00 or (torch.isnan(hist.float()).all() and torch.isnan(y_in.float()).all())
        y = y0.clone()
        for e in range(7):
            hip.ms_stage(e, table, y, vs[e], hist, y_in)
        out[byte] = (y, y_in)
    assert torch.isfinite(out[0xFF][0]).all() and torch.isfinite(out[0xFF][1].float()).all()
    assert torch.equal(out[0xFF][0], out[0x00][0]) and torch.equal(out[0xFF][1], out[0x00][1])
    assert not torch.equal(out[0x00][0], y0)


def test_fused_start_ignores_a_poisoned_workspace():
    """a fresh model and handle per pattern: the whole workspace (state, ring, table, y_in included) holds the pattern before prepare"""
    from tests.helpers import tiny_model
    from tests.poison import poisoned_empty
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=2, seed=7)
    out = {}
    for byte in (0x00, 0xFF):
        with poisoned_empty(byte) as p:
            m, _ = tiny_model()
            x = inp["x"].to(DEV, torch.float32)
            out[byte] = _sampler().sample_ode_multistep(order=4, num_steps=8, do_shift=True, time_shifting_factor=1,
                                                        return_trajectory=True)(x, m.forward, _kw(inp))
        assert p.count > 0
    assert torch.isfinite(out[0xFF]).all() and torch.equal(out[0xFF], out[0x00])


# ---------------------------------------------------------------------------------------------- 3. fused == eager twin
def _twin(m, x, kw, order, num_steps, strength=None, cfg_scale=None):
    """the eager restatement: transport.multistep_integrate through Flux.forward as a foreign callable, the velocity kept in bf16"""
    from visualcloze_amd import transport as T
    t = T.solver_time_grid(num_steps, x.shape[1], 0.0 if strength is None else strength, 1, True, 1)
    if cfg_scale is None:
        fwd = lambda xin, **k: m.forward(xin, **k)  # noqa: E731
    else:
        fwd = lambda xin, **k: m.forward_with_cfg(xin, cfg_scale=cfg_scale, **k)  # noqa: E731
    return T._sample_multistep_foreign(fwd, x, dict(kw), t, order, True, bf16_out=True)


def _fused(m, x, kw, order, num_steps, strength=None, cfg_scale=None, trajectory=True):
    fn = _sampler().sample_ode_multistep(order=order, num_steps=num_steps, do_shift=True, time_shifting_factor=1, strength=strength,
                                         return_trajectory=trajectory)
    if cfg_scale is None:
        return fn(x, m.forward, kw)
    return fn(x, m.forward_with_cfg, dict(kw, cfg_scale=cfg_scale))


@pytest.fixture(scope="module")
def b2():
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=2, seed=7)
    return inp, _kw(inp)


@pytest.mark.parametrize("order", [2, 3, 4])
def test_fused_equals_the_eager_twin_bitwise(model, b2, order):
    m, _ = model
    inp, kw = b2
    x = inp["x"].to(DEV, torch.float32)
    fused = _fused(m, x, kw, order, 9)
    torch.cuda.synchronize()
    eager = _twin(m, x, kw, order, 9)
    assert fused.dtype == torch.float32 and fused.shape == (9,) + tuple(x.shape) and torch.isfinite(fused).all()
    assert torch.equal(fused[0], x)
    for i in range(9):
        assert torch.equal(fused[i], eager[i]), f"row {i}: {(fused[i] != eager[i]).float().mean().item():.4f} of the elements differ"
    assert not torch.equal(fused[-1], fused[-2])
    # a bf16 caller: widened on entry, stepped in f32, rounded once per output
    xb = x.to(torch.bfloat16)
    f16 = _fused(m, xb, kw, order, 9)
    f32 = _fused(m, xb.float(), kw, order, 9)
    last = _fused(m, xb, kw, order, 9, trajectory=False)
    assert f16.dtype == torch.bfloat16 and torch.equal(f16, f32.to(torch.bfloat16))
    assert torch.equal(f16, _twin(m, xb, kw, order, 9))
    assert not torch.equal(f32[-1].to(torch.bfloat16).float(), f32[-1])
    assert last.shape == (1,) + tuple(x.shape) and torch.equal(last[0], f16[-1])


@pytest.mark.parametrize("order", [2, 4])
def test_fused_with_true_cfg_and_with_strength(model, b2, order):
    from tests.procedural import tiny_inputs
    m, _ = model
    inp4 = tiny_inputs(B=4, seed=5)                                               # two pairs (j, j + 2)
    kw4 = _kw(inp4)
    x4 = inp4["x"].to(DEV, torch.float32)
    fused = _fused(m, x4, kw4, order, 9, cfg_scale=2.5)
    eager = _twin(m, x4, kw4, order, 9, cfg_scale=2.5)
    assert torch.equal(fused, eager)
    assert all(not torch.equal(fused[-1][b], x4[b]) for b in range(4))           # both halves move
    plain = _fused(m, x4, kw4, order, 9, trajectory=False)
    assert not torch.equal(plain[-1][0], fused[-1][0])                            # the combine reached the conditional half
    # an SDEdit grid: the solve starts at t = 0.4
    inp, kw = b2
    for x in (inp["x"].to(DEV, torch.float32), inp["x"].to(DEV, torch.bfloat16)):
        fused = _fused(m, x, kw, order, 9, strength=0.4)
        assert torch.equal(fused, _twin(m, x, kw, order, 9, strength=0.4))
        assert not torch.equal(fused[-1], _fused(m, x, kw, order, 9)[-1])


# ---------------------------------------------------------------------------------------------- 4. one graph, the option, the refusals
PLAN_CAPACITY = 4          # the handle's list of captured steps: at 4 a new capture evicts one and the count stays


def test_one_captured_step_serves_every_order(b2):
    """on a handle of its own: the count of captured steps tells a new capture only while it is below the list's capacity"""
    from tests.helpers import tiny_model
    m, _ = tiny_model()
    inp, kw = b2
    x = inp["x"].to(DEV, torch.bfloat16)
    h = m.handle()
    assert h.plan_count() == 0
    _sampler().sample_ode(sampling_method="euler", num_steps=9, do_shift=True, time_shifting_factor=1)(x, m.forward, kw)
    euler_nodes = h.step_nodes()
    assert h.plan_count() == 1
    a = _fused(m, x, kw, 2, 9)
    plans, nodes = h.plan_count(), h.step_nodes()
    assert plans == 2 < PLAN_CAPACITY                                             # the multistep step was captured, and the count can still move
    assert nodes == euler_nodes and nodes[1:] == (0, 0)                           # the Euler step's node count, one graph
    b = _fused(m, x, kw, 4, 9)
    assert h.plan_count() == plans and h.step_nodes() == nodes                    # order 4 on the same geometry captured nothing
    assert torch.equal(_fused(m, x.float(), kw, 4, 9).to(torch.bfloat16), b)      # an f32 caller: the same f32-state step again
    assert h.plan_count() == plans
    assert torch.equal(b, _twin(m, x, kw, 4, 9)) and not torch.equal(a[-1], b[-1])
    assert torch.equal(_fused(m, x, kw, 2, 9), a) and h.plan_count() == plans     # ... and order 2 again replays the same bits
    _sampler().sample_ode(sampling_method="midpoint", num_steps=9, do_shift=True, time_shifting_factor=1)(x, m.forward, kw)
    assert h.plan_count() == plans + 1                                            # (the count does move where a step IS captured)


def test_option_off_changes_nothing_and_the_refusals():
    from tests.helpers import tiny_model
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
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
    h.set_multistep(True)
    n = B * N * x.shape[2]
    assert all(o - b >= n * 4 + 3 * n * 2 + S * 4 * 4 for o, b, S in zip(sizes(), before, (4, 7, 30)))     # the state, the ring, the table
    h.set_multistep(False)
    assert sizes() == before
    s0 = _fused(m, x, kw, 3, 5, trajectory=False)
    assert h.step_nodes() == ode_nodes
    assert h.ws_options["multistep"] == 0 and sizes() == before                         # the sampler leaves the option off behind it
    assert torch.equal(euler(), e0) and h.step_nodes() == ode_nodes       # the same Euler bits and nodes after a multistep run on the handle
    # the refusals, on the handle directly
    from visualcloze_amd.transport import solver_time_grid
    t = solver_time_grid(5, N, 0.0, 1, True, 1)
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        prep = lambda S=4: h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S, stream=s)  # noqa: E731
        ms = lambda xs, order=3, grid=t: h.sample_multistep(order, xs, kw["cond"], grid, True, s)  # noqa: E731
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*multistep"):                # VC_ERR_STATE: the option is off
            ms(x.clone())
        xe = x.clone()
        h.sample_ode("euler", xe, kw["cond"], t, True, s)                                  # ... and the handle runs Euler afterwards
        h.set_multistep(True)
        h.set_step_cache(StepCache(0.1))
        prep()
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*step cache"):               # VC_ERR_ARG
            ms(x.clone())
        h.set_step_cache(None)
        prep()
        h.set_monitor(1, 8)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*monitor"):
            ms(x.clone())
        h.set_monitor(0)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*evaluations"):
            ms(x.clone(), grid=solver_time_grid(7, N, 0.0, 1, True, 1))                    # 6 evaluations, 4 prepared
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*order"):
            ms(x.clone(), order=5)                                                         # the plan's refusal, before the device
        h.set_cfg(2.0)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*odd"):
            ms(x.clone())                                                                  # true CFG with B = 1
        h.set_cfg(None)
        x1 = x.clone()                                                                     # ... and the handle is usable afterwards
        ms(x1)
        h.set_multistep(False)
    torch.cuda.synchronize()
    assert torch.equal(x1[None], s0)
    assert torch.equal(xe, e0[-1])
    assert torch.equal(euler(), e0)


def test_the_pipeline_passes_it_through(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import packing, pipeline
    from visualcloze_amd.transport import StepCache
    m, _ = model
    inp = tiny_inputs(B=1)
    noise = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16) for _ in range(2)]
    lat = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16) for _ in range(2)]
    masks = [torch.ones(1, 1, 64, 192, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    txt, vec = inp["txt"].to(DEV, torch.bfloat16), inp["y"].to(DEV, torch.bfloat16)
    ms = dict(order=3)
    rows = pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=5, multistep=ms)
    # ... equals the sampler called directly on the packed grid
    img, img_ids, img_mask = packing.prepare_grid([noise])
    cond = packing.pack_cond(lat, masks)
    fn = _sampler().sample_ode_multistep(order=3, num_steps=5, do_shift=True, time_shifting_factor=1)
    direct = fn(img, m.forward, pipeline._kwargs(img_ids, img_mask, txt, vec, cond, 30.0, torch.device(DEV)))[-1][:1]
    want = packing.unpack_rows(direct, [tuple(r.shape[-2:]) for r in noise])
    assert len(rows) == len(want) == 2 and all(torch.equal(a, b) for a, b in zip(rows, want))
    euler = pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=5)
    assert all(torch.isfinite(r.float()).all() for r in rows) and not torch.equal(rows[0], euler[0])
    for kw, match in ((dict(use_grid_handle=True), "use_grid_handle"), (dict(adaptive=dict(rtol=1e-2, atol=1e-6)), "adaptive"),
                      (dict(sde=dict(diffusion_form="sigma")), "sde"), (dict(step_cache=StepCache(0.1)), "step_cache")):
        with pytest.raises(ValueError, match=r"multistep.*" + match):
            pipeline.generate_grid(m, None, None, None, [], [], None, None, 0, multistep=ms, **kw)
    with pytest.raises(ValueError, match="multistep"):
        pipeline.denoise_grid(m, noise, lat, masks, txt, vec, cfg=30.0, steps=5, multistep=ms, step_cache=StepCache(0.1))


def test_generate_grid_multistep_equals_the_sampler_called_directly(model, monkeypatch):
    """pixels in, pixels out on the tiny model, autoencoder and text encoders: generate_grid(multistep=dict(order=3)) == the rows of
    Sampler.sample_ode_multistep(order=3) on the packed grid, decoded - and not the Euler result; the monitor= re-entry hands the
    keyword on"""
    from tests.procedural import TINY, TINY_T5, procedural_ae_param, procedural_text_param, ptensor, tiny_ids
    from visualcloze_amd import packing, pipeline
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m, _ = model
    AE = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 1, 1, 1], num_res_blocks=1, z_channels=16,
              scale_factor=0.3611, shift_factor=0.1159)
    CL = dict(vocab_size=128, hidden_size=TINY["vec_in_dim"], intermediate_size=128, num_hidden_layers=1,
              num_attention_heads=1, max_position_embeddings=16, layer_norm_eps=1e-5, eos_token_id=127)
    ae = AutoEncoder(AutoEncoderParams(**AE))
    ae.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in ae.state_dict().items()})
    ae = ae.to(DEV).to(torch.bfloat16)
    t5 = T5EncoderModel(T5Config(**TINY_T5))
    tsd = {k: procedural_text_param(k, v.shape) for k, v in t5.state_dict().items()}
    tsd["encoder.embed_tokens.weight"] = tsd["shared.weight"]
    t5.load_state_dict(tsd)
    t5 = t5.to(DEV).to(torch.bfloat16)
    clip = CLIPTextModel(CLIPTextConfig(**CL))
    clip.load_state_dict({k: procedural_text_param(k, v.shape) for k, v in clip.state_dict().items()})
    clip = clip.to(DEV).to(torch.bfloat16)
    H, W = 32, 64
    c = lambda t: t.to(DEV, torch.bfloat16)  # noqa: E731
    rows = [c(ptensor((3, H, W), 201 + i, q=7)) for i in range(2)]
    masks = [c(torch.zeros(1, 1, H, W)), c(torch.cat((torch.zeros(1, 1, H, W // 2), torch.ones(1, 1, H, W // 2)), -1))]
    enoise = [c(ptensor((1, 16, H // 8, W // 8), 211 + i, q=5)) for i in range(2)]
    t5_ids, clip_ids = tiny_ids(64, 128, seed=5)[None].to(DEV), tiny_ids(16, 128, seed=6, eos=127, eos_at=7)[None].to(DEV)
    args = (m, ae, t5, clip, rows, masks, t5_ids, clip_ids, 3)
    seen = []
    inner = pipeline.denoise_grid

    def spy(model_, noise_rows, cond_latent_rows, mask_rows, txt, vec, **k):          # what generate_grid hands to the solve
        seen.append(([t.clone() for t in noise_rows], [t.clone() for t in cond_latent_rows], mask_rows, txt, vec, dict(k)))
        return inner(model_, noise_rows, cond_latent_rows, mask_rows, txt, vec, **k)
    monkeypatch.setattr(pipeline, "denoise_grid", spy)
    got = pipeline.generate_grid(*args, cfg=30.0, steps=5, encode_noise=enoise, multistep=dict(order=3))
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][5]["multistep"] == dict(order=3)
    noise, lat, mask_rows, txt, vec, _ = seen[0]
    # ---- the sampler called directly on the packed grid, decoded as generate_grid decodes
    img, img_ids, img_mask = packing.prepare_grid([noise])
    cond = packing.pack_cond(lat, mask_rows)
    fn = _sampler().sample_ode_multistep(order=3, num_steps=5, do_shift=True, time_shifting_factor=1)
    direct = fn(img, m.forward, pipeline._kwargs(img_ids, img_mask, txt, vec, cond, 30.0, torch.device(DEV)))[-1][:1]
    want = [((ae.decode(z)[0].float() + 1.0) / 2.0).clamp_(0.0, 1.0) for z in packing.unpack_rows(direct, [tuple(r.shape[-2:]) for r in noise])]
    assert len(got) == len(want) == 2 and all(g.shape == (3, H, W) for g in got)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    euler = pipeline.generate_grid(*args, cfg=30.0, steps=5, encode_noise=enoise)
    assert not any(torch.equal(g, e) for g, e in zip(got, euler))                     # not the Euler solve
    # monitor=0 re-enters generate_grid: the keyword travels with it; a level above 0 is refused, by name
    again = pipeline.generate_grid(*args, cfg=30.0, steps=5, encode_noise=enoise, multistep=dict(order=3), monitor=0)
    assert seen[-1][5]["multistep"] == dict(order=3) and all(torch.equal(g, w) for g, w in zip(again, want))
    with pytest.raises(ValueError, match=r"multistep.*monitor"):
        pipeline.generate_grid(*args, cfg=30.0, steps=5, encode_noise=enoise, multistep=dict(order=3), monitor=1)
