"""-m gpu: the flow-matching loss (vc_fm_plan, vc_fm_loss, vc_flux_eval_loss, Transport.training_losses fused).

  * vc_fm_plan against the torch f32 expression, bit for bit: the 16-byte path (cols 64 into ld 384) and the element-wise path (cols 6
    into ld 11, x1 a view one element off), bf16 and f32 x1, t in {0, 1, 0.37} and different per sample, a tensor x0 and the in-kernel
    draw == hip.randn at the same seed / offset (a phase that is no multiple of 4, a block counter that carries into its high word),
    the destination outside [0, cols) untouched;
  * vc_fm_loss bit-equal to the ordered twin (transport.fm_loss_reduce) and within the f32 budget of a float64 reference: ragged valid
    rows, a size that straddles one block's share of units, one beyond the cap on blocks, the element-wise path, device and host
    counts, repeated runs, an inf;
  * the handle: vc_flux_eval_loss == plan -> Flux.forward -> ordered twin, with cond (without it: refused on the handle, the kernels around a toy model), ragged B = 2, a batch beyond the
    chunk, bf16 and f32, NoiseStream == the tensor it stands for, true CFG refused;
  * off means off: workspace bytes and node counts against a second handle, an Euler trajectory's bits after an eval_loss call.
The value of the loss on real weights is not measured here (only random-init weights exist)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()


def _kw(inp):
    return dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                guidance=inp["guidance"].to(DEV))


# ---------------------------------------------------------------------------------------------- 1. vc_fm_plan
def _plan_case(dtype, rows, cols, ld, shifted, t_vals, offset, draw):
    from visualcloze_amd import hip
    B = len(t_vals)
    g = torch.Generator().manual_seed(rows * 1000 + cols + int(shifted))
    flat = torch.randn(B * rows * cols + 8, generator=g).to(DEV, dtype)
    x1 = flat[int(shifted):int(shifted) + B * rows * cols].view(B, rows, cols)        # shifted: one element off its 16-byte boundary
    t = torch.tensor(t_vals, dtype=torch.float32, device=DEV)
    x0 = None if draw else torch.randn(B, rows, cols, generator=g).to(DEV, dtype)
    xt = torch.full((B, rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    ut = hip.fm_plan(x1, t, xt, x0=x0, seed=SEED, offset=offset)
    torch.cuda.synchronize()
    z = hip.randn((B, rows, cols), SEED, offset, dtype=dtype, device=DEV) if draw else x0
    tb = t.view(B, 1, 1)
    want_xt = (tb * x1.float() + (1 - tb) * z.float()).to(torch.bfloat16)               # the torch f32 expression, rounded once
    want_ut = x1.float() - z.float()
    assert torch.equal(xt[..., :cols], want_xt), f"x_t differs in {(xt[..., :cols] != want_xt).float().mean().item():.4f} of the elements"
    assert torch.equal(ut, want_ut) and ut.dtype == torch.float32
    assert bool((xt[..., cols:] == 7.0).all())                                         # the cond columns are the caller's
    return xt, ut


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geom", ["vec", "elem"])
def test_plan_equals_the_torch_expression_bitwise(dtype, geom):
    rows, cols, ld, shifted = (5, 64, 384, False) if geom == "vec" else (5, 6, 11, True)
    for t_vals in ((0.0, 1.0), (0.37, 0.81), (1.0, 0.37)):
        _plan_case(dtype, rows, cols, ld, shifted, t_vals, 0, draw=False)
    # the in-kernel draw: phase 0, a phase that is no multiple of 4, a block counter (position >> 2) that carries into its high word
    for offset in (0, 3, 1001, (1 << 34) - 5):
        _plan_case(dtype, rows, cols, ld, shifted, (0.37, 0.81), offset, draw=True)
    xt0, ut0 = _plan_case(dtype, rows, cols, ld, shifted, (0.0, 1.0), 3, draw=True)    # t = 0: x_t = x0; t = 1: x_t = x1
    assert torch.isfinite(ut0).all()


def test_plan_beyond_the_capped_grid():
    """more work items than 2048 blocks of 256 threads take in one round: the grid-stride loop (vector path, 8 elements per item)"""
    _plan_case(torch.bfloat16, 2048 * 256 * 8 // 64 + 3, 64, 64, False, (0.37,), 5, draw=True)


# ---------------------------------------------------------------------------------------------- 2. vc_fm_loss
def _loss_inputs(B, rows, cols, ld, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.full((B, rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    out[..., :cols] = torch.randn(B, rows, cols, generator=g).to(DEV, torch.bfloat16)
    ut = (torch.randn(B, rows, cols, generator=g) * 1.5).to(DEV)
    return out, ut


def _check_loss(out, ut, cols, valid):
    """bit-equal to the ordered twin; within the f32 budget of the float64 value.  The budget: d = (-out) - ut is one f32 rounding,
    d * d one more on top of twice d's, each of the n - 1 additions and the division one - (n + 4) * 2^-24 of the sum of the terms,
    whatever the order (tests/budget.py: f32_terms)."""
    from tests.budget import EPS24, assert_within_budget
    from visualcloze_amd import hip, transport as T
    B, rows = ut.shape[:2]
    mask = None
    if valid is not None:
        mask = torch.zeros(B, rows)
        for b, v in enumerate(valid):
            mask[b, :v] = 1
    dev_counts = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)
    got = hip.fm_loss(out[..., :cols], ut, dev_counts)
    again = hip.fm_loss(out[..., :cols], ut, dev_counts)
    host = hip.fm_loss(out[..., :cols], ut, None if valid is None else list(valid))
    torch.cuda.synchronize()
    twin = T.fm_loss_reduce(out[..., :cols].cpu(), ut.cpu(), mask, ordered=True)
    assert torch.equal(got.cpu(), twin), (got.cpu(), twin)
    assert torch.equal(got, again) and torch.equal(got, host)                         # repeated runs, host counts: the same bits
    d = (-out[..., :cols].double().cpu()) - ut.double().cpu()
    n = torch.tensor([rows * cols if valid is None else v * cols for v in (valid or [rows] * B)], dtype=torch.float64)
    keep = torch.ones(B, rows, 1, dtype=torch.float64) if mask is None else mask.double().unsqueeze(-1)
    ref = (d * d * keep).sum(dim=(1, 2)) / n
    worst = assert_within_budget(got, ref, roundings=0, f32_terms=(n + 4) * EPS24 * ref, what="fm_loss")
    print(f"fm_loss B={B} rows={rows} cols={cols} valid={valid}: worst ratio to the f32 budget {worst:.4f}")
    return got


def test_loss_ragged_valid_rows():
    out, ut = _loss_inputs(3, 70, 64, 64, 1)
    got = _check_loss(out, ut, 64, (70, 33, 1))
    full = _check_loss(out, ut, 64, None)
    assert torch.equal(got[0], full[0]) and not torch.equal(got[1], full[1])          # 70 of 70 rows: the unmasked mean


def test_loss_block_boundaries():
    from visualcloze_amd import hip
    upr = 64 // 8
    straddle = (256 + upr) // upr                      # 33 rows: 264 units, one more row than ONE block of 256 threads takes
    beyond = (hip.FM_LOSS_MAX_BLOCKS * 256) // upr + 8   # 8200 rows: 65600 units, past the cap of 256 blocks - a second round
    for rows in (straddle, beyond):
        out, ut = _loss_inputs(1, rows, 64, 64, rows)
        _check_loss(out, ut, 64, None)
        _check_loss(out, ut, 64, (rows - 1,))


def test_loss_element_path_and_a_column_window():
    out, ut = _loss_inputs(2, 37, 6, 11, 3)            # cols 6 of ld 11: short units, element loads
    _check_loss(out, ut, 6, (37, 5))
    out, ut = _loss_inputs(2, 9, 64, 384, 4)           # a window of a wider row, 16-byte loads
    _check_loss(out, ut, 64, (9, 2))


def test_loss_of_an_inf_is_inf():
    from visualcloze_amd import hip
    out, ut = _loss_inputs(2, 70, 64, 64, 5)
    out[1, 3, 17] = float("inf")
    got = hip.fm_loss(out, ut)
    torch.cuda.synchronize()
    assert torch.isfinite(got[0]) and got[1] == float("inf")
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*valid_rows\[1\] = 0"):
        hip.fm_loss(out, ut, [70, 0])


# ---------------------------------------------------------------------------------------------- 3. the handle
def _twin_loss(m, x1, kw, cond, t, x0):
    """plan -> Flux.forward -> the ordered reduction, in torch: what vc_flux_eval_loss computes"""
    from visualcloze_amd import transport as T
    fwd = lambda xin, **k: m.forward(xin, **k)  # noqa: E731        (a foreign callable: never the fused path)
    return T.fm_loss_terms(fwd, x1, t, x0, kw, cond, ordered=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", ["b1", "b2_ragged", "b6_chunks"])
def test_eval_loss_equals_plan_forward_twin_bitwise(model, case, dtype):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import transport as T
    from visualcloze_amd.pipeline import NoiseStream
    m, _ = model
    B = {"b1": 1, "b2_ragged": 2, "b6_chunks": 6}[case]
    inp = tiny_inputs(B=B, seed=7)
    if case == "b2_ragged":
        inp["img_mask"][1, -12:] = 0
        inp["img_mask"][0, 5] = 0                      # not a prefix: the handle reorders the rows valid-first
        inp["txt_mask"][0, -5:] = 0
    kw = _kw(inp)
    assert B <= m.max_batch() or case == "b6_chunks"
    x1 = inp["x"].to(DEV, dtype)
    cond = inp["cond"].to(DEV, torch.bfloat16)
    t = torch.tensor([0.37, 0.81, 0.05, 0.5, 0.93, 0.66][:B])
    x0 = torch.randn(x1.shape, generator=torch.Generator().manual_seed(B)).to(DEV, dtype)
    tr = T.create_transport()
    fused = tr.training_losses(m.forward, x1, kw, {"cond": cond}, t=t, x0=x0)
    torch.cuda.synchronize()
    twin = _twin_loss(m, x1, kw, cond, t.to(DEV), x0)
    assert fused["loss"].dtype == torch.float32 and fused["loss"].shape == (B,) and torch.isfinite(fused["loss"]).all()
    assert torch.equal(fused["loss"], twin["loss"]), (fused["loss"], twin["loss"])
    assert fused["t"].dtype == dtype and torch.equal(fused["t"].cpu(), t.to(dtype)) and not fused["loss"].requires_grad
    if case == "b6_chunks":
        return
    # rng = NoiseStream(s): the in-kernel draw == the tensor the stream holds there, IN THE HANDLE'S ROW ORDER; the offset advances
    rng = NoiseStream(SEED, 1003, device=DEV)
    drawn = tr.training_losses(m.forward, x1, kw, {"cond": cond}, t=t, rng=rng)
    assert rng.offset == 1003 + x1.numel()
    plan = m.chunk_plan(B, x1.shape[1], kw)
    z = plan.img_back(NoiseStream(SEED, 1003, device=DEV).randn(tuple(x1.shape), dtype=dtype), slice(0, B))
    given = tr.training_losses(m.forward, x1, kw, {"cond": cond}, t=t, x0=z)
    assert torch.equal(drawn["loss"], given["loss"]) and not torch.equal(drawn["loss"], fused["loss"])


def test_without_cond(model):
    """the handle exists for in_channels > out_channels only (vc_flux_create), so on a Flux the loss without cond is refused, never
    computed on a wrong input; a model whose input is x_t alone runs the two kernels around its own evaluation (the eager path:
    tests/test_fm_loss_cpu.py), here on the device with ld == cols - no cond columns beside x_t"""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip, transport as T
    m, _ = model
    inp = tiny_inputs(B=2, seed=3)
    kw = _kw(inp)
    x1 = inp["x"].to(DEV, torch.bfloat16)
    t = torch.tensor([0.25, 0.75])
    x0 = torch.randn(x1.shape, generator=torch.Generator().manual_seed(9)).to(DEV, torch.bfloat16)
    with pytest.raises(hip.VclozeHipError, match="in_channels"):
        T.create_transport().training_losses(m.forward, x1, kw, {"cond": None}, t=t, x0=x0)
    toy = lambda xin, timesteps, **k: (torch.sin(xin.float()) * (0.5 + timesteps.float().view(-1, 1, 1))).to(torch.bfloat16)  # noqa: E731
    twin = T.fm_loss_terms(toy, x1, t.to(DEV), x0, None, None, ordered=True)
    xt = torch.empty_like(x1)
    ut = hip.fm_plan(x1, t.to(DEV, torch.bfloat16).float(), xt, x0=x0)
    got = hip.fm_loss(toy(xt, (1 - t.to(DEV, torch.bfloat16))), ut)
    assert torch.equal(got, twin["loss"])


def test_true_cfg_is_refused_and_the_option_is_needed(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    m, _ = model
    inp = tiny_inputs(B=2, seed=7)
    kw = _kw(inp)
    h = m.handle()
    x1, cond = inp["x"].to(DEV, torch.bfloat16), inp["cond"].to(DEV, torch.bfloat16)
    prep = lambda: h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 1)  # noqa: E731
    prep()
    with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*eval_loss"):                # VC_ERR_STATE: the option is off
        h.eval_loss(x1, cond, [0.5, 0.5])
    h.set_eval_loss(True)
    try:
        prep()
        h.set_cfg(2.0)
        with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*CFG"):                  # VC_ERR_STATE
            h.eval_loss(x1, cond, [0.5, 0.5])
        h.set_cfg(None)
        with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*finite"):
            h.eval_loss(x1, cond, [0.5, float("nan")])
        assert torch.isfinite(h.eval_loss(x1, cond, [0.5, 0.5])).all()                 # ... and the handle is usable afterwards
    finally:
        h.set_cfg(None)
        h.set_eval_loss(False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. off means off
def test_off_means_off():
    from tests.helpers import tiny_model
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip, transport as T
    m, _ = tiny_model()                                # the handle the loss runs on
    other, _ = tiny_model()                            # a handle built the same way that never hears of the option
    inp = tiny_inputs(B=1)
    kw = dict(_kw(inp), cond=inp["cond"].to(DEV, torch.bfloat16))
    x = inp["x"].to(DEV, torch.bfloat16)
    L = hip.lib()
    B, T_, N = 1, kw["txt"].shape[1], x.shape[1]
    sizes = lambda h: [L.vc_flux_workspace_bytes(h.h, B, T_, N, S) for S in (1, 4, 30)]  # noqa: E731
    euler = lambda mm: T.Sampler(T.create_transport()).sample_ode(sampling_method="euler", num_steps=5, do_shift=True,  # noqa: E731
                                                                  time_shifting_factor=1, return_trajectory=True)(x, mm.forward, dict(kw))
    e_other = euler(other)
    e0 = euler(m)
    h, ho = m.handle(), other.handle()
    assert torch.equal(e0, e_other) and sizes(h) == sizes(ho) and h.step_nodes() == ho.step_nodes()
    loss_kw = {k: v for k, v in kw.items() if k != "cond"}
    terms = T.create_transport().training_losses(m.forward, x, loss_kw, {"cond": kw["cond"]}, t=torch.tensor([0.4]),
                                                 x0=torch.randn(x.shape, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16))
    assert torch.isfinite(terms["loss"]).all()
    assert h.ws_options["eval_loss"] == 0 and sizes(h) == sizes(ho)                                   # the option is off again behind the call
    h.set_eval_loss(True)
    n = B * N * x.shape[2]
    assert all(a - b >= n * 4 for a, b in zip(sizes(h), sizes(ho)))                     # u_t, carved only with the option
    h.set_eval_loss(False)
    assert sizes(h) == sizes(ho)
    e1 = euler(m)
    assert torch.equal(e1, e0) and h.step_nodes() == ho.step_nodes()                    # the same Euler bits and nodes after an eval_loss call
