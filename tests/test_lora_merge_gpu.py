"""GPU: vc_lora_merge (csrc/lora_merge.hip) - W' = bf16(W + s * B @ A), b' = bf16(b + s * b_B) - against torch on the CPU where the
arithmetic leaves no freedom (bit for bit), against the exact value under a derived bound everywhere else, against today's torch
merge, over the layouts prepare() uses, and through the tiny model with Flux.lora_merge = "hip"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
SHAPES = [(3072, 3072, 256), (9216, 3072, 256), (64, 3072, 64), (3072, 384, 256), (3072, 15360, 256),
          (4, 12, 4), (40, 24, 20), (130, 72, 33)]
RAGGED = SHAPES[5:]
# rank 257 .. 512: the LDS image of lora_A grows to 96 / 128 KiB (more than a launch gets by default, one workgroup per CU)
HIGH_RANK = [(320, 520, 300), (512, 520, 512), (400, 392, 384)]          # (rank <= min(out, in), the clip of lora.py:66-67)
# with exact partial sums, ANY scale leaves no freedom: s * acc rounds once, W + that rounds once - a fused multiply-add
# (one rounding) would differ, so 0.7 and -1.3 pin the two separate roundings
EXACT_SCALES = [1.0, 0.5, 0.7, -1.3]
TOL_GOLDEN = 3e-2          # the bound tests/test_model_gpu.py holds the torch path to


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


def gen(seed):
    return torch.Generator().manual_seed(seed)


def small_int_factors(O, I, R, seed):
    """entries k / 8, |k| <= 4: every product and every partial sum of B @ A is exact in f32 in any order"""
    g = gen(seed)
    A = (torch.randint(-4, 5, (R, I), generator=g).float() / 8).to(BF)
    B = (torch.randint(-4, 5, (O, R), generator=g).float() / 8).to(BF)
    return A, B


def merge_cpu(W, A, B, s):
    return (W.float() + s * (B.float() @ A.float())).to(BF)


def run(hip, W, A, B, s, **kw):
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    out, b = hip.lora_merge(d(W), d(A), d(B), s, **{k: d(v) for k, v in kw.items()})
    torch.cuda.synchronize()
    return out.cpu(), None if b is None else b.cpu()


def holder(W, A, B, s, bias=None, bB=None):
    """a Linear of the product package with these tensors as its parameters (on the GPU), for Flux.merged_linear"""
    from visualcloze_amd.model import Linear
    O, I = W.shape
    lin = Linear(I, O, bias=bias is not None)
    lin.add_lora(A.shape[0], float(s))
    assert lin.rank == A.shape[0]
    lin.weight.data, lin.lora_A.weight.data, lin.lora_B.weight.data = W.to(DEV), A.to(DEV), B.to(DEV)
    if bias is not None:
        lin.bias.data = bias.to(DEV)
    lin.lora_B.bias.data = (torch.zeros(O, dtype=A.dtype) if bB is None else bB).to(DEV)
    return lin


# ------------------------------------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("O,I,R", SHAPES + HIGH_RANK)
@pytest.mark.parametrize("s", EXACT_SCALES)
def test_bit_exact_where_the_arithmetic_leaves_no_freedom(hip, O, I, R, s):
    A, B = small_int_factors(O, I, R, 11)
    W = torch.randn(O, I, generator=gen(3)).to(BF)
    out, _ = run(hip, W, A, B, s)
    assert torch.equal(out, merge_cpu(W, A, B, s))


@pytest.mark.parametrize("O,I,R", [(3072, 3072, 256), (64, 3072, 64), (3072, 384, 256)] + RAGGED + HIGH_RANK)
@pytest.mark.parametrize("s", EXACT_SCALES)
def test_bit_exact_f32_weight_and_bias(hip, O, I, R, s):
    A, B = small_int_factors(O, I, R, 12)
    g = gen(4)
    W32 = torch.randn(O, I, generator=g)
    bB = (torch.randint(-4, 5, (O,), generator=g).float() / 8).to(BF)
    for b in (torch.randn(O, generator=g), torch.randn(O, generator=g).to(BF)):
        out, bo = run(hip, W32, A, B, s, bias=b, lora_b_bias=bB)
        assert torch.equal(out, merge_cpu(W32, A, B, s))
        assert torch.equal(bo, (b.float() + s * bB.float()).to(BF))
    _, bo = run(hip, W32, A, B, s, lora_b_bias=bB)              # no base bias: 0 + s * b_B
    assert torch.equal(bo, (0 + s * bB.float()).to(BF))
    _, bo = run(hip, W32, A, B, s, bias=b)                      # no LoRA bias: a conversion
    assert torch.equal(bo, b.to(BF))
    assert run(hip, W32, A, B, s)[1] is None


# ------------------------------------------------------------------------------------------------ 2. + 3. general data
def ulp_bf16(x):
    """2^(floor(log2|x|) - 7) in float64; the smallest bf16 subnormal step for 0 and below the normal range"""
    _, e = torch.frexp(x.double().abs())                       # |x| = m * 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 1).clamp(min=-126) - 7)


def general_inputs(kind, O, I, R):
    if kind == "procedural":
        from tests.procedural import ptensor_torch
        W = ptensor_torch((O, I), 101, q=7, dtype=BF)
        A = ptensor_torch((R, I), 102, q=8, dtype=BF)
        B = ptensor_torch((O, R), 103, q=8, dtype=BF)
    else:
        g = gen(7)
        W, A, B = (torch.randn(sh, generator=g).to(BF) for sh in ((O, I), (R, I), (O, R)))
    return W, A, B


@pytest.mark.parametrize("O,I,R", SHAPES + HIGH_RANK)
@pytest.mark.parametrize("kind", ["procedural", "normal"])
def test_every_element_within_the_bound_of_the_exact_value_and_of_the_torch_merge(hip, kind, O, I, R):
    """E = W + s32 * (B @ A) in float64.  For EVERY element
        |out - E| <= ulp_bf16(out) / 2 + (R + 2) * 2^-24 * (|W| + |s32| * (|B| @ |A|)):
    half a bf16 step for the last rounding plus the forward bound of an f32 sum of R exact products, one multiply and one add, in
    any order.  Asserted for the kernel AND for today's torch merge (a violation then points at the kernel, not at the bound), and
    the two against each other under the sum of their bounds.  Measured on MI355X (share of elements where hip != torch, largest
    |hip - torch| / bound, largest |hip - E| / bound): see DESIGN.md §4."""
    from tests.helpers import parity_log
    from visualcloze_amd.model import Flux
    W, A, B = general_inputs(kind, O, I, R)
    BA = B.double() @ A.double()
    absBA = B.double().abs() @ A.double().abs()
    for s in (1.0, 0.7, -1.3):
        s32 = float(torch.tensor(s, dtype=torch.float32))
        E = W.double() + s32 * BA
        slack = (R + 2) * 2.0 ** -24 * (W.double().abs() + abs(s32) * absBA)
        got, _ = run(hip, W, A, B, s)
        ref, _ = Flux.merged_linear(holder(W, A, B, s))
        ref = ref.cpu()
        bound_h = ulp_bf16(got) / 2 + slack
        bound_t = ulp_bf16(ref) / 2 + slack
        err_h, err_t = (got.double() - E).abs(), (ref.double() - E).abs()
        diff = (got.double() - ref.double()).abs()
        parity_log(f"[lora_merge {kind} {O}x{I} r={R} s={s}] hip != torch in {float((got != ref).double().mean()):.2e} of the elements, "
                   f"max |hip - torch| / bound {float((diff / (bound_h + bound_t)).max()):.3f}, max |hip - E| / bound "
                   f"{float((err_h / bound_h).max()):.3f}, max |torch - E| / bound {float((err_t / bound_t).max()):.3f}")
        assert torch.isfinite(got.float()).all()
        assert int((err_t > bound_t).sum()) == 0            # the bound holds for torch's own merge ...
        assert int((err_h > bound_h).sum()) == 0            # ... and for the kernel, every element
        assert int((diff > bound_h + bound_t).sum()) == 0


# ------------------------------------------------------------------------------------------------ 4. layouts
@pytest.mark.parametrize("O,I,R", [(3072, 3072, 256), (130, 72, 33), (4, 12, 4)])
def test_in_place_equals_out_of_place(hip, O, I, R):
    W, A, B = general_inputs("normal", O, I, R)
    want, _ = run(hip, W, A, B, 0.7)
    Wd = W.to(DEV)
    out, _ = hip.lora_merge(Wd, A.to(DEV), B.to(DEV), 0.7, out=Wd)
    torch.cuda.synchronize()
    assert out.data_ptr() == Wd.data_ptr() and torch.equal(Wd.cpu(), want)


@pytest.mark.parametrize("O,I,R", [(768, 256, 8), (130, 72, 33)])
def test_out_as_a_row_slice_of_a_stacked_matrix_leaves_its_neighbours_alone(hip, O, I, R):
    W, A, B = general_inputs("normal", O, I, R)
    want, _ = run(hip, W, A, B, 1.0)
    stacked = torch.full((O + 10, I), 1.5, dtype=BF, device=DEV)
    hip.lora_merge(W.to(DEV), A.to(DEV), B.to(DEV), 1.0, out=stacked[7:7 + O])
    torch.cuda.synchronize()
    st = stacked.cpu()
    assert torch.equal(st[7:7 + O], want)
    assert bool((st[:7] == 1.5).all()) and bool((st[7 + O:] == 1.5).all())


@pytest.mark.parametrize("O,I,R,pad", [(256, 384, 64, 8), (256, 384, 64, 3), (130, 72, 33, 5), (40, 24, 20, 16)])
@pytest.mark.parametrize("f32", [False, True])
def test_padded_row_strides_on_all_four_matrices(hip, O, I, R, pad, f32):
    """each matrix is a column range of a wider one; the columns beside it hold a sentinel that must survive"""
    W, A, B = general_inputs("normal", O, I, R)
    if f32:
        W = torch.randn(O, I, generator=gen(9))
    want, _ = run(hip, W, A, B, -1.3)

    def wide(t, extra):
        big = torch.full((t.shape[0], t.shape[1] + extra), 2.5, dtype=t.dtype, device=DEV)
        big[:, :t.shape[1]] = t.to(DEV)
        return big, big[:, :t.shape[1]]
    (_, Wv), (_, Av), (_, Bv) = wide(W, pad), wide(A, 2 * pad), wide(B, 3 * pad)
    big_o, Ov = wide(torch.zeros(O, I, dtype=BF), 4 * pad)
    hip.lora_merge(Wv, Av, Bv, -1.3, out=Ov)
    torch.cuda.synchronize()
    assert torch.equal(Ov.cpu(), want) and bool((big_o[:, I:] == 2.5).all())


@pytest.mark.parametrize("O,I", [(3072, 3072), (130, 72), (4, 12)])
def test_rank_zero_is_a_conversion(hip, O, I):
    g = gen(5)
    for W in (torch.randn(O, I, generator=g), torch.randn(O, I, generator=g).to(BF)):
        W[0, 0], W[-1, -1] = -0.0, 0.0
        b = torch.randn(O, generator=g).to(W.dtype)
        out, bo = run(hip, W, None, None, 0.7, bias=b)
        assert torch.equal(out.view(torch.int16), W.to(BF).view(torch.int16)) and torch.equal(bo, b.to(BF))


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_prepare_leaves_the_state_dict_bit_identical(hip, dtype):
    """without `consume` the module's own parameters are never written, bf16 or f32 (the contract
    test_f32_parameters_are_never_merged_in_place pins for the torch path)"""
    from tests.helpers import tiny_model
    m, _ = tiny_model(dtype=dtype)
    if dtype == torch.float32:               # the factors must be bf16 values in bf16 storage for this backend
        for n, p in m.named_parameters():
            if ".lora_" in n:
                p.data = p.data.to(BF)
    m.lora_merge = "hip"
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.prepare()
    m.set_lora_scale(0.5)
    m.prepare()
    torch.cuda.synchronize()
    after = m.state_dict()
    assert set(after) == set(before)
    assert all(after[k].dtype == before[k].dtype and torch.equal(after[k], before[k]) for k in before)


def test_consume_merges_in_place_and_empties_the_holder(hip):
    from visualcloze_amd.model import Flux
    W, A, B = general_inputs("normal", 256, 384, 64)
    g = gen(6)
    b, bB = torch.randn(256, generator=g).to(BF), torch.randn(256, generator=g).to(BF)
    want, want_b = Flux.merged_linear(holder(W, A, B, 0.5, b, bB), backend="hip")
    lin = holder(W, A, B, 0.5, b, bB)
    ptr = lin.weight.data_ptr()
    out, bo = Flux.merged_linear(lin, consume=True, backend="hip")
    torch.cuda.synchronize()
    assert out.data_ptr() == ptr and torch.equal(out, want) and torch.equal(bo, want_b)
    assert all(p.numel() == 0 for p in lin.parameters())


def test_consume_with_nothing_to_merge_hands_the_weight_over(hip):
    from visualcloze_amd.model import Flux, Linear
    lin = Linear(24, 40, bias=True).to(DEV, BF)
    W, b = lin.weight.detach().clone(), lin.bias.detach().clone()
    ptr = lin.weight.data_ptr()
    out, bo = Flux.merged_linear(lin, consume=True, backend="hip")
    torch.cuda.synchronize()
    assert out.data_ptr() == ptr and torch.equal(out, W) and torch.equal(bo, b)
    assert all(p.numel() == 0 for p in lin.parameters())


def test_tensors_on_different_devices_are_refused(hip):
    W, A, B = general_inputs("normal", 40, 24, 20)
    with pytest.raises(hip.VclozeHipError, match="device"):
        hip.lora_merge(W.to(DEV), A, B.to(DEV), 1.0)                     # lora_a left on the CPU
    if torch.cuda.device_count() > 1:
        with pytest.raises(hip.VclozeHipError, match="device"):
            hip.lora_merge(W.to(DEV), A.to("cuda:1"), B.to(DEV), 1.0)


# ------------------------------------------------------------------------------------------------ 5. through the model
def _fwd(model, inp, t, dev=DEV):
    img = torch.cat((inp["x"], inp["cond"]), -1)
    out = model(img.to(dev, BF), img_ids=inp["img_ids"].to(dev), txt=inp["txt"].to(dev, BF), txt_ids=inp["txt_ids"].to(dev),
                timesteps=t.to(dev), y=inp["y"].to(dev, BF), txt_mask=inp["txt_mask"].to(dev), img_mask=inp["img_mask"].to(dev),
                guidance=inp["guidance"].to(dev))
    torch.cuda.synchronize()
    return out.float().cpu()


def test_tiny_model_forward_on_the_hip_merge_vs_golden(hip, golden):
    from tests.helpers import parity_log, rel_l2, tiny_model
    from tests.procedural import tiny_inputs
    inp, t = tiny_inputs(B=1), torch.tensor([0.7])
    m_t, _ = tiny_model()
    base = _fwd(m_t, inp, t)
    m, _ = tiny_model()
    m.lora_merge = "hip"
    got = _fwd(m, inp, t)
    e_gold, e_back = rel_l2(got, torch.tensor(golden["flux_b1"])), rel_l2(got, base)
    parity_log(f"[tiny, lora_merge=hip] Flux.forward vs golden flux_b1 {e_gold:.3e} (torch merge: "
               f"{rel_l2(base, torch.tensor(golden['flux_b1'])):.3e}); hip merge vs torch merge {e_back:.3e}")
    assert e_gold < TOL_GOLDEN
    # the one LoRA knob of the reference: every change re-prepares, and coming back reproduces the first output bit for bit
    m.set_lora_scale(0.5)
    half = _fwd(m, inp, t)
    m.set_lora_scale(1.0)
    again = _fwd(m, inp, t)
    assert not torch.equal(half, got) and torch.equal(again, got)
    m.lora_merge = "blas"
    with pytest.raises(ValueError):
        m.prepare()


def test_rank_clipped_lora_merge_vs_reference_on_the_hip_merge(hip, golden):
    """tests/test_golden_ops_gpu.py::test_rank_clipped_lora_merge_vs_reference's case (in 12, out 4, rank 8 clipped to 4, scale
    0.5) through backend="hip", under that test's check"""
    from tests.procedural import procedural_param
    from tests.test_golden_ops_gpu import bf, check
    from visualcloze_amd.model import Flux, Linear
    lin = Linear(12, 4, bias=True)
    lin.add_lora(8, 0.5)
    assert lin.rank == 4
    keys = [str(k) for k in golden["lora_clip_keys"]]
    shapes = [tuple(int(x) for x in str(s).split(",")) for s in golden["lora_clip_shapes"]]
    lin.load_state_dict({k: procedural_param("lltest." + k, s) for k, s in zip(keys, shapes)})
    w, b = Flux.merged_linear(lin.to(DEV, BF), backend="hip")
    wp = torch.zeros(8, 64, dtype=BF, device=DEV)
    bp = torch.zeros(8, dtype=BF, device=DEV)
    xp = torch.zeros(3, 64, dtype=BF, device=DEV)
    wp[:4, :12], bp[:4], xp[:, :12] = w, b, bf(golden["lora_clip_in"])
    out = hip.linear(xp, wp, bp)
    torch.cuda.synchronize()
    check(out[:, :4], golden["lora_clip_out"])


def test_f32_factors_are_refused_not_rounded(hip):
    from visualcloze_amd.model import Flux
    W, A, B = general_inputs("normal", 40, 24, 20)
    with pytest.raises(hip.VclozeHipError, match='lora_merge="torch"'):
        Flux.merged_linear(holder(W.float(), A.float(), B.float(), 1.0), backend="hip")
    with pytest.raises(hip.VclozeHipError, match='lora_merge="torch"'):
        hip.lora_merge(W.to(DEV), A.float().to(DEV), B.to(DEV), 1.0)


# ------------------------------------------------------------------------------------------------ 6. no vendor GEMM
def test_prepare_on_the_hip_merge_calls_no_matmul(hip, monkeypatch):
    from tests.helpers import tiny_model
    calls = []
    real_mm, real_op = torch.matmul, torch.Tensor.__matmul__
    monkeypatch.setattr(torch, "matmul", lambda *a, **k: (calls.append("matmul"), real_mm(*a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "__matmul__", lambda *a, **k: (calls.append("@"), real_op(*a, **k))[1])
    m, _ = tiny_model()
    m.prepare()
    assert calls, "the probe sees the torch merge's matmuls"
    del calls[:]
    m.lora_merge = "hip"
    m.prepare()
    torch.cuda.synchronize()
    assert calls == []
