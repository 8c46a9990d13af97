"""tests/budget.py on a machine without a GPU: every budget the glue-kernel tests (test_glue_gpu.py) apply is one that torch's
own CPU result meets at the same shapes, and one that a subtly wrong result does not meet."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import budget as B

GN_SHAPES = [(64, 32), (128, 32), (256, 32), (512, 32), (2048, 32), (128, 64), (8, 1)]
GN_HW = [1, 127, 128, 129]
SOFTMAX_COLS = [1, 255, 256, 257, 512, 513, 2048, 2049, 8192, 8193, 16384]
NORM_D = [8, 504, 512, 520, 4088, 4096]


def test_ulp_and_rounding_helpers():
    assert B.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, 0.0, 2.0 ** -130])).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0, 2.0 ** -133]
    x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 37.0
    assert torch.equal(B.rbf64(x.float()), x.float().to(torch.bfloat16).double())        # one rounding from f32 agrees with torch
    assert B.rbf64(torch.tensor(1.0 + 2.0 ** -8)).item() == 1.0                           # tie to even
    assert B.rbf64(torch.tensor(1.0 + 3 * 2.0 ** -8)).item() == 1.0 + 2.0 ** -6
    a = torch.tensor([1.0, -1.0, 0.0, 1.0], dtype=torch.bfloat16)
    b = torch.tensor([1.0078125, -1.015625, -0.0, -1.0], dtype=torch.bfloat16)
    assert B.ulp_diff(a, b).tolist() == [1, 2, 0, 2 * 0x3F80]
    assert not B.bits_equal(a[2:3], b[2:3]) and B.bits_equal(a, a.clone())


def torch_groupnorm(x, gamma, beta, G, swish):
    """plain f32 F.group_norm, then the bf16 roundings of the reference's bf16 tensors"""
    HW, C = x.shape
    y = F.group_norm(x.float().t().reshape(1, C, HW, 1), G, gamma.float(), beta.float(), eps=1e-6).to(torch.bfloat16)
    if swish:
        y = (y.float() * torch.sigmoid(y.float())).to(torch.bfloat16)
    return y.reshape(C, HW).t()


# The largest |mean|/std of {4, 16} at which plain f32 torch F.group_norm stays inside the budget is 16 (this test passes at
# both), so 16 is the cap test_glue_gpu.py holds the kernel to.
@pytest.mark.parametrize("ratio", [0.0, 4.0, 16.0])
@pytest.mark.parametrize("C,G", GN_SHAPES)
def test_torch_groupnorm_meets_budget(C, G, ratio):
    for HW in GN_HW + ([32769] if C == 64 else []):
        x, gamma, beta = B.gn_inputs(HW, C, G, ratio, seed=HW + C, const_group=G // 2 if ratio == 4.0 else None)
        for swish in (False, True):
            ref, mags, f32 = B.groupnorm_case(x, gamma, beta, G, swish)
            B.assert_within_budget(torch_groupnorm(x, gamma, beta, G, swish), ref, len(mags), mags, f32,
                                   what=f"group_norm C={C} G={G} HW={HW} ratio={ratio} swish={swish}")


def test_groupnorm_budget_rejects_small_errors():
    C, G, HW = 128, 32, 129
    x, gamma, beta = B.gn_inputs(HW, C, G, 4.0, seed=7)
    ref, mags, f32 = B.groupnorm_case(x, gamma, beta, G, False)
    good = torch_groupnorm(x, gamma, beta, G, False)
    B.assert_within_budget(good, ref, len(mags), mags, f32)
    # one small-magnitude element moved by 2 bf16 ulps: invisible to a bound normalised by max|ref|
    i = int(torch.where(ref.abs() > 2.0 ** -6, ref.abs(), torch.full_like(ref, math.inf)).argmin())
    bad = good.clone().flatten()
    moved = bad[i:i + 1].view(torch.int16) + 2
    bad[i:i + 1] = moved.view(torch.bfloat16)
    assert (bad.float() - good.flatten().float()).abs().max().item() < 2e-2 * ref.abs().max().item()
    with pytest.raises(AssertionError):
        B.assert_within_budget(bad.reshape(HW, C), ref, len(mags), mags, f32)
    # one group's mean shifted by 2^-6 std: every xhat of group 5 is off by 2^-6, every t by 2^-6 * gamma
    cpg = C // G
    wrong = ref.clone()
    wrong[:, 5 * cpg:6 * cpg] -= 2.0 ** -6 * gamma.double()[5 * cpg:6 * cpg]
    assert (wrong - ref).abs().max().item() < 2e-2 * ref.abs().max().item()
    with pytest.raises(AssertionError):
        B.assert_within_budget(wrong.to(torch.bfloat16), ref, len(mags), mags, f32)


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_torch_softmax_meets_budget(cols):
    g = torch.Generator().manual_seed(cols)
    x = (torch.randn(5, cols, generator=g) * 3.0)
    x[1] = torch.linspace(-80.0, 80.0, cols) if cols > 1 else 80.0
    x[2] = 1.25
    x[3] = -4.0
    x[3, cols // 2] = 9.0
    x = x.to(torch.bfloat16)
    bias = (torch.randn(5, cols, generator=g)).to(torch.bfloat16)
    for scale, bb in ((1.0, None), (0.3, None), (0.125, bias)):
        ref, mags, f32 = B.softmax_case(x, scale, bb)
        got = torch.softmax(B.softmax_logits(x, scale, bb).float(), dim=-1).to(torch.bfloat16)
        B.assert_within_budget(got, ref, 1, mags, f32, what=f"softmax cols={cols} scale={scale}")
    # a dropped tail element (its probability set to 0) fails unless it is below the floor
    ref, mags, f32 = B.softmax_case(x, 0.3)
    got = torch.softmax(B.softmax_logits(x, 0.3).float(), dim=-1).to(torch.bfloat16)
    got[0, cols - 1] = 0.0
    with pytest.raises(AssertionError):
        B.assert_within_budget(got, ref, 1, mags, f32)


@pytest.mark.parametrize("D", NORM_D)
def test_torch_row_norms_meet_budget(D):
    for rows in (1, 5):
        x, w, b = B.norm_inputs(rows, D)
        ref, mags, f32 = B.layernorm_case(x, w, b, 1e-5)
        got = F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5).to(torch.bfloat16)
        B.assert_within_budget(got, ref, 1, mags, f32, what=f"layer_norm D={D}")
        ref, mags, f32 = B.rmsnorm_case(x, w, 1e-6)
        xf = x.float()                                                  # T5LayerNorm.forward, run on a bf16 tensor
        hs = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).to(torch.bfloat16)
        B.assert_within_budget(w * hs, ref, 2, mags, f32, what=f"t5 rms D={D}")
        if D >= 16:                                                     # a wrong lane tail: the last chunk normalised as zeros
            bad = (w * hs).clone()
            bad[:, -8:] = 0
            with pytest.raises(AssertionError):
                B.assert_within_budget(bad, ref, 2, mags, f32)


def test_torch_activations_meet_budget():
    x = B.act_values(2056)
    B.assert_within_budget(F.silu(x), B.silu64(x), what="silu")
    # torch evaluates 0.5 x (1 + tanh u) in f32: 1 + tanh(u) carries an absolute error of 2^-24 where tanh(u) ~ -1, which the
    # kernel's x * rcp(1 + exp2(.)) form does not have; that term belongs to torch's formulation alone
    B.assert_within_budget(F.gelu(x, approximate="tanh"), B.gelu_tanh64(x), f32_terms=2.0 * B.EPS24 * x.double().abs(), what="gelu")
    xq = x[x.abs() <= 12]
    ref, mags, _ = B.quick_gelu_case(xq)
    got = xq * torch.sigmoid(1.702 * xq)                                # transformers QuickGELUActivation on a bf16 tensor
    B.assert_within_budget(got, ref, 3, mags, what="quick_gelu")


def test_torch_gaussian_sample_meets_budget():
    g = torch.Generator().manual_seed(3)
    mean = torch.randn(16, 257, generator=g).to(torch.bfloat16)
    logvar = (torch.rand(16, 257, generator=g) * 30.0 - 20.0).to(torch.bfloat16)
    noise = torch.randn(16, 257, generator=g).to(torch.bfloat16)
    # torch's bf16 sequence as it runs on the device (f32 scalars; CPU torch rounds the scalar of `- shift` to bf16 instead)
    z = mean + torch.exp(0.5 * logvar) * noise
    zs = (z.float() - torch.tensor(0.1159, dtype=torch.float32)).to(torch.bfloat16)
    got = (zs.float() * torch.tensor(0.3611, dtype=torch.float32)).to(torch.bfloat16)
    ref, mags, _ = B.gaussian_case(mean, logvar, noise, 0.3611, 0.1159)
    B.assert_within_budget(got, ref, len(mags), mags, what="gaussian_sample")
