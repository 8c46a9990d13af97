"""tests/budget.py on a machine without a GPU: every budget the glue-kernel tests (test_glue_gpu.py) and the hot-path tests
(test_hotpath_gpu.py: GEMM, ln_modulate, QKNorm + RoPE, attention) apply is one that torch's own CPU result - or an f32 emulation
of the kernel's rounding sequence - meets at the same shapes, and one that a subtly wrong result does not meet."""
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


# ================================================================ the hot path: GEMM, block norms, attention
def old_check_passes(got, ref, tol=2e-2):
    """the criterion of check() in tests/test_ops_gpu.py: |err| <= tol * max|ref| and relative L2 <= tol"""
    got, ref = got.double(), ref.double()
    return bool((got - ref).abs().max() <= tol * (ref.abs().max() + 1e-12)) and bool((got - ref).norm() / ref.norm() <= tol)


def rb(x):
    return x.to(torch.bfloat16).float()


def gemm_epilogue(y, epi, res, gate):
    """each epilogue's bf16 sequence on an f32 acc + bias (gemm.hip header), torch f32 ops"""
    t = rb(y)
    if epi == 1:
        return rb(F.gelu(t, approximate="tanh"))
    if epi == 3:
        return rb(F.silu(t))
    if epi == 2:
        g = gate.float() if gate.dim() == 2 else gate.float()[None, :]
        return rb(res.float() + rb(g * t))
    return t


def gemm_sliced(a, w, bias, S, bias_first=True, bias_every_slice=False, drop=None):
    """the f32 product summed as S K-slices of whole 64-wide K-tiles (unequal where nk % S != 0), the bias in front or behind"""
    K = a.shape[1]
    nk = K // 64
    cuts = [64 * (s * nk // S) for s in range(S + 1)]
    acc = torch.zeros(a.shape[0], w.shape[0])
    if bias_first:
        acc = acc + bias.float()
    for s in range(S):
        part = a[:, cuts[s]:cuts[s + 1]].float() @ w[:, cuts[s]:cuts[s + 1]].float().t()
        if bias_every_slice and s > 0:
            part = part + bias.float()
        acc = acc + part
    if not bias_first:
        acc = acc + bias.float()
    return acc


HOT_GEMM_SHAPES = [(1, 8, 64), (37, 64, 128), (129, 200, 192), (257, 264, 320), (37, 200, 1024)]


@pytest.mark.parametrize("kind", ["cancel", "same", "exact"])
@pytest.mark.parametrize("M,N,K", HOT_GEMM_SHAPES)
def test_torch_gemm_meets_budget(M, N, K, kind):
    """torch's f32 matmul + each epilogue's bf16 sequence, the same product summed in 2, 3 and 8 K-slices, bias first and last"""
    a, w, bias, res, gate = B.gemm_inputs(M, N, K, kind)
    for epi in (0, 1, 2, 3, 4):
        ref, mags, f32 = B.gemm_case(a, w, bias, epi, res, gate)
        accs = [a.float() @ w.float().t() + bias.float()]
        for S in (2, 3, 8):
            if K // 64 >= S:
                accs += [gemm_sliced(a, w, bias, S, True), gemm_sliced(a, w, bias, S, False)]
        if epi == 1:      # torch's 0.5 x (1 + tanh u) loses 2^-24 |x| where tanh u ~ -1 (test_torch_activations_meet_budget): torch's alone
            f32 = f32 + 2.0 * B.EPS24 * mags[0][0].abs()
        for i, y in enumerate(accs):
            got = gemm_epilogue(y, epi, res, gate)
            B.assert_within_budget(got, ref, len(mags), mags, f32, what=f"gemm {M}x{N}x{K} {kind} epi {epi} order {i}")
            if kind == "exact" and epi in (0, 4):
                mass = a.double().abs() @ w.double().abs().t() + bias.double().abs()
                assert float(mass.max()) <= 255.0
                assert torch.equal(got.double(), ref)


def test_gemm_budget_rejects_subtle_faults():
    # one product dropped from one output element at K = 256 (the median |a w| of that element: ~0.03 beside |t| ~ 1)
    a, w, bias, res, gate = B.gemm_inputs(37, 64, 256, "cancel")
    ref, mags, f32 = B.gemm_case(a, w, bias, 0)
    acc = a.float() @ w.float().t() + bias.float()
    prod = a[5].float() * w[9].float()
    kk = int(prod.abs().argsort()[128])
    bad = acc.clone()
    bad[5, 9] -= prod[kk]
    B.assert_within_budget(rb(acc), ref, 1, mags, f32)
    assert old_check_passes(rb(bad), ref)
    with pytest.raises(AssertionError):
        B.assert_within_budget(rb(bad), ref, 1, mags, f32)
    # one 64-wide K-tile dropped from one 4-column group at K = 1024 (row 3, columns 8 .. 11, K-tile 5): errors ~ N(0, 1/16)
    a, w, bias, res, gate = B.gemm_inputs(37, 200, 1024, "cancel")
    ref, mags, f32 = B.gemm_case(a, w, bias, 0)
    acc = a.float() @ w.float().t() + bias.float()
    bad = acc.clone()
    bad[3, 8:12] -= a[3, 320:384].float() @ w[8:12, 320:384].float().t()
    with pytest.raises(AssertionError):
        B.assert_within_budget(rb(bad), ref, 1, mags, f32)
    assert not old_check_passes(rb(bad), ref)      # check() catches this one: one of the four errors exceeds 2e-2 max|ref| ~ 0.1
    # the bias added to both slices of a two-way split: every element off by its bias - check() catches that too (relative L2 ~ 0.7)
    bad = gemm_sliced(a, w, bias, 2, True, bias_every_slice=True)
    assert not old_check_passes(rb(bad), ref)
    with pytest.raises(AssertionError):
        B.assert_within_budget(rb(bad), ref, 1, mags, f32)
    # the gate of batch element 0 used for a row of batch element 1 (GATE_RES, rows_per_batch = 20: row 20 is the first of batch 1)
    gates = torch.stack([gate, gate.flip(0)])
    grow = gates[(torch.arange(37) >= 20).long()]
    ref, mags, f32 = B.gemm_case(a, w, bias, 2, res, grow)
    B.assert_within_budget(gemm_epilogue(acc, 2, res, grow), ref, len(mags), mags, f32)
    wrong = grow.clone()
    wrong[20] = gates[0]
    bad = gemm_epilogue(acc, 2, res, wrong)
    with pytest.raises(AssertionError):
        B.assert_within_budget(bad, ref, len(mags), mags, f32)
    # (one row of 37 with another gate: errors of |g0 - g1| |t| ~ 1 - check() catches it on the max criterion)
    assert not old_check_passes(bad, ref)


def ln_modulate_f32(x, shift, scale, cols=None):
    """F.layer_norm + modulate as norm.hip rounds it; cols: the (faulty) number of columns the mean is taken over"""
    xf = x.float()
    D = x.shape[1]
    if cols is None:
        ln = F.layer_norm(xf, (D,), eps=1e-6)
    else:
        mean = xf[:, :cols].mean(-1, keepdim=True)
        ln = (xf - mean) * torch.rsqrt(((xf - mean) ** 2).mean(-1, keepdim=True) + 1e-6)
    return rb(rb(1 + scale.float()) * ln + shift.float())


@pytest.mark.parametrize("D", [8, 256, 3072, 4096])
def test_torch_ln_modulate_meets_budget(D):
    """F.layer_norm + modulate at a DC offset of 16 standard deviations (norm_inputs): the offset test_hotpath_gpu.py holds the
    kernel to is one that plain f32 torch meets; and the mean taken over D - 8 columns does not."""
    for rows in (1, 3, 10):
        x, w, b = B.norm_inputs(rows, D)
        scale = (w.float() - 1.25).to(torch.bfloat16)            # in [-0.75, 0.75): 1 + scale is not a bf16 value
        ref, mags, f32 = B.ln_modulate_case(x, b, scale)
        B.assert_within_budget(ln_modulate_f32(x, b, scale), ref, 1, mags, f32, what=f"ln_modulate D={D} rows={rows}")
        if D >= 256:
            bad = ln_modulate_f32(x, b, scale, cols=D - 8)
            assert old_check_passes(bad, ref)
            with pytest.raises(AssertionError):
                B.assert_within_budget(bad, ref, 1, mags, f32)


def qkn_inputs(L, H, seed=0):
    g = torch.Generator().manual_seed(5 * L + H + seed)
    x = torch.randn(L, 3 * H * 128, generator=g)
    x[L // 2, :128] *= 1e-4                                        # one head row of very small values against the 1e-6 epsilon
    sc = [(1 + 0.1 * torch.randn(128, generator=g)).to(torch.bfloat16) for _ in range(2)]
    return x.to(torch.bfloat16), sc[0], sc[1]


@pytest.mark.parametrize("L,H", [(1, 1), (40, 3), (64, 1), (333, 9)])
def test_qknorm_rope_ref_meets_budget(L, H):
    from tests import ref_ops as R
    qkv, qs, ks = qkn_inputs(L, H)
    rope = B.rope_angles(L)
    qr, kr, _ = R.qknorm_rope_ref(qkv, qs, ks, rope, H)
    x = qkv.reshape(L, 3, H, 128)
    for got, part, sc in ((qr, 0, qs), (kr, 1, ks)):
        ref, mags, f32 = B.qknorm_rope_case(x[:, part], sc, rope)
        B.assert_within_budget(got, ref, len(mags), mags, f32, what=f"qknorm_rope L={L} H={H} part={part}")
    # QKN_QPRE: the rotated value times 128^-0.5 * log2(e), rounded once (the f32 sequence of qknorm_rope8)
    t = x[:, 0].float()
    t = rb(rb(t * torch.rsqrt((t * t).mean(-1, keepdim=True) + 1e-6)) * qs.float()).reshape(L, H, 64, 2)
    co, si = rope[:, None, :, 0], rope[:, None, :, 1]
    c32 = torch.tensor(B.QK_PRESCALE, dtype=torch.float32)
    got = rb(torch.stack([(co * t[..., 0] - si * t[..., 1]) * c32, (si * t[..., 0] + co * t[..., 1]) * c32], -1).reshape(L, H, 128))
    ref, mags, f32 = B.qknorm_rope_case(x[:, 0], qs, rope, prescale=True)
    B.assert_within_budget(got, ref, len(mags), mags, f32, what=f"qknorm_rope prescaled L={L} H={H}")


def test_qknorm_budget_rejects_scale_of_the_other_stream():
    """the second stream's scale (2 bf16 ulps away: 1.6 %) used one row too early at `split`: check() passes it"""
    from tests import ref_ops as R
    L, H, split = 40, 3, 16
    qkv, qs, _ = qkn_inputs(L, H)
    qs2 = (qs.float() * (1 + 2.0 ** -6)).to(torch.bfloat16)
    rope = B.rope_angles(L)
    rows = lambda s: torch.where((torch.arange(L) < s)[:, None, None], qs.float()[None, None], qs2.float()[None, None]).to(torch.bfloat16)  # noqa: E731
    qa, _, _ = R.qknorm_rope_ref(qkv, qs, qs, rope, H)
    qb, _, _ = R.qknorm_rope_ref(qkv, qs2, qs2, rope, H)
    ref, mags, f32 = B.qknorm_rope_case(qkv.reshape(L, 3, H, 128)[:, 0], rows(split), rope)
    B.assert_within_budget(torch.cat([qa[:split], qb[split:]]), ref, len(mags), mags, f32)
    bad = torch.cat([qa[:split - 1], qb[split - 1:]])
    assert old_check_passes(bad, ref)
    with pytest.raises(AssertionError):
        B.assert_within_budget(bad, ref, len(mags), mags, f32)


def attn_emulate(q, k, v, live, qmode, pieces=1, l_fault=None):
    """f32 emulation of the kernels' rounding sequence for one (sample, head): the query scaled and rounded once ("scale"), or
    the scale applied to the f32 logit ("stored"), or none ("prescaled"); P = 2^(s - m) rounded to bf16 for P.V while l adds the
    f32 probabilities; bf16 store.  pieces > 1: the keys cut into that many ranges of whole 64-key tiles, each piece normalised by
    its own l and rounded to f16, combined as merge_fold64 does.  l_fault = (piece, key): that piece's l is off by key's weight."""
    c32 = torch.tensor(B.QK_PRESCALE, dtype=torch.float32)
    qf, kf, vf = q.float(), k.float(), v.float()
    if qmode == "scale":
        s = rb(qf * c32) @ kf.t()
    elif qmode == "stored":
        s = (qf @ kf.t()) * c32
    else:
        s = qf @ kf.t()
    s = s.masked_fill(~live[None, :], -math.inf)
    nkt = -(-k.shape[0] // 64)
    cuts = [64 * (p * nkt // pieces) for p in range(pieces + 1)]
    parts = []
    for p in range(pieces):
        sp = s[:, cuts[p]:cuts[p + 1]]
        m = sp.amax(-1, keepdim=True).clamp_min(-1e30)
        m = (m.to(torch.bfloat16).float() + 0.0)                       # attention64 keeps its reference point bf16-representable
        pe = torch.exp2(sp - m)
        l = pe.sum(-1, keepdim=True)
        if l_fault is not None and l_fault[0] == p:
            l = l + pe[:, l_fault[1] - cuts[p]][:, None]
        parts.append((m, l, rb(pe) @ vf[cuts[p]:cuts[p + 1]]))
    if pieces == 1:
        m, l, o = parts[0]
        return (o / l).to(torch.bfloat16)
    mt = torch.stack([m for m, _, _ in parts]).amax(0)
    acc, wsum = 0.0, 0.0
    for m, l, o in parts:
        wgt = l * torch.exp2(m - mt)
        on = torch.where(l > 0, o / l, torch.zeros_like(o)).to(torch.float16).float()
        acc, wsum = acc + wgt * on, wsum + wgt
    return (acc / wsum).to(torch.bfloat16)


ATTN_CPU_CASES = [(1, None, None), (63, None, None), (64, None, None), (65, None, None), (200, None, None), (333, 301, None),
                  (320, None, (0, 128)), (512, 470, (100, 230))]


@pytest.mark.parametrize("kind", ["normed", "peaked"])
@pytest.mark.parametrize("L,kv_len,gap", ATTN_CPU_CASES)
def test_attention_emulation_meets_budget(L, kv_len, gap, kind):
    q, k, v = B.attn_inputs(L, kind)
    live = B.live_mask(L, kv_len, gap)
    for qmode in ("stored", "scale", "prescaled"):
        ref, mags, f32 = B.attention_case(q, k, v, live, B.attention_route(qmode))
        B.assert_within_budget(attn_emulate(q, k, v, live, qmode), ref, 1, mags, f32, what=f"attention L={L} {kind} q={qmode}")
    L2 = 1000                                                            # 16 key tiles: two and seven key ranges (no masks: attn_plan.hip)
    if L == 200:
        q, k, v = B.attn_inputs(L2, kind)
        live = B.live_mask(L2)
        for pieces in (2, 7):
            ref, mags, f32 = B.attention_case(q, k, v, live, B.attention_route("prescaled", "f16", pieces))
            B.assert_within_budget(attn_emulate(q, k, v, live, "prescaled", pieces), ref, 1, mags, f32, what=f"attention {pieces} pieces {kind}")


@pytest.mark.parametrize("L,kv_len,gap", [(65, 65, None), (333, 301, (40, 100)), (1000, 1000, (100, 230))])
def test_attention_budget_rejects_one_key(L, kv_len, gap):
    """An off-by-one at kv_len, at a kv_gap edge or at a tail-piece boundary moves output (i, d) by w_ij |v_jd - o_id|.  Half of
    V's columns carry a common offset of 4 (outputs ~ 4, which set max|ref| and the L2 norm), the other half are zero-mean.
    L = 65: the faulted key has a quarter of the norm (an even weight of ~ 1.5 % in every row): check() passes every fault, the
    per-element budget none.  L = 333, 1000: a key of even weight (0.3 %, 0.1 %) is inside what the bf16 rounding of P allows in the
    worst case (HALF * 2^-7 sum w |v|), so the keys are left as seeded - heavy in some rows - and the budget rejects every fault.
    check() passes all of those too, except key 300 dropped at L = 333 (heavy enough in one row for its max criterion) and the
    tail piece's l at L = 1000; each outcome is asserted."""
    q, k, v = B.attn_inputs(L + 1, "normed")
    v = torch.cat([v[:, :64].float() + 4.0, v[:, 64:].float()], 1).to(torch.bfloat16)
    live = B.live_mask(L + 1, kv_len, gap)
    route = B.attention_route("scale")
    faults = {"last live key dropped": (kv_len - 1, False), "key kv_len let in": (kv_len, True)}
    if gap is not None:
        faults["key at gap_hi dropped"] = (gap[1], False)
    for name, (j, val) in faults.items():
        kk = k.clone()
        if L == 65:
            kk[j] = (kk[j].float() * 0.25).to(torch.bfloat16)
        ref, mags, f32 = B.attention_case(q, kk, v, live, route)
        B.assert_within_budget(attn_emulate(q, kk, v, live, "scale"), ref, 1, mags, f32)
        wrong = live.clone()
        wrong[j] = val
        bad = attn_emulate(q, kk, v, wrong, "scale")
        assert old_check_passes(bad[live], ref[live]) == ((L, j) != (333, 300)), name
        with pytest.raises(AssertionError):
            B.assert_within_budget(bad[live], ref[live], 1, mags, f32[live], what=name)
    if L == 1000:      # one tail piece's l off by one key's weight (piece 3 of 7, key 500): check() catches this one on its max criterion too
        live = B.live_mask(L + 1, kv_len)
        route = B.attention_route("prescaled", "f16", 7)
        ref, mags, f32 = B.attention_case(q, k, v, live, route)
        B.assert_within_budget(attn_emulate(q, k, v, live, "prescaled", 7), ref, 1, mags, f32)
        bad = attn_emulate(q, k, v, live, "prescaled", 7, l_fault=(3, 500))
        assert not old_check_passes(bad[live], ref[live])
        with pytest.raises(AssertionError):
            B.assert_within_budget(bad[live], ref[live], 1, mags, f32[live])


@pytest.mark.parametrize("L,H", [(65, 2), (333, 1)])
def test_attention_emulation_with_in_kernel_query_norm_meets_budget(L, H):
    """attention64's q_norm route: the reference query is the fp64 value of QKNorm + RoPE times c, its error allowance the budget of
    qknorm_rope_case(prescale=True) (attention_case q_err); the emulation feeds the f32 sequence of qknorm_rope8 to the attention."""
    qkv, qs, _ = qkn_inputs(L, H)
    rope = B.rope_angles(L)
    x = qkv.reshape(L, 3, H, 128)
    t = x[:, 0].float()
    t = rb(rb(t * torch.rsqrt((t * t).mean(-1, keepdim=True) + 1e-6)) * qs.float()).reshape(L, H, 64, 2)
    co, si = rope[:, None, :, 0], rope[:, None, :, 1]
    c32 = torch.tensor(B.QK_PRESCALE, dtype=torch.float32)
    qpre = torch.stack([(co * t[..., 0] - si * t[..., 1]) * c32, (si * t[..., 0] + co * t[..., 1]) * c32], -1).reshape(L, H, 128).to(torch.bfloat16)
    qref, mags, f32 = B.qknorm_rope_case(x[:, 0], qs, rope, prescale=True)
    qerr = B.budget(qref, len(mags), mags, f32)
    live = B.live_mask(L, L - 7, (3, 20))
    for h in range(H):
        k, v = x[:, 1, h], x[:, 2, h]
        ref, m, f = B.attention_case(qref[:, h], k, v, live, B.attention_route("prescaled"), q_err=qerr[:, h])
        B.assert_within_budget(attn_emulate(qpre[:, h], k, v, live, "prescaled"), ref, 1, m, f, what=f"attention q_norm L={L} h={h}")


def test_one_hot_inputs_hold_their_precondition():
    """budget.one_hot_inputs: every live row's stray weight is far below 2^-12, every live key is some live row's partner, and the f32
    emulation returns the partner's V row bit for bit with and without a running max."""
    for L, kv_len, gap in ATTN_CPU_CASES:
        live = B.live_mask(L, kv_len, gap)
        q, k, partner, vf = B.one_hot_inputs(L, live)
        assert B.one_hot_stray_weight(q, k, live, partner) <= 2.0 ** -12
        assert sorted(partner[live].tolist()) == live.nonzero().flatten().tolist()
        v = vf(0)
        for qmode in ("stored", "scale"):
            assert B.bits_equal(attn_emulate(q, k, v, live, qmode)[live], v[partner][live])


# ---------------------------------------------------------------- conv3x3_case
@pytest.mark.parametrize("mode,H,W", [(0, 1, 1), (0, 5, 7), (1, 2, 2), (1, 6, 10), (2, 1, 1), (2, 3, 5)])
@pytest.mark.parametrize("with_res", [False, True])
def test_conv3x3_case_is_the_convolution(mode, H, W, with_res):
    """budget.conv3x3_case: its im2col matrix (F.unfold, fp64) times the weight IS F.conv2d's fp64 value (asserted inside the
    builder), torch's own f32 convolution rounded to bf16 meets the budget, and the convolution with dy and dx
    swapped does not."""
    C, O = 64, 24
    hs, ws = (H // 2, W // 2) if mode == 1 else (2 * H, 2 * W) if mode == 2 else (H, W)
    g = torch.Generator().manual_seed(100 * mode + 10 * H + W)
    x = torch.zeros(hs * ws + 1, C, dtype=torch.bfloat16)
    x[:-1] = torch.randn(hs * ws, C, generator=g).to(torch.bfloat16)
    w, bias = (torch.randn(O, 9 * C, generator=g) * (9 * C) ** -0.5).to(torch.bfloat16), torch.randn(O, generator=g).to(torch.bfloat16)
    res = torch.randn(H * W, O, generator=g).to(torch.bfloat16) if with_res else None
    gate = torch.randn(O, generator=g).to(torch.bfloat16) if with_res else None
    ref, mags, f32 = B.conv3x3_case(x, w, bias, H, W, mode, res, gate)

    def torch_conv(wt):
        img = x[:-1].float().reshape(hs, ws, C).permute(2, 0, 1)[None]
        if mode == 1:
            img = F.interpolate(img, scale_factor=2, mode="nearest")
        if mode == 2:
            img = F.pad(img, (0, 1, 0, 1))
        y = F.conv2d(img, wt.float().reshape(O, 3, 3, C).permute(0, 3, 1, 2), bias.float(), stride=2 if mode == 2 else 1,
                     padding=0 if mode == 2 else 1)[0].permute(1, 2, 0).reshape(H * W, O)
        return gemm_epilogue(y, 2 if with_res else 0, res, gate)
    B.assert_within_budget(torch_conv(w), ref, len(mags), mags, f32, what=f"conv2d mode={mode} {H}x{W}")
    swapped = w.reshape(O, 3, 3, C).transpose(1, 2).reshape(O, 9 * C)
    if (mode, H, W) != (0, 1, 1):                                    # a 1x1 map sees the centre tap alone
        with pytest.raises(AssertionError, match="over budget"):
            B.assert_within_budget(torch_conv(swapped), ref, len(mags), mags, f32)


# ---------------------------------------------------------------- unfused_attention_case
def chain_emulate(q, k, v, scale, bias=None, causal=False, drop_last=False, extra_zero=False, swap=None):
    """The unfused chain in torch: f32 matmul of the bf16 values, every store rounded with .to(bfloat16) - s = bf16(q k^T),
    v_ = bf16(scale * s) [+ bias, rounded again] (budget.softmax_logits: the kernel's own sequence), P = bf16(softmax(v_)),
    O = bf16(P V).  Faults: drop_last (the last key takes no part), extra_zero (one more key with logit 0 and a zero V row: a
    pad column that took part in the softmax), swap = j (V rows j and j + 1 exchanged)."""
    L = q.shape[0]
    s = (q.float() @ k.float().t()).to(torch.bfloat16)
    z = B.softmax_logits(s, scale, bias).float()
    if causal:
        z = z.masked_fill(torch.arange(L).reshape(1, L) > torch.arange(L).reshape(L, 1), -math.inf)
    if drop_last:
        z[:, -1] = -math.inf
    if extra_zero:
        z = torch.cat([z, torch.zeros(L, 1)], dim=1)
    P = torch.softmax(z, dim=-1).to(torch.bfloat16)[:, :L]
    vv = v.float().clone()
    if swap is not None:
        vv[[swap, swap + 1]] = vv[[swap + 1, swap]]
    return (P.float() @ vv).to(torch.bfloat16)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("L,dh", [(35, 64), (77, 64), (256, 128)])
def test_unfused_attention_emulation_meets_budget(L, dh, with_bias, causal):
    """The torch emulation of the chain meets budget.unfused_attention_case at scale = dh^-0.5 (VAE, CLIP) and at scale = 1
    (T5: no rounding of the scaled logit, logits of ~ +-100 with a bf16 ulp of 0.5).  Measured here: worst/budget 0.63 over
    all 24 cases (0.25 .. 0.63)."""
    q, k, v, bias, _ = B.unfused_attention_inputs(L, dh)
    for scale in (dh ** -0.5, 1.0):
        b = bias if with_bias else None
        ref, mags, f32 = B.unfused_attention_case(q, k, v, scale, b, causal)
        got = chain_emulate(q, k, v, scale, b, causal)
        what = f"chain L={L} dh={dh} scale={scale:.4f} bias={with_bias} causal={causal}"
        print(what, "worst/budget", B.worst_ratio(got, ref, 1, mags, f32))
        B.assert_within_budget(got, ref, 1, mags, f32, what=what)


@pytest.mark.parametrize("L,dh", [(35, 64), (77, 64), (256, 128)])
def test_unfused_attention_budget_rejects_four_faults(L, dh):
    """The last key dropped; one extra key with logit 0 (a pad column that took part); V rows j and j + 1 swapped for one j; the
    bias of the next head used for this one: each is outside the budget, at every shape, and the sound emulation inside it."""
    q, k, v, bias, other = B.unfused_attention_inputs(L, dh)
    scale = dh ** -0.5
    ref, mags, f32 = B.unfused_attention_case(q, k, v, scale, bias)
    B.assert_within_budget(chain_emulate(q, k, v, scale, bias), ref, 1, mags, f32)
    for fault in ({"drop_last": True}, {"extra_zero": True}, {"swap": L // 2}):
        with pytest.raises(AssertionError, match="over budget"):
            B.assert_within_budget(chain_emulate(q, k, v, scale, bias, **fault), ref, 1, mags, f32, what=str(fault))
    with pytest.raises(AssertionError, match="over budget"):
        B.assert_within_budget(chain_emulate(q, k, v, scale, other), ref, 1, mags, f32, what="bias of the next head")
    ref, mags, f32 = B.unfused_attention_case(q, k, v, scale)                            # and without a bias
    for fault in ({"drop_last": True}, {"extra_zero": True}, {"swap": L // 2}):
        with pytest.raises(AssertionError, match="over budget"):
            B.assert_within_budget(chain_emulate(q, k, v, scale, **fault), ref, 1, mags, f32, what=str(fault))
