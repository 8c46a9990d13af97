"""Per-element fp64 error budgets for the bf16 glue kernels (vae.hip, text.hip, pack.hip, elementwise.hip).

A kernel that stores bf16(f(x)) computed in f32 differs from the fp64 value of f by at most half a bf16 ulp per rounding
point plus whatever its f32 arithmetic adds.  `assert_within_budget` checks exactly that, for EVERY element, against the
element's own magnitude - never against the largest element of the tensor, where an error in the small elements of a row
(another group's statistics, a dropped tail chunk) would pass unseen.

    |got - ref64| <= sum over rounding points r of (1/2 + 1/64) * gain_r * ulp_bf16(mag_r)  +  f32_terms  +  floor

  ref64      the fp64 value of the expression in the kernel's header comment.  Roundings whose input is exactly
             reproducible (a scale or a bias applied to the bf16 input) are applied inside ref64 with torch f32/bf16 ops;
             every other rounding is a budgeted rounding point
  mag_r      fp64 magnitude of the intermediate that rounding point r rounds (default |ref64|: the final store)
  gain_r     |d out / d intermediate_r|, 1 unless the entry of `mags` is a (mag, gain) pair
  1/64 ulp   f32 arithmetic between two roundings and the exp2 / rcp intrinsics: relative errors of 2^-22 .. 2^-17,
             far below 2^-15 = 1/64 of the SMALLEST relative size of a bf16 ulp (2^-9 .. 2^-8 is half an ulp)
  f32_terms  f32 reductions and cancelling f32 sums: n_serial * 2^-24 * sum|terms|, propagated to the output by the caller
  floor      absolute slack for results below any bf16 a kernel's f32 intrinsics resolve (denormal products)

The `*_case` functions below build (ref64, mags, f32_terms) for each kernel from its header comment; tests/test_budget_cpu.py
shows that torch's own CPU results meet every one of them and that a 2-ulp error in one small element, or one group's mean
moved by 2^-6 std, does not.  No constant here was fitted to what a GPU returned.
"""
import math

import torch

HALF = 0.5 + 1.0 / 64.0
EPS24 = 2.0 ** -24


def ulp_bf16(m):
    """2^(floor(log2 m) - 7) for fp64 magnitudes m (8 significand bits); the subnormal spacing 2^-133 below 2^-126; 0 at 0."""
    m = torch.as_tensor(m, dtype=torch.float64).abs()
    _, e = torch.frexp(m)                                  # m = f * 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    e = torch.clamp(e.to(torch.float64) - 1.0, min=-126.0)
    return torch.where(m > 0, torch.exp2(e - 7.0), torch.zeros_like(m))


def rbf64(x):
    """fp64 -> nearest bf16 value (ties to even), kept in fp64: one rounding, not fp64 -> f32 -> bf16."""
    x = torch.as_tensor(x, dtype=torch.float64)
    q = ulp_bf16(x)
    q = torch.where(q > 0, q, torch.ones_like(q))
    return torch.round(x / q) * q                          # x / q is exact (q a power of two); round() is half-to-even


def budget(ref64, roundings=1, mags=None, f32_terms=None, floor=1e-30):
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    mags = list(mags) if mags is not None else []
    assert len(mags) <= roundings
    total = torch.zeros_like(ref64)
    for r in range(roundings):
        m = mags[r] if r < len(mags) else None
        gain = 1.0
        if isinstance(m, tuple):
            m, gain = m
        m = ref64.abs() if m is None else torch.as_tensor(m, dtype=torch.float64).abs()
        total = total + HALF * torch.as_tensor(gain, dtype=torch.float64).abs() * ulp_bf16(m)
    if f32_terms is not None:
        total = total + torch.as_tensor(f32_terms, dtype=torch.float64).abs()
    return total + floor


def worst_ratio(got, ref64, roundings=1, mags=None, f32_terms=None, floor=1e-30):
    """max over elements of |got - ref64| / budget (for printing a measurement before asserting)."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    return float(((got - ref64).abs() / budget(ref64, roundings, mags, f32_terms, floor)).max())


def assert_within_budget(got, ref64, roundings=1, mags=None, f32_terms=None, floor=1e-30, what=""):
    """Every element of `got` within its own budget of ref64 (see the module docstring).  Returns the worst ratio."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    bud = budget(ref64, roundings, mags, f32_terms, floor)
    err = (got - ref64).abs()
    ratio = err / bud
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref64.shape))
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements over budget; worst at {idx}: "
                             f"got {got.flatten()[i].item()!r} ref {ref64.flatten()[i].item()!r} |err| {err.flatten()[i].item():.4e} "
                             f"budget {bud.flatten()[i].item():.4e} (x{worst:.3f})")
    return worst


def ulp_diff(got, ref_bf16):
    """Distance in bf16 steps between two bf16 tensors (+0 and -0 coincide), elementwise, int32."""
    def key(t):
        assert t.dtype == torch.bfloat16
        i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(got) - key(ref_bf16)).abs()


def bits_equal(a, b):
    """Same bf16 bit patterns (distinguishes +0 from -0, compares NaN payloads)."""
    return torch.equal(a.detach().cpu().contiguous().view(torch.int16), b.detach().cpu().contiguous().view(torch.int16))


# ---------------------------------------------------------------- GroupNorm (vae.hip)
def gn_serial(HW, C, G):
    """Longest f32 addition chain of gn_partial_kernel (vae.hip: blocks of 128 rows, 256 threads, fixed order): a thread adds the
    min(8, C/G) channels of a group in each of its ceil(rows * (C/8) / 256) chunks, then one thread adds the 256 / (C/8) thread
    sums of each of the group's ceil((C/G) / 8) chunks.  The sums over blocks are fp64 (gn_finalize_kernel)."""
    cpr, cpg = C // 8, C // G
    rows = min(HW, 128)
    return -(-rows * cpr // 256) * min(8, cpg) + -(-cpg // 8) * (256 // cpr)


def groupnorm_case(x, gamma, beta, G, swish, eps=1e-6):
    """x [HW, C], gamma/beta [C] (bf16 values).  y = bf16(t), t = (x - mean_g) * rstd_g * gamma + beta, swish: bf16(t * sigmoid(t))
    with t = bf16(t) first (vae.hip header).  Budget:
      rounding 1   at t (its input carries the statistics' error, so it is budgeted, not applied): ulp(|t|), gain |swish'| <= 1.1
                   is absorbed by the statistics allowance
      rounding 2   swish only: the output store, at max(|t|, |out|)
      statistics   half an ulp of t: the relative error of rstd and the part of the mean's error that scales with t
      f32_terms    what does NOT scale with t (t can cancel to ~0 while xhat*gamma and beta do not):
                   4 * 2^-24 * (|xhat*gamma| + |beta|)             the four f32 operations of the apply expression
                   n_serial * 2^-24 * E_g|x| * rstd * |gamma|      the mean's f32 partial sums (n_serial: gn_serial)
                   n_serial * 2^-24 * E_g[x^2] * rstd^2 / 2 * |xhat*gamma|   the E[x^2] - mean^2 variance through rstd"""
    x = x.to(torch.float64)
    HW, C = x.shape
    cpg = C // G
    xg = x.reshape(HW, G, cpg)
    mean = xg.mean(dim=(0, 2), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(0, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = gamma.to(torch.float64).reshape(1, G, cpg)
    be = beta.to(torch.float64).reshape(1, G, cpg)
    xh = (xg - mean) * rstd * ga
    t = xh + be
    n = gn_serial(HW, C, G)
    f32 = EPS24 * (4.0 * (xh.abs() + be.abs())
                   + n * xg.abs().mean(dim=(0, 2), keepdim=True) * rstd * ga.abs()
                   + n * (xg ** 2).mean(dim=(0, 2), keepdim=True) * rstd * rstd * 0.5 * xh.abs())
    if swish:
        ref = t * torch.sigmoid(t)
        mags = [t, torch.maximum(t.abs(), ref.abs()), t]
    else:
        ref = t
        mags = [t, t]
    shp = (HW, C)
    # the statistics' half ulp is passed as one more "rounding" at t (HALF instead of 1/2: the same 1/64 margin)
    return ref.reshape(shp), [m.reshape(shp) for m in mags], f32.expand_as(t).reshape(shp)


def gn_inputs(HW, C, G, ratio, seed, const_group=None):
    """Seeded N(0,1) values plus a per-group DC offset of |mean|/std ~ ratio * (0.75 .. 1), alternating sign, different in
    every group; `const_group` holds one group constant (var = 0).  gamma in [0.5, 2), beta in +-[0.25, 1.25), per channel."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // G
    x = torch.randn(HW, G, cpg, generator=g, dtype=torch.float64)
    gi = torch.arange(G, dtype=torch.float64)
    off = ratio * (0.75 + 0.25 * (gi + 1) / G) * torch.where(gi % 2 == 0, 1.0, -1.0)
    x = x + off.reshape(1, G, 1)
    if const_group is not None:
        x[:, const_group, :] = 1.5
    c = torch.arange(C, dtype=torch.float64)
    gamma = 0.5 + 1.5 * torch.frac(c * 0.6180339887 + 0.1)
    beta = (0.25 + torch.frac(c * 0.7548776662 + 0.3)) * torch.where(c % 2 == 0, 1.0, -1.0)
    return x.reshape(HW, C).to(torch.bfloat16), gamma.to(torch.bfloat16), beta.to(torch.bfloat16)


# ---------------------------------------------------------------- softmax_rows (vae.hip)
def softmax_logits(x, scale, bias=None):
    """v = bf16(scale * x) (skipped at scale == 1) [+ bias, rounded to bf16 again]: reproducible bit for bit with torch's f32
    multiply / add followed by one bf16 rounding, which is what the kernel does."""
    v = x.float().cpu()
    if scale != 1.0:
        v = (v * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16).float()
    if bias is not None:
        v = (v + bias.float().cpu()).to(torch.bfloat16).float()
    return v.to(torch.float64)


def softmax_case(x, scale, bias=None, causal_period=0):
    """y = bf16(softmax(v)) per row, f32 internal (vae.hip header); v as softmax_logits; causal: columns j > row % period
    are masked (exactly 0).  Budget: one rounding at the output; f32_terms = cols * 2^-24 * ref for the f32 sum of `cols`
    positive terms (every partial sum <= the total, so n_serial <= cols whatever the order)."""
    v = softmax_logits(x, scale, bias)
    rows, cols = v.shape
    if causal_period > 0:
        lim = (torch.arange(rows) % causal_period + 1).reshape(rows, 1)
        v = torch.where(torch.arange(cols).reshape(1, cols) < lim, v, torch.full_like(v, -math.inf))
    ref = torch.softmax(v, dim=-1)
    return ref, None, cols * EPS24 * ref


# ---------------------------------------------------------------- rmsnorm / layernorm (text.hip)
def row_serial(D):
    """rownorm_kernel: one wave per row, a lane adds its D/64 (rounded up to 8) elements, then 6 butterfly steps."""
    return 8 * -(-D // 512) + 6


def rmsnorm_case(x, w, eps):
    """y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))) (text.hip header; T5LayerNorm).  Two roundings: the inner one at |x * rstd|
    with gain |w|, then the store.  f32_terms: mean(x^2) is a sum of D non-negative f32 terms, relative error
    <= n_serial * 2^-24, half of it in rstd; plus 2 * 2^-24 for rstd's own sqrt and divide: all relative to |ref|."""
    x = x.to(torch.float64)
    w = w.to(torch.float64).reshape(1, -1)
    rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    xn = x * rstd
    ref = w * xn
    f32 = EPS24 * (0.5 * row_serial(x.shape[1]) + 2.0) * ref.abs()
    return ref, [(xn, w.expand_as(xn)), ref], f32


def layernorm_case(x, w, b, eps):
    """y = bf16((x - mean) * rstd * w + b), f32 statistics, the variance from a second pass over (x - mean) (text.hip).
    One rounding.  f32_terms, none of which scales with y (y can cancel to ~0):
      4 * 2^-24 * (|xhat*w| + |b|)                   the four f32 operations of the expression
      n_serial * 2^-24 * E|x| * rstd * |w|           the mean's f32 sum
      (n_serial / 2 + 2) * 2^-24 * |xhat*w|          rstd: a sum of D non-negative squares, sqrt, divide"""
    x = x.to(torch.float64)
    w = w.to(torch.float64).reshape(1, -1)
    b = b.to(torch.float64).reshape(1, -1)
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd * w
    n = row_serial(x.shape[1])
    f32 = EPS24 * (4.0 * (xh.abs() + b.abs()) + n * x.abs().mean(-1, keepdim=True) * rstd * w.abs() + (0.5 * n + 2.0) * xh.abs())
    return xh + b, None, f32


# ---------------------------------------------------------------- activations
def silu64(x):
    x = x.to(torch.float64)
    return x * torch.sigmoid(x)


def gelu_tanh64(x):
    """0.5 x (1 + tanh(u)) = x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): the second form keeps its digits for u << 0."""
    x = x.to(torch.float64)
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x * torch.sigmoid(2.0 * u)


def quick_gelu_case(x):
    """y = bf16(x * bf16(sigmoid(bf16(1.702 * x)))) (text.hip header): three roundings - at 1.702 x with gain |x| * sigmoid',
    at the sigmoid with gain |x|, and the store."""
    x = x.to(torch.float64)
    a = 1.702 * x
    sg = torch.sigmoid(a)
    ref = x * sg
    return ref, [(a, x.abs() * sg * (1.0 - sg)), (sg, x.abs()), ref], None


def gaussian_case(mean, logvar, noise, scale, shift):
    """out = bf16(scale * bf16(bf16(mean + bf16(bf16(exp(bf16(0.5 * logvar))) * noise)) - shift)) (vae.hip header).  0.5 * logvar
    is exact in bf16; the other five roundings: sd = exp(.) (gain |noise| * scale), sd * noise, the sum, the difference
    (gain scale each) and the store."""
    mean, logvar, noise = (t.to(torch.float64) for t in (mean, logvar, noise))
    sd = torch.exp(0.5 * logvar)
    sn = sd * noise
    z = mean + sn
    zs = z - shift
    ref = scale * zs
    s = torch.full_like(ref, abs(scale))
    return ref, [(sd, noise.abs() * s), (sn, s), (z, s), (zs, s), ref], None


# ---------------------------------------------------------------- shared seeded inputs
def norm_inputs(rows, D):
    g = torch.Generator().manual_seed(D + rows)
    x = torch.randn(rows, D, generator=g) + 16.0 * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0).reshape(rows, 1)
    x[0] -= 16.0                                                       # row 0 has zero mean, the others a DC offset of 16 std
    c = torch.arange(D, dtype=torch.float64)
    w = (0.5 + 1.5 * torch.frac(c * 0.6180339887 + 0.1)).to(torch.bfloat16)
    b = ((0.25 + torch.frac(c * 0.7548776662 + 0.3)) * torch.where(c % 2 == 0, 1.0, -1.0)).to(torch.bfloat16)
    return x.to(torch.bfloat16), w, b


def act_values(n):
    g = torch.Generator().manual_seed(n)
    u, z = (torch.rand(max(n, 6), generator=g) - 0.5) * 200.0, torch.randn(max(n, 6), generator=g) * 3.0
    v = torch.cat([torch.tensor([0.0, -0.0, 100.0, -100.0, 12.0, -12.0]), torch.stack([u, z], dim=1).flatten()])
    return v.to(torch.bfloat16)                                        # +-0 and the extremes first, then wide and narrow values in turn
