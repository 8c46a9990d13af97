"""Per-element fp64 error budgets for the bf16 kernels: the glue kernels (vae.hip, text.hip, pack.hip, elementwise.hip) and the hot
path of a Flux step (gemm.hip, norm.hip, attention.hip, attention64.hip).

A kernel that stores bf16(f(x)) computed in f32 differs from the fp64 value of f by at most half a bf16 ulp per rounding
point plus whatever its f32 arithmetic adds.  `assert_within_budget` checks exactly that, for EVERY element, against the
element's own magnitude - never against the largest element of the tensor, where an error in the small elements of a row
(another group's statistics, a dropped tail chunk, one product or one key lost) would pass unseen.

    |got - ref64| <= sum over rounding points r of (1/2 + 1/64) * gain_r * ulp_bf16(mag_r)  +  f32_terms  +  floor

  ref64      the fp64 value of the expression in the kernel's header comment.  Roundings whose input is exactly
             reproducible (a scale or a bias applied to the bf16 input) are applied inside ref64 with torch f32/bf16 ops;
             every other rounding is a budgeted rounding point
  mag_r      fp64 magnitude of the intermediate that rounding point r rounds (default |ref64|: the final store)
  gain_r     |d out / d intermediate_r|, 1 unless the entry of `mags` is a (mag, gain) pair
  1/64 ulp   f32 arithmetic between two roundings and the exp2 / rcp intrinsics: relative errors of 2^-22 .. 2^-17,
             far below 2^-15 = 1/64 of the SMALLEST relative size of a bf16 ulp (2^-9 .. 2^-8 is half an ulp)
  f32_terms  f32 reductions and cancelling f32 sums: n_serial * 2^-24 * sum|terms|, propagated to the output by the caller.
             Where the order of a sum is the hardware's or the launch plan's business (the matrix pipe, split-K slices, stream
             pieces, attention's tail pieces) the term is the order-independent (n - 1) * eps * sum|terms|, and for sums the
             matrix pipe accumulates eps = 2^-23 per addition (EPS_MFMA): neither the kernels nor the hardware guides
             establish round-to-nearest for its accumulate, so truncation is allowed for
  floor      absolute slack for results below any bf16 a kernel's f32 intrinsics resolve (denormal products)

The `*_case` functions below build (ref64, mags, f32_terms) for each kernel from its header comment and its code;
tests/test_budget_cpu.py shows that torch's own CPU results (and f32 emulations of the kernels' rounding sequences) meet every
one of them and that a subtly wrong result - a 2-ulp error in one small element, one group's mean moved by 2^-6 std, one
product of a GEMM or one key of an attention row lost - does not.  No constant here was fitted to what a GPU returned.
"""
import math

import torch

HALF = 0.5 + 1.0 / 64.0
EPS24 = 2.0 ** -24
EPS_MFMA = 2.0 ** -23      # one addition of the matrix pipe's f32 accumulate (rounding mode not established: see above)


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


STORE = "store"      # entry of `mags`: the final store, rounded at the LARGEST magnitude the stored value can have


def budget(ref64, roundings=1, mags=None, f32_terms=None, floor=1e-30):
    """An entry of `mags` is a magnitude, a (magnitude, gain) pair, None (= |ref64|) or STORE: the store of a value that earlier
    rounding points have already moved rounds at |ref64| + (everything budgeted before it), not at |ref64| - a value that sits
    half an ulp below a power of two in fp64 is stored from the binade above it as often as not, where the ulp is twice as
    large.  (An intermediate rounding point behind another one gets the same treatment from its case builder.)"""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    mags = list(mags) if mags is not None else []
    assert len(mags) <= roundings
    total = torch.zeros_like(ref64)
    if f32_terms is not None:
        total = total + torch.as_tensor(f32_terms, dtype=torch.float64).abs()
    for r in range(roundings):
        m = mags[r] if r < len(mags) else None
        gain = 1.0
        if isinstance(m, str):
            assert m == STORE and r == roundings - 1
            m = ref64.abs() + total
        elif isinstance(m, tuple):
            m, gain = m
        m = ref64.abs() if m is None else torch.as_tensor(m, dtype=torch.float64).abs()
        total = total + HALF * torch.as_tensor(gain, dtype=torch.float64).abs() * ulp_bf16(m)
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


# ---------------------------------------------------------------- GEMM (gemm.hip)
def _dact(fn, t):
    """|d fn / d t| in fp64 (autograd on the fp64 formula: no hand-written derivative to get wrong)"""
    t = t.detach().clone().requires_grad_(True)
    fn(t).sum().backward()
    return t.grad.abs()


def gemm_case(a, w, bias, epi, res=None, gate=None):
    """a [M, K], w [N, K], bias [N] or None (bf16 values); gate broadcastable to [M, N] (a row per batch element), res [M, N].
    gemm.hip header: t = bf16(acc + b), acc = sum_k a w in f32 on the matrix pipe (the products of two bf16 values are exact
    in f32), then  EPI_BIAS / EPI_QKV  y = t (EPI_QKV only moves the V columns: same value wherever it lands),
    EPI_GELU  y = bf16(gelu_tanh(t)),  EPI_SILU  y = bf16(silu(t)),  EPI_GATE_RES  y = bf16(res + bf16(gate * t)).
    Rounding points:
      t            at |acc + b|; gain |act'(t)| (fp64, autograd) for GELU / SiLU, |gate| for GATE_RES
      gate * t     GATE_RES only, at |gate * t|
      the store    GELU / SiLU / GATE_RES, at |y| + what the points before it can have moved it by (STORE)
    f32_terms: (K + 1) * EPS_MFMA * (sum_k |a w| + |b|), times the same gain: K products and the bias are K + 1 terms, summed
    in an order that depends on the tile family (bias first or last), the MFMA's internal order and the split of K into slices or
    stream pieces - the bound holds for every order, and it does not shrink with |acc + b| when the sum cancels.  The single f32
    operations of the epilogues (gate * t, res + ., the activations' intrinsics) sit inside the 1/64 ulp of their rounding."""
    a64, w64 = a.to(torch.float64), w.to(torch.float64)
    K = a64.shape[1]
    acc = a64 @ w64.t()
    mass = a64.abs() @ w64.abs().t()
    if bias is not None:
        acc = acc + bias.to(torch.float64).reshape(1, -1)
        mass = mass + bias.to(torch.float64).abs().reshape(1, -1)
    t = acc
    f32 = (K + 1) * EPS_MFMA * mass
    t_mag = t.abs() + f32                              # what is rounded is the f32 sum, not acc + b
    if epi in (0, 4):
        return t, [t_mag], f32
    if epi in (1, 3):
        fn = gelu_tanh64 if epi == 1 else silu64
        g = _dact(fn, t)
        return fn(t), [(t_mag, g), STORE], f32 * g
    assert epi == 2
    g64 = gate.to(torch.float64).expand_as(t) if gate.dim() == 2 else gate.to(torch.float64).reshape(1, -1).expand_as(t)
    gt_mag = g64.abs() * (t_mag + HALF * ulp_bf16(t_mag))          # gate times the ROUNDED t
    return res.to(torch.float64) + g64 * t, [(t_mag, g64.abs()), gt_mag, STORE], f32 * g64.abs()


# ---------------------------------------------------------------- conv3x3 (gemm.hip, CONV = true)
def conv3x3_case(x, w, bias, H, W, mode, res=None, gate=None):
    """x [Hs*Ws + 1, C] NHWC map with its zero row, w [O, 9C] with K ordered (dy, dx, c), bias [O], res [H*W, O], gate [O] (bf16
    values); (H, W) is the OUTPUT map.  mode 0: same size; 1: nearest 2x upsampling first; 2: pad (0, 1, 0, 1) + stride 2.
    The convolution is the GEMM's arithmetic with another A loader, so the case is gemm_case over the fp64 im2col matrix -
    built here with F.unfold on the fp64 NCHW map, by no kernel of the project - with K = 9C and epi 0 (bias) or 2 (res + gate * .);
    no constant of its own.  That the matrix spells the convolution is asserted on the spot: ref64 equals F.conv2d's fp64 value
    (weight reordered to [O, C, 3, 3] by a view and a permute) to 1e-12 of the magnitudes summed."""
    import torch.nn.functional as F
    C, O = x.shape[1], w.shape[0]
    hs, ws = (H // 2, W // 2) if mode == 1 else (2 * H, 2 * W) if mode == 2 else (H, W)
    assert x.shape[0] == hs * ws + 1 and w.shape[1] == 9 * C and not bool(x[-1].to(torch.float64).abs().any())
    img = x[:-1].to(torch.float64).reshape(hs, ws, C).permute(2, 0, 1)[None]
    if mode == 1:
        img = F.interpolate(img, scale_factor=2, mode="nearest")
    if mode == 2:
        img, stride, pad = F.pad(img, (0, 1, 0, 1)), 2, 0
    else:
        stride, pad = 1, 1
    col = F.unfold(img, kernel_size=3, padding=pad, stride=stride)[0]                      # [(c, tap), H*W]
    col = col.reshape(C, 9, H * W).permute(2, 1, 0).reshape(H * W, 9 * C)                    # -> [pixel, (tap, c)]
    ref, mags, f32 = gemm_case(col, w, bias, 0 if res is None else 2, res, gate)
    w4 = w.to(torch.float64).reshape(O, 3, 3, C).permute(0, 3, 1, 2)
    conv = F.conv2d(img, w4, None if bias is None else bias.to(torch.float64), stride=stride, padding=pad)
    assert conv.shape == (1, O, H, W), conv.shape
    conv = conv[0].permute(1, 2, 0).reshape(H * W, O)
    mass = col.abs() @ w.to(torch.float64).abs().t() + (0.0 if bias is None else bias.to(torch.float64).abs().reshape(1, -1))
    if res is not None:
        g64 = gate.to(torch.float64).reshape(1, -1)
        conv, mass = res.to(torch.float64) + g64 * conv, res.to(torch.float64).abs() + g64.abs() * mass
    assert bool(((ref - conv).abs() <= 1e-12 * mass).all()), "im2col + GEMM and F.conv2d disagree in fp64"
    return ref, mags, f32


# ---------------------------------------------------------------- unfused attention (vae.py _attn, text.py _heads_attention)
def unfused_attention_case(q, k, v, scale, bias=None, causal=False, pad_to=None):
    """One head of the chain S GEMM -> softmax_rows -> transpose -> P.V GEMM: q, k, v [L, dh] (the bf16 values the GEMMs read),
    bias [L, L] (bf16 values) or None, causal: row i sees the keys j <= i; pad_to: K of the P.V product where the plan pads it
    with zero columns (default L).  The chain stores every intermediate as bf16:
      s = bf16(q.k) over K = dh;  v_ = bf16(scale * s) (no rounding at scale == 1: softmax_logits), then bf16(v_ + bias);
      P = bf16(softmax(v_));  O = bf16(sum_j P_j V_j)
    fp64: softmax(scale * q.k + bias) over the visible keys, times V, no rounding inside.  Budget, derived as attention_case's:
      logit      E_ij = scale * (HALF * ulp(|s_ij| + f32_ij) + f32_ij)    the S GEMM, f32_ij = (dh + 1) * EPS_MFMA * sum|q k|, and its store
                      + HALF * ulp(scale * |s_ij|)                        the scaled logit's store (absent at scale == 1)
                      + HALF * ulp(|scale * s_ij + b_ij|)                 the biased logit's store (with a bias)
                 each ulp taken at the magnitude plus what the roundings before it can have moved it by;
                 a softmax whose logits move by at most E moves by  dP_ij <= P_ij * expm1(E_ij + sum_k P_ik E_ik)  (the first order
                 P_ij * (e_ij - sum_k P_ik e_ik), with expm1 because E reaches ~2e-2 at |s| ~ 100: a bf16 logit of 100 has ulp 0.5)
      softmax    cols * 2^-24 * P_ij, as softmax_case (cols = L: the f32 sum of the row's exponentials)
      P's store  HALF * ulp(P_ij): P is stored normalised, so its binade is known (unlike attention_case's deferred one)
      output     sum_j (dP_ij + softmax_ij + HALF * ulp(P_ij)) |V_jd| + (K + 1) * EPS_MFMA * sum_j P_ij |V_jd| (K = pad_to), then STORE"""
    q64, k64, v64 = q.to(torch.float64), k.to(torch.float64), v.to(torch.float64)
    L, dh = q64.shape
    Kp = L if pad_to is None else pad_to
    s = q64 @ k64.t()
    f32s = (dh + 1) * EPS_MFMA * (q64.abs() @ k64.abs().t())
    s_mag = s.abs() + f32s
    E = abs(scale) * (HALF * ulp_bf16(s_mag) + f32s)
    z_mag = abs(scale) * (s_mag + HALF * ulp_bf16(s_mag))
    z = scale * s
    if scale != 1.0:
        E = E + HALF * ulp_bf16(z_mag)
        z_mag = z_mag + HALF * ulp_bf16(z_mag)
    if bias is not None:
        b64 = bias.to(torch.float64)
        z = z + b64
        E = E + HALF * ulp_bf16(z.abs() + E)
    if causal:
        hidden = torch.arange(L).reshape(1, L) > torch.arange(L).reshape(L, 1)
        z = z.masked_fill(hidden, -math.inf)
        E = E.masked_fill(hidden, 0.0)
    P = torch.softmax(z, dim=-1)
    dP = P * torch.expm1(E + (P * E).sum(-1, keepdim=True)) + L * EPS24 * P
    dP = dP + HALF * ulp_bf16(P + dP)
    va = v64.abs()
    return P @ v64, [STORE], dP @ va + (Kp + 1) * EPS_MFMA * ((P + dP) @ va)


def unfused_attention_inputs(L, dh, seed=0):
    """(q, k, v [L, dh], bias [L, L], other head's bias [L, L]) bf16 on the CPU.  q = 4 * randn (the logits q.k reach ~ +-100 at
    dh = 64), every third row 1/32 of that (a flat softmax row beside the peaked ones); keys 0 and 1 are the same vector and the
    queries 0 and 1 are 2x and 1/2 of it: two rows on which two keys tie, at the row's largest logit.  Every key holds half of a
    common +-1 vector u and query 2 is -u: a row whose logits are all ~ -dh^0.5 / 2 after the dh^-0.5 scale, on which a pad column of
    logit 0 that took part in the softmax outweighs the real keys (on a flat row of 256 keys it weighs 1/257, about the rounding)."""
    g = torch.Generator().manual_seed(4099 * L + dh + seed)
    q, k, v = 4.0 * torch.randn(L, dh, generator=g), torch.randn(L, dh, generator=g), torch.randn(L, dh, generator=g)
    q[1::3] *= 1.0 / 32.0
    u = torch.where(torch.rand(dh, generator=g) < 0.5, -1.0, 1.0)
    k = k + 0.5 * u
    if L > 2:
        k[1] = k[0]
        q[0], q[1], q[2] = 2.0 * k[0], 0.5 * k[0], -u
    bias, other = 2.0 * torch.randn(L, L, generator=g), 2.0 * torch.randn(L, L, generator=g)
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, bias, other))


# ---------------------------------------------------------------- ln_modulate (norm.hip)
def ln_modulate_case(x, shift, scale, eps=1e-6):
    """x [rows, D]; shift, scale [D] or [rows, D] (the row's modulation).  y = bf16(bf16(1 + scale) * LN(x) + shift) (norm.hip
    header).  bf16(1 + scale) is reproducible (one f32 add of a bf16 value, one rounding) and is applied inside the reference
    with torch f32 / bf16 ops; one budgeted rounding, the store.  f32_terms as layernorm_case, none of which scales with y, with
    a = bf16(1 + scale) for the weight and the shift for the bias.  Serial length of the mean and variance sums
    (ln_modulate_kernel: one wave per row, a lane adds the 8 elements of each of its ceil(D / 512) chunks, then wave_sum's 6
    butterfly steps): row_serial(D); the mean's division by D is one more operation."""
    x = x.to(torch.float64)
    a = (1.0 + scale.float()).to(torch.bfloat16).to(torch.float64)
    a = a.reshape(1, -1) if a.dim() == 1 else a
    sh = shift.to(torch.float64)
    sh = sh.reshape(1, -1) if sh.dim() == 1 else sh
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd * a
    n = row_serial(x.shape[1])
    f32 = EPS24 * (4.0 * (xh.abs() + sh.abs()) + (n + 1) * x.abs().mean(-1, keepdim=True) * rstd * a.abs() + (0.5 * n + 2.0) * xh.abs())
    return xh + sh, [STORE], f32.expand_as(xh)


# ---------------------------------------------------------------- QKNorm + RoPE (norm.hip, common.h qknorm_rope8)
QK_PRESCALE = 128 ** -0.5 * 1.4426950408889634      # VC_QK_PRESCALE: 128^-0.5 * log2(e)


def qknorm_rope_case(x, scale, rope, prescale=False, eps=1e-6):
    """x [L, H, 128] (the q or the k columns of the qkv rows), scale [128] or [L, 1, 128] (the row's stream), rope [L, 64, 2] =
    (cos, sin).  common.h qknorm_rope8: rrms = rsq(sum(x^2) / 128 + 1e-6); t = bf16(bf16(x * rrms) * scale); the interleaved
    pairs are rotated, re = cos t0 - sin t1, im = sin t0 + cos t1 (written-out FMAs), and the rotated value times `post` is
    rounded ONCE: post = 1, or 128^-0.5 * log2(e) with QKN_QPRE (and in attention64.hip's in-kernel query norm, which folds the
    scale in the same way).  Rounding points of an output element (re shown; im has cos and sin swapped):
      x0 * rrms    gain |scale0 cos| post        t0 = . * scale0    gain |cos| post
      x1 * rrms    gain |scale1 sin| post        t1 = . * scale1    gain |sin| post
      the store    at |post * re| + what the four points before it can have moved it by (STORE)
    f32_terms, relative to |cos t0| + |sin t1| (NOT to the result: the rotation's two products can cancel), times post:
      2 * 2^-24        the product and the FMA of the rotation
      (12 / 2 + 3)     rrms: a sum of 128 non-negative squares, 8 serial FMAs per lane and 4 butterfly steps over the row's 16
                       lanes, relative error <= 12 * 2^-24, half of it in rrms; the FMA with 1/128 and 1e-6 and the 1-ulp v_rsq"""
    x = x.to(torch.float64)
    L, H, D = x.shape
    g = scale.to(torch.float64)
    g = g.reshape(1, 1, D) if g.dim() == 1 else g
    post = QK_PRESCALE if prescale else 1.0
    rrms = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    xn = x * rrms
    t = (xn * g).reshape(L, H, D // 2, 2)
    xn, gp = xn.reshape(L, H, D // 2, 2), g.expand(L, H, D).reshape(L, H, D // 2, 2)
    co, si = rope.to(torch.float64)[:, None, :, 0], rope.to(torch.float64)[:, None, :, 1]
    t0, t1, x0, x1, g0, g1 = t[..., 0], t[..., 1], xn[..., 0], xn[..., 1], gp[..., 0], gp[..., 1]
    st = lambda re, im: torch.stack([re, im], -1).reshape(L, H, D)  # noqa: E731
    ref = st(co * t0 - si * t1, si * t0 + co * t1) * post
    ca, sa = co.abs() * post, si.abs() * post
    tm0, tm1 = t0.abs() + g0.abs() * HALF * ulp_bf16(x0), t1.abs() + g1.abs() * HALF * ulp_bf16(x1)      # scale times the ROUNDED x * rrms
    mags = [(st(x0, x0), st(g0.abs() * ca, g0.abs() * sa)), (st(tm0, tm0), st(ca.expand_as(t0), sa.expand_as(t0))),
            (st(x1, x1), st(g1.abs() * sa, g1.abs() * ca)), (st(tm1, tm1), st(sa.expand_as(t1), ca.expand_as(t1))), STORE]
    f32 = (2.0 + 12 / 2 + 3.0) * EPS24 * st(ca * t0.abs() + sa * t1.abs(), sa * t0.abs() + ca * t1.abs())
    return ref, mags, f32


# ---------------------------------------------------------------- attention (attention.hip, attention64.hip)
def attention_route(q="stored", partial=None, pieces=0):
    """q        how the kernel treats the query rows it reads:
                  "stored"     attention.hip (variants 0-7): the bf16 rows as they are, the scale c applied to the f32 logit
                  "scale"      attention64.hip after the pre-pass: bf16(c * q), one rounding ("rounded to bf16 once more")
                  "prescaled"  VcAttention.q_prescaled: the rows hold c * q already; the reference takes them as they are (c = 1)
       partial  None, "f32" (attention.hip's tail split: un-normalised f32 pieces) or "f16" (attention64.hip: pieces normalised
                by their own row sums and stored as f16, attn_plan.h PART64_O_BYTES)
       pieces   an upper bound of the number of pieces of one item (0: one per 64-key tile)"""
    assert q in ("stored", "scale", "prescaled") and partial in (None, "f32", "f16")
    return {"q": q, "partial": partial, "pieces": pieces}


def attention_case(q, k, v, live, route, rows=None, chunk=32, q_err=None):
    """One (sample, head): q [Lq, 128], k, v [Lk, 128] (the bf16 values the kernel reads), live [Lk] bool (keys below kv_len and
    outside kv_gap), route = attention_route(...); rows: the query rows to evaluate (default all).  Masked QUERY rows are the
    caller's: they must be exactly 0.  fp64: s = c q.k (log2 domain, c = 128^-0.5 * log2(e), 1 on the prescaled route),
    w = softmax2(s) over the live keys, o = sum_j w_j v_j.  Budget per element (i, d), to first order:
      logit      an error dl_j of logit j moves o by ln2 * w_j * dl_j * (v_j - o):  ln2 * sum_j w_ij dl_ij |v_jd - o_id| with
                   dl_ij = sum_d' HALF * ulp_bf16(c q_id') |k_jd'|                 the query's one rounding after the scale (route
                                                                                  "scale"; absent for "stored" and "prescaled")
                         + 130 * EPS_MFMA * (sum_d' |c q_id' k_jd'| + m_i)        128 products summed by the matrix pipe in its own
                           order, the reference point m (attention64: subtracted by a 9th k-step of the same accumulator;
                           attention.hip: one f32 multiply by c and one subtract) - m_i = (1 + 2^-8) max_j |s_ij| bounds any
                           reference point the online softmax can hold.  The VALUE of m cancels (a softmax is the same function for
                           any reference point, and attention64 keeps m bf16-exact so that what the pipe subtracts is what the row
                           sum and O are scaled by); what does not cancel is that the accumulator's additions are rounded at
                           magnitudes that include m, which is why m_i stands beside the products in this term
                   q_err (optional, [rows, 128], with route "prescaled" and q given in fp64): the queries are not an input but
                   the result of a norm inside the kernel (attention64's q_norm); q is then the fp64 value of that norm
                   (qknorm_rope_case(prescale=True)) and q_err its per-element budget: dl_ij += sum_d' q_err_id' |k_jd'|
      probability P goes to the P.V product as bf16 while the row sum l adds the f32 probabilities: only the numerator is rounded,
                 HALF * 2^-7 * sum_j w_ij |v_jd| - the reference point is deferred (P may sit up to 2^8 above 1), so P's binade is
                 not known and the worst relative size of half an ulp, 2^-8 = 2^-7 / 2, is taken.  The 1/64 in HALF covers v_exp
      sums       (n_live + 64) * EPS_MFMA * sum_j w_ij |v_jd|: the f32 sums of O (matrix pipe) and l over n_live keys, the
                 rescales of the online softmax (at most one per 64-key tile, far fewer), the reciprocal and the final multiply
      tail split "f16": 2^-11 * sum_j w_ij |v_jd| + 2^-25 (half an f16 ulp of every normalised piece, half the f16 subnormal
                 spacing), and for both kinds (4 * pieces + 2) * EPS_MFMA * sum_j w_ij |v_jd| for the merge (per piece one exp2,
                 the weight's multiply and two FMAs; the reciprocal and the final multiply)
      store      one rounding at |o| + everything above (STORE)
    The [rows, Lk, 128] intermediate of the logit term is built `chunk` query rows at a time."""
    dev = q.device
    q64, k64, v64 = q.to(torch.float64), k.to(torch.float64), v.to(torch.float64)
    if rows is not None:
        q64 = q64[rows]
    c = 1.0 if route["q"] == "prescaled" else QK_PRESCALE
    live = live.to(dev)
    n_live = int(live.sum())
    cq = c * q64
    s = (cq @ k64.t()).masked_fill(~live[None, :], -math.inf)
    w = torch.softmax(s * math.log(2.0), dim=-1)
    o = w @ v64
    wv = w @ v64.abs()
    m_i = (1.0 + 2.0 ** -8) * s.masked_fill(~live[None, :], 0.0).abs().amax(-1, keepdim=True)
    dl = 130.0 * EPS_MFMA * (cq.abs() @ k64.abs().t() + m_i)
    if route["q"] == "scale":
        dl = dl + (HALF * ulp_bf16(cq)) @ k64.abs().t()
    if q_err is not None:
        assert route["q"] == "prescaled"
        dl = dl + q_err.to(torch.float64) @ k64.abs().t()
    wdl = w * dl
    logit = torch.empty_like(o)
    for r0 in range(0, q64.shape[0], chunk):
        r1 = min(r0 + chunk, q64.shape[0])
        logit[r0:r1] = torch.einsum("rj,rjd->rd", wdl[r0:r1], (v64[None, :, :] - o[r0:r1, None, :]).abs())
    f32 = math.log(2.0) * logit + (HALF * 2.0 ** -7 + (n_live + 64) * EPS_MFMA) * wv
    if route["partial"] is not None:
        pieces = route["pieces"] or -(-k64.shape[0] // 64)
        f32 = f32 + (4 * pieces + 2) * EPS_MFMA * wv
        if route["partial"] == "f16":
            f32 = f32 + 2.0 ** -11 * wv + 2.0 ** -25
    return o, [STORE], f32


def gemm_inputs(M, N, K, kind, seed=0):
    """(a [M, K], w [N, K], bias [N], res [M, N], gate [N]) bf16 on the CPU.  kind:
      "cancel"  seeded normal a, w scaled by K^-1/2: acc cancels, the f32 term of the budget matters
      "same"    |a|, |w|, |bias|: nothing cancels, the budget is close to one rounding
      "exact"   integer-valued a (0, +-1 .. +-3), w (0, +-1, +-2), bias (-8 .. 8), sparse enough that sum_k |a w| + |b| <= 255 for
                every output (the caller asserts it): every partial sum is an integer below 2^8 in any order, so EPI_BIAS is exact"""
    g = torch.Generator().manual_seed(1000 * seed + M + 7 * N + 13 * K)
    if kind == "exact":
        p = min(0.5, 4.0 / math.sqrt(K))
        rs = lambda *shape: torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
        a = torch.randint(1, 4, (M, K), generator=g).float() * rs(M, K) * (torch.rand(M, K, generator=g) < p)
        w = torch.randint(1, 3, (N, K), generator=g).float() * rs(N, K) * (torch.rand(N, K, generator=g) < p)
        bias = torch.randint(-8, 9, (N,), generator=g).float()
    else:
        a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
        if kind == "same":
            a, w, bias = a.abs(), w.abs(), bias.abs()
    res, gate = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    return tuple(t.to(torch.bfloat16) for t in (a, w, bias, res, gate))


def rope_angles(L, seed=0):
    """[L, 64, 2] f32 (cos, sin): seeded angles, with row 0 at angle 0 (sin = 0), row 1 (if any) at pi / 2 (cos ~ 0: 6e-17 in
    fp64, 4e-8 after the f32 rounding) and row 2 at pi"""
    g = torch.Generator().manual_seed(77 + L + seed)
    ang = torch.rand(L, 64, generator=g, dtype=torch.float64) * 2 * math.pi
    for i, v in enumerate((0.0, math.pi / 2, math.pi)[:L]):
        ang[i] = v
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()


def attn_inputs(L, kind, seed=0):
    """(q, k, v) [L, 128] bf16 on the CPU for one (sample, head).  "normed": |q| = |k| = sqrt(128) as after QKNorm (what the
    bounded form requires); "peaked": normed, and each query is partly aligned with one key through a seeded permutation (q_i =
    normed(0.5 k_perm(i) + noise): logit ~ 6 in the log2 domain above the rest), so a few keys carry most of the weight."""
    g = torch.Generator().manual_seed(31 * L + seed)
    nrm = lambda t: t / t.pow(2).mean(-1, keepdim=True).sqrt()  # noqa: E731
    q, k, v = torch.randn(L, 128, generator=g), nrm(torch.randn(L, 128, generator=g)), torch.randn(L, 128, generator=g)
    if kind == "peaked":
        q = 0.5 * k[torch.randperm(L, generator=g)] + q
    else:
        assert kind == "normed"
    return nrm(q).to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)


def live_mask(L, kv_len=None, gap=None):
    live = torch.ones(L, dtype=torch.bool)
    if kv_len is not None:
        live[kv_len:] = False
    if gap is not None:
        live[gap[0]:gap[1]] = False
    return live


def one_hot_inputs(L, live, seed=0):
    """(q, k [L, 128], partner [L], v(head) -> [L, 128]) bf16 on the CPU: q_i = 4 u_partner(i), k_j = u_j with seeded +-1 vectors u;
    `partner` is a seeded permutation of the live indices (every live key is some live query's partner; a masked query row gets a
    live key too).  The aligned logit is 128 * bf16(4 c) = 65.5 in the log2 domain EXACTLY (4 c = 0.5101 rounds to 131 / 256, and the
    same value comes out of c * 512 in f32), a bf16 value: the running max lands on it and P = 1; without a running max P = 2^65.5,
    whose bf16 rounding is 2^-13 away - in both cases the output row rounds to the partner's V row bit for bit.  Every MASKED key
    gets k = 1.5 u_partner(i) of a seeded live query i (logit 98.25 <= 100, above i's true partner) and V = 64: a leak is a gross
    error.  v(head): magnitudes 1 + n / 128, seeded signs, rows distinct (asserted)."""
    g = torch.Generator().manual_seed(977 * L + seed)
    u = torch.where(torch.rand(L, 128, generator=g) < 0.5, -1.0, 1.0)
    idx = live.nonzero().flatten()
    dead = (~live).nonzero().flatten()
    partner = torch.zeros(L, dtype=torch.long)
    partner[idx] = idx[torch.randperm(len(idx), generator=g)]
    partner[dead] = idx[torch.randint(len(idx), (len(dead),), generator=g)]
    k = u.clone()
    k[dead] = 1.5 * u[partner[idx[torch.randint(len(idx), (len(dead),), generator=g)]]]

    def v(head):
        gv = torch.Generator().manual_seed(977 * L + seed + 31 * (head + 1))
        x = (1.0 + torch.randint(0, 128, (L, 128), generator=gv) / 128.0) * torch.where(torch.rand(L, 128, generator=gv) < 0.5, -1.0, 1.0)
        assert torch.unique(x, dim=0).shape[0] == L
        x[dead] = 64.0
        return x.to(torch.bfloat16)
    return (4.0 * u[partner]).to(torch.bfloat16), k.to(torch.bfloat16), partner, v


def one_hot_stray_weight(q, k, live, partner):
    """fp64: the largest share of a live row's softmax weight that keys other than its partner hold"""
    s = (QK_PRESCALE * q.to(torch.float64)) @ k.to(torch.float64).t()
    s = s.masked_fill(~live.to(s.device)[None, :], -math.inf)
    w = torch.softmax(s * math.log(2.0), dim=-1)
    own = w.gather(1, partner.to(s.device)[:, None])[:, 0]
    return float((1.0 - own)[live.to(s.device)].max())
