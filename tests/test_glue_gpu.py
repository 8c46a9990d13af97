"""The HBM-bound glue kernels (vae.hip, text.hip, pack.hip, the non-solver part of elementwise.hip) against plain fp64
references, element by element, with the budgets of tests/budget.py (each derived from the kernel's header comment and met by
torch's own CPU result in tests/test_budget_cpu.py), or bit for bit where torch's bf16 expression is the same sequence.
Shapes sit on the tile edges and on every threshold between two code paths; output buffers are pre-filled with a sentinel and
everything a kernel must not write is checked to be untouched."""
import pytest
import torch

from oracle import flux_oracle as FO
from tests import budget as B
from tests.helpers import patterned, sentinel, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


# ---------------------------------------------------------------- GroupNorm
GN_SHAPES = [(64, 32), (128, 32), (256, 32), (512, 32), (2048, 32), (128, 64), (8, 1)]
GN_CASES = [(C, G, HW) for C, G in GN_SHAPES for HW in (1, 127, 128, 129)] + [(64, 32, 32769)]
GN_KINDS = {"zero": (0.0, False), "dc4": (4.0, False), "dc16": (16.0, False), "const": (4.0, True)}


@pytest.mark.parametrize("kind", list(GN_KINDS))
@pytest.mark.parametrize("C,G,HW", GN_CASES)
def test_groupnorm_within_budget(hip, C, G, HW, kind):
    """y = bf16(t), t = (x - mean_g) * rstd_g * gamma + beta; swish: bf16(t * sigmoid(t)) on the rounded t (vae.hip header).
    Budget (budget.groupnorm_case): (1/2 + 1/64) ulp(t) for the rounding at t, the same again for the f32 statistics, with
    swish one more at max(|t|, |out|), plus the f32 terms that do not scale with t: 4 * 2^-24 (|xhat gamma| + |beta|) for the
    apply expression and n_serial * 2^-24 * (E|x| rstd |gamma| + E[x^2] rstd^2 |xhat gamma| / 2) for the f32 partial sums of
    128-row blocks (n_serial = budget.gn_serial, 40 at C = 64 .. 1032 at C = 2048; the sums over blocks are fp64, so HW = 32769
    with its 257 partial blocks - a second pass of the finalize loop - adds nothing).  Inputs: zero mean; per-group DC offsets
    of |mean|/std ~ 4 and ~ 16 (16 is the cap: plain f32 F.group_norm meets this budget there, test_budget_cpu.py), different
    in every group; one constant group (var = 0, the output is beta).  gamma, beta differ per channel."""
    ratio, const = GN_KINDS[kind]
    cg = G // 2 if const else None
    x, gamma, beta = B.gn_inputs(HW, C, G, ratio, seed=HW + C, const_group=cg)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    sc = torch.empty(hip.groupnorm_scratch_floats(HW, G), dtype=torch.float32, device=DEV)
    for swish in (False, True):
        y = sentinel((HW, C), float("nan"))
        hip.groupnorm(xd, gd, bd, y, sc, groups=G, swish=swish)
        y2 = sentinel((HW, C), float("nan"))
        hip.groupnorm(xd, gd, bd, y2, sc, groups=G, swish=swish)
        assert torch.equal(y, y2)                                            # deterministic reduction
        ref, mags, f32 = B.groupnorm_case(x, gamma, beta, G, swish)
        what = f"groupnorm C={C} G={G} HW={HW} {kind} swish={swish}"
        print(what, "worst/budget", B.worst_ratio(y, ref, len(mags), mags, f32))
        B.assert_within_budget(y, ref, len(mags), mags, f32, what=what)
        if const and not swish:
            cpg = C // G
            assert B.bits_equal(y[:, cg * cpg:(cg + 1) * cpg], beta[cg * cpg:(cg + 1) * cpg].expand(HW, cpg)), "var = 0: y = beta"


# ---------------------------------------------------------------- softmax_rows
SOFTMAX_COLS = [1, 255, 256, 257, 512, 513, 2048, 2049, 8192, 8193, 16384]


def softmax_rows_input(cols):
    g = torch.Generator().manual_seed(cols)
    x = torch.empty(3, cols)
    x[0] = (torch.linspace(-80.0, 80.0, cols) if cols > 1 else torch.tensor([80.0]))[torch.randperm(cols, generator=g)]
    x[1] = 1.25                                                             # a row of equal values
    x[2] = torch.randn(cols, generator=g) * 3.0                             # one dominant value
    x[2, cols // 2] = 40.0
    bias = torch.randn(3, cols, generator=g)
    return x.to(BF), bias.to(BF)


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows_within_budget(hip, cols):
    """y = bf16(softmax(v)), v = bf16(scale * x) [+ bias, rounded again], f32 internal (vae.hip header).  The scale and bias
    roundings are reproduced exactly inside the reference (budget.softmax_logits); budget: one rounding at the output plus
    cols * 2^-24 * ref for the f32 sum of `cols` positive terms.  cols covers the four template instances (<= 512, <= 2048,
    <= 8192, <= 16384) and both sides of each boundary; ld = cols + 8, the pad columns stay untouched; the bias has its own
    stride."""
    x, bias = softmax_rows_input(cols)
    bbuf = sentinel((3, cols + 24))
    bbuf[:, :cols] = bias.to(DEV)
    for scale, bb in ((1.0, None), (0.3, None), (0.125, bbuf[:, :cols])):
        buf = sentinel((3, cols + 8))
        buf[:, :cols] = x.to(DEV)
        hip.softmax_rows(buf[:, :cols], scale, bias=bb)
        ref, mags, f32 = B.softmax_case(x, scale, None if bb is None else bias)
        what = f"softmax cols={cols} scale={scale} bias={bb is not None}"
        print(what, "worst/budget", B.worst_ratio(buf[:, :cols], ref, 1, mags, f32))
        B.assert_within_budget(buf[:, :cols], ref, 1, mags, f32, what=what)
        assert untouched(buf[:, cols:]), "pad columns written"
    assert untouched(bbuf[:, cols:])


@pytest.mark.parametrize("cols", [77, 80])
def test_softmax_rows_causal(hip, cols):
    """causal_period = 77 over 154 rows: row r sees columns j <= r % 77; everything beyond is exactly 0 (also the columns
    77..79 of a row with cols = 80).  Budget as above, over the visible columns."""
    g = torch.Generator().manual_seed(77 + cols)
    x = (torch.randn(154, cols, generator=g) * 4.0).to(BF)
    buf = sentinel((154, cols + 8))
    buf[:, :cols] = x.to(DEV)
    hip.softmax_rows(buf[:, :cols], 0.125, causal_period=77)
    ref, mags, f32 = B.softmax_case(x, 0.125, None, causal_period=77)
    B.assert_within_budget(buf[:, :cols], ref, 1, mags, f32, what=f"causal softmax cols={cols}")
    got = buf[:, :cols].cpu()
    hidden = torch.arange(cols).reshape(1, cols) > (torch.arange(154) % 77).reshape(154, 1)
    assert hidden.any() and bool((got[hidden].view(torch.int16) == 0).all()), "masked columns must be exactly +0"
    assert untouched(buf[:, cols:])


def test_softmax_rows_refuses_too_many_columns(hip):
    buf = sentinel((1, 16385))
    with pytest.raises(hip.VclozeHipError):
        hip.softmax_rows(buf, 1.0)
    assert untouched(buf)


# ---------------------------------------------------------------- rmsnorm / layernorm
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [8, 504, 512, 520, 4088, 4096])
def test_row_norms_within_budget(hip, D, rows):
    """rmsnorm y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))): two roundings, the inner one at |x rstd| with gain |w|, then the
    store; f32: (n_serial / 2 + 2) * 2^-24 * |ref| for the sum of D squares through rstd.  layernorm y = bf16((x - mean) *
    rstd * w + b): one rounding; f32 terms that do not scale with y: 4 * 2^-24 (|xhat w| + |b|), n_serial * 2^-24 E|x| rstd
    |w| for the mean, (n_serial / 2 + 2) * 2^-24 |xhat w| for rstd (text.hip header; n_serial = budget.row_serial: D/64
    elements per lane, 6 butterfly steps).  D/8 = 63, 64, 65, 511, 512 chunks: the lane tail and the second register slot;
    rows = 5 reaches the second block's 1-row tail.  Row 0 has zero mean, the others a DC offset of 16 std."""
    x, w, b = B.norm_inputs(rows, D)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = sentinel((rows, D), float("nan"))
    hip.rmsnorm(xd, wd, y, 1e-6)
    ref, mags, f32 = B.rmsnorm_case(x, w, 1e-6)
    print(f"rmsnorm D={D} rows={rows} worst/budget", B.worst_ratio(y, ref, 2, mags, f32))
    B.assert_within_budget(y, ref, 2, mags, f32, what=f"rmsnorm D={D} rows={rows}")
    y = sentinel((rows, D), float("nan"))
    hip.layernorm(xd, wd, bd, y, 1e-5)
    ref, mags, f32 = B.layernorm_case(x, w, b, 1e-5)
    print(f"layernorm D={D} rows={rows} worst/budget", B.worst_ratio(y, ref, 1, mags, f32))
    B.assert_within_budget(y, ref, 1, mags, f32, what=f"layernorm D={D} rows={rows}")


@pytest.mark.parametrize("D", [4104, 12])
def test_row_norms_refuse_bad_width(hip, D):
    x, y = sentinel((2, D), 1.0), sentinel((2, D))
    w = sentinel((D,), 1.0)
    with pytest.raises(hip.VclozeHipError):
        hip.rmsnorm(x, w, y, 1e-6)
    with pytest.raises(hip.VclozeHipError):
        hip.layernorm(x, w, w, y, 1e-5)
    assert untouched(y)


# ---------------------------------------------------------------- embedding
@pytest.mark.parametrize("D", [8, 64])
def test_embedding_is_exact(hip, D):
    """out[i] = table[clamp(ids[i], 0, V - 1)]: the table is a column slice (ldt = D + 16 > D), L = 257 spans two blocks at
    D = 8 chunks per row; ids -1, V and V + 5 clamp to rows 0 and V - 1 (the behaviour the kernel has)."""
    V, L = 11, 257
    full = patterned((V, D + 16)).to(DEV)
    table = full[:, 8:8 + D]
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, V, (L,), generator=g, dtype=torch.int32)
    ids[3], ids[100], ids[256] = -1, V, V + 5
    out = sentinel((L, D))
    hip.embedding(ids.to(DEV), table, out)
    assert B.bits_equal(out, table.cpu()[ids.clamp(0, V - 1).long()])


# ---------------------------------------------------------------- mul / add / quick_gelu
def ewise_values(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(n, generator=g) - 0.5) * 24.0
    v[:4] = torch.tensor([0.0, -0.0, 12.0, -12.0])
    return v[torch.randperm(n, generator=g)].to(BF)


@pytest.mark.parametrize("n", [8, 8 * 257])
def test_mul_add_exact_quick_gelu_within_budget(hip, n):
    """mul, add: one f32 operation on two bf16 values and one rounding, torch's own sequence - bit-exact (signed zeros
    included).  quick_gelu y = bf16(x * bf16(sigmoid(bf16(1.702 x)))) (text.hip header): three roundings, at 1.702 x with gain
    |x| sigmoid', at the sigmoid with gain |x|, and the store.  n = 8 * 257: a second block with one live thread."""
    a, b = ewise_values(n, 1), ewise_values(n, 2)
    ad, bd = a.to(DEV), b.to(DEV)
    y = sentinel((n,), float("nan"))
    hip.mul(ad, bd, y)
    assert B.bits_equal(y, a * b)
    y = sentinel((n,), float("nan"))
    hip.add(ad, bd, y)
    assert B.bits_equal(y, a + b)
    y = sentinel((n,), float("nan"))
    hip.quick_gelu(ad, y)
    ref, mags, _ = B.quick_gelu_case(a)
    print(f"quick_gelu n={n} worst/budget", B.worst_ratio(y, ref, 3, mags))
    B.assert_within_budget(y, ref, 3, mags, what=f"quick_gelu n={n}")


def test_elementwise_refuses_n_12(hip):
    a, y = sentinel((12,), 1.0), sentinel((12,))
    for fn in (lambda: hip.mul(a, a, y), lambda: hip.add(a, a, y), lambda: hip.quick_gelu(a, y)):
        with pytest.raises(hip.VclozeHipError):
            fn()
    assert untouched(y)


# ---------------------------------------------------------------- silu, act2d, gate_residual, add3
def act_rows(rows, cols):
    return B.act_values(rows * cols)[:rows * cols].reshape(rows, cols)     # +-0, +-100, +-12, then uniform in [-100, 100]


@pytest.mark.parametrize("n", [1, 255, 257])
def test_silu_within_budget(hip, n):
    """y = bf16(x * sigmoid(x)) (elementwise.hip): one rounding at the output; values in [-100, 100] with +-0."""
    x = B.act_values(n)[:n]
    y = sentinel((n + 8,))
    hip.silu(x.to(DEV), out=y[:n])
    B.assert_within_budget(y[:n], B.silu64(x), what=f"silu n={n}")
    assert untouched(y[n:])


@pytest.mark.parametrize("act", ["gelu", "silu"])
@pytest.mark.parametrize("rows,cols", [(1, 8), (1, 257), (5, 8), (5, 257)])
def test_act2d_within_budget(hip, rows, cols, act):
    """y[m, n] = bf16(act(x[m, n])) on row views, act = GELU(tanh) or SiLU (elementwise.hip): one rounding at the output.
    ldx = cols + 8 and ldy = cols + 16 differ; the pad columns of y stay untouched."""
    x = act_rows(rows, cols)
    xb = sentinel((rows, cols + 8), 3.0)
    xb[:, :cols] = x.to(DEV)
    yb = sentinel((rows, cols + 16))
    hip.act2d(xb[:, :cols], yb[:, :cols], act)
    ref = B.gelu_tanh64(x) if act == "gelu" else B.silu64(x)
    print(f"act2d {act} {rows}x{cols} worst/budget", B.worst_ratio(yb[:, :cols], ref))
    B.assert_within_budget(yb[:, :cols], ref, what=f"act2d {act} {rows}x{cols}")
    assert untouched(yb[:, cols:])


@pytest.mark.parametrize("mode", ["plain", "step", "alias"])
@pytest.mark.parametrize("rows,cols", [(1, 8), (1, 257), (5, 8), (5, 257)])
def test_gate_residual_is_exact(hip, rows, cols, mode):
    """out = bf16(res + bf16(gate * y)): torch's bf16 expression is the same sequence, so ulp_diff == 0.  The three strides
    differ (cols + 8, + 16, + 24) and the pads stay untouched; "step": a device step counter of 2 with gate_step_stride =
    cols + 8 picks the third gate row; "alias": out is res."""
    g = torch.Generator().manual_seed(rows * 100 + cols)
    y, res = (torch.randn(rows, cols, generator=g) * 3.0).to(BF), (torch.randn(rows, cols, generator=g) * 3.0).to(BF)
    gates = torch.randn(3, cols + 8, generator=g).to(BF)
    yb, rb, ob = sentinel((rows, cols + 8), 3.0), sentinel((rows, cols + 16)), sentinel((rows, cols + 24))
    yb[:, :cols], rb[:, :cols] = y.to(DEV), res.to(DEV)
    out = rb[:, :cols] if mode == "alias" else ob[:, :cols]
    if mode == "step":
        step = torch.tensor([2], dtype=torch.int32, device=DEV)
        hip.gate_residual(yb[:, :cols], rb[:, :cols], gates.to(DEV), out, step_ptr=step, gate_step_stride=cols + 8)
        gate = gates[2, :cols]
    else:
        hip.gate_residual(yb[:, :cols], rb[:, :cols], gates.to(DEV), out)
        gate = gates[0, :cols]
    ref = res + gate.reshape(1, cols) * y
    assert int(B.ulp_diff(out, ref).max()) == 0
    assert untouched(rb[:, cols:]) and untouched(ob[:, cols:]) and (mode != "alias" or untouched(ob))


def test_add3_is_exact(hip):
    """y[i] = bf16(bf16(a[i] + b[i % bn]) + c[i % cn]) with bn = D and cn = 2 D over 4 rows: the two broadcasts index
    differently.  torch's bf16 expression is the same sequence: ulp_diff == 0; c = None leaves the first sum."""
    D = 24
    g = torch.Generator().manual_seed(5)
    a, b, c = ((torch.randn(s, generator=g) * 3.0).to(BF) for s in ((4, D), (D,), (2 * D,)))
    y = sentinel((4 * D + 8,))
    hip.add3(a.to(DEV), b.to(DEV), c.to(DEV), out=y[:4 * D])
    ref = ((a + b).reshape(2, 2 * D) + c).reshape(4, D)
    assert int(B.ulp_diff(y[:4 * D].reshape(4, D), ref).max()) == 0 and untouched(y[4 * D:])
    hip.add3(a.to(DEV), b.to(DEV), None, out=y[:4 * D])
    assert int(B.ulp_diff(y[:4 * D].reshape(4, D), a + b).max()) == 0 and untouched(y[4 * D:])


# ---------------------------------------------------------------- sdedit_mix
@pytest.mark.parametrize("n", [1 << 20, 1003])
@pytest.mark.parametrize("s", [0.09, 0.16, 0.33, 0.4, 0.42, 0.58, 0.85, 1.0 / 3.0])
def test_sdedit_mix_is_torch_exact(hip, s, n):
    """x0 = noise * (1 - s) + latent * s on bf16 tensors with s a Python float (visualcloze.py:221): torch multiplies by
    f32(1.0 - s), the subtraction done in double, and by f32(s).  Bit-exact against that expression evaluated by torch on the
    CPU and on the device.  (1.0f - f32(s) is another f32 at s = 0.09, 0.16, 0.33, 0.42, 0.58 - and equal at 0.4, 0.85.)"""
    g = torch.Generator().manual_seed(20)
    noise, latent = torch.randn(n, generator=g).to(BF), torch.randn(n, generator=g).to(BF)
    nd, ld = noise.to(DEV), latent.to(DEV)
    out = sentinel((n + 8,))
    hip.sdedit_mix(nd, ld, s, out=out[:n])
    cpu = noise * (1 - s) + latent * s
    dev = nd * (1 - s) + ld * s
    print(f"sdedit s={s} n={n}: differ from cpu {int((out[:n].cpu() != cpu).sum())}, from device {int((out[:n] != dev).sum())}")
    assert B.bits_equal(dev, cpu)
    assert B.bits_equal(out[:n], cpu)
    assert untouched(out[n:])


# ---------------------------------------------------------------- packers
@pytest.mark.parametrize("C,h,w", [(16, 2, 2), (16, 4, 130), (16, 2, 256), (16, 2, 258), (2, 2, 6), (64, 2, 132)])
def test_pack_unpack_latent_exact(hip, C, h, w):
    """pack_latent / unpack_latent against oracle.flux_oracle, bit for bit, into columns [8, 8 + 4C) of a token buffer with
    ld = 4C + 24: every other column stays untouched.  w/2 = 65, 129, 66 leave a tail tile of 1, 1, 2 tokens in x; w/2 = 128
    is two full tiles.  Every element of the latent is distinct."""
    lat = patterned((C, h, w))
    ntok, ld = (h // 2) * (w // 2), 4 * C + 24
    tok = sentinel((ntok, ld))
    hip.pack_latent(lat.to(DEV), tok, col0=8)
    assert B.bits_equal(tok[:, 8:8 + 4 * C], FO.pack_latent(lat))
    assert untouched(tok[:, :8]) and untouched(tok[:, 8 + 4 * C:])
    back = sentinel((C, h, w), float("nan"))
    hip.unpack_latent(tok, back, col0=8)
    assert B.bits_equal(back, lat) and B.bits_equal(back, FO.unpack_latent(tok[:, 8:8 + 4 * C].cpu(), h, w))


@pytest.mark.parametrize("H,W", [(16, 16), (32, 272), (16, 528)])
def test_pack_mask_exact(hip, H, W):
    """pack_mask against oracle.flux_oracle into columns [64, 320) of rows with ld = 328; W/16 = 17, 33 leave a tail tile of
    one token.  The mask value is distinct for every pixel."""
    mask = patterned((H, W))
    tok = sentinel(((H // 16) * (W // 16), 328))
    hip.pack_mask(mask.to(DEV), tok, col0=64)
    assert B.bits_equal(tok[:, 64:320], FO.pack_mask(mask))
    assert untouched(tok[:, :64]) and untouched(tok[:, 320:])


def test_packers_refuse_bad_arguments(hip):
    """odd h, odd w, C = 66, ld % 8 != 0, col0 % 8 != 0, and a token view that starts 2 elements into its buffer (the token side
    is read and written in 16-byte vectors): refused by all three, nothing written."""
    def lat(C, h, w):
        return sentinel((C, h, w), 1.0)

    def check(fn):
        with pytest.raises(hip.VclozeHipError):
            fn()

    tok = sentinel((64, 88))
    for C, h, w in ((16, 3, 4), (16, 4, 3), (66, 2, 2)):
        t = sentinel(((h // 2) * (w // 2), 4 * C + 24))
        check(lambda: hip.pack_latent(lat(C, h, w), t, col0=8))
        check(lambda: hip.unpack_latent(t, lat(C, h, w), col0=8))
        assert untouched(t)
    l4 = lat(16, 4, 4)
    flat = sentinel((4 * 88 + 8,))
    views = {"ld": (sentinel((4, 84)), 8), "col0": (sentinel((4, 88)), 4), "base": (flat[2:2 + 4 * 88].view(4, 88), 8)}
    for name, (t, col0) in views.items():
        check(lambda: hip.pack_latent(l4, t, col0=col0))
        check(lambda: hip.unpack_latent(t, l4, col0=col0))
        assert untouched(t), name
    assert untouched(l4, 1.0) and untouched(tok)
    m = sentinel((16, 16), 1.0)
    flat = sentinel((328 + 8,))
    for t, col0 in ((sentinel((1, 324)), 64), (sentinel((1, 328)), 60), (flat[2:2 + 328].view(1, 328), 64)):
        check(lambda: hip.pack_mask(m, t, col0=col0))
        assert untouched(t)


# ---------------------------------------------------------------- layout kernels
def test_transpose_is_exact(hip):
    """[R, Cc] -> [Cc, R] for R, Cc in {1, 31, 32, 33, 70}: below, at and above the 32 x 32 tile, and three tiles; the source is
    a row view (lds = Cc + 8), ldd = R + 8 and the pad columns of the destination stay untouched."""
    for R in (1, 31, 32, 33, 70):
        for Cc in (1, 31, 32, 33, 70):
            src = patterned((R, Cc + 8)).to(DEV)
            dst = sentinel((Cc, R + 8))
            hip.transpose(src[:, :Cc], dst[:, :R])
            assert B.bits_equal(dst[:, :R], src[:, :Cc].t()), (R, Cc)
            assert untouched(dst[:, R:]), (R, Cc)


def test_layout_kernels_exact(hip):
    """nchw_to_nhwc: dst = bf16(src / div + add) from an f32 source, bf16(bf16(src / div) + add) from a bf16 source - torch's
    own sequences on the device (f32 scalars) - and exactly 0 in the pad channels 16..63; nhwc_to_nchw back to f32 and to
    bf16.  C = 16, Cp = 64, HW = 257."""
    g = torch.Generator().manual_seed(9)
    z = (torch.randn(16, 1, 257, generator=g) * 2.0).to(DEV)
    for src in (z, z.to(BF)):
        dst = sentinel((257, 64))
        hip.nchw_to_nhwc(src, dst, 0.3611, 0.1159)
        ref = (src / 0.3611 + 0.1159).to(BF).reshape(16, 257).t()
        assert B.bits_equal(dst[:, :16], ref)
        assert bool((dst[:, 16:].cpu().view(torch.int16) == 0).all()), "pad channels must be exactly +0"
        for dt in (torch.float32, BF):
            back = torch.full((16, 1, 257), float("nan"), dtype=dt, device=DEV)
            hip.nhwc_to_nchw(dst, back)
            assert torch.equal(back.reshape(16, 257).t(), dst[:, :16].to(dt))


def test_gaussian_sample(hip):
    """out = scale * ((mean + exp(0.5 * logvar) * noise) - shift) with every intermediate a bf16 tensor (vae.hip header), Z = 16,
    Cp = 64, HW = 257, logvar in [-20, 10].  Against torch's bf16 sequence on the device: at most 1 ulp apart (expf and torch's
    exp may differ in the last f32 bit before a rounding), and every element within the fp64 budget of the five roundings
    (budget.gaussian_case: exp, the product, the sum, the difference, the store; 0.5 * logvar is exact).  Without noise the
    sample is the mean: two roundings, the difference and the store."""
    g = torch.Generator().manual_seed(3)
    Z, Cp, HW, scale, shift = 16, 64, 257, 0.3611, 0.1159
    mom = torch.randn(HW, Cp, generator=g)
    mom[:, Z:2 * Z] = torch.rand(HW, Z, generator=g) * 30.0 - 20.0
    mom = mom.to(BF)
    noise = torch.randn(Z, 1, HW, generator=g).to(BF)
    md, nd = mom.to(DEV), noise.to(DEV)
    mean, logvar = md[:, :Z].t().reshape(Z, 1, HW), md[:, Z:2 * Z].t().reshape(Z, 1, HW)
    out = sentinel((Z, 1, HW), float("nan"))
    hip.gaussian_sample(md, nd, out, scale, shift)
    ref_t = scale * ((mean + torch.exp(0.5 * logvar) * nd) - shift)
    d = B.ulp_diff(out, ref_t)
    print("gaussian_sample: elements 1 ulp from torch:", int((d == 1).sum()), "max", int(d.max()))
    assert int(d.max()) <= 1
    ref, mags, _ = B.gaussian_case(mean.cpu(), logvar.cpu(), noise, scale, shift)
    B.assert_within_budget(out, ref, len(mags), mags, what="gaussian_sample")
    out = sentinel((Z, 1, HW), float("nan"))
    hip.gaussian_sample(md, None, out, scale, shift)
    assert int(B.ulp_diff(out, scale * (mean - shift)).max()) <= 1
    m64 = mean.cpu().double()
    B.assert_within_budget(out, scale * (m64 - shift), 2, [(m64 - shift, torch.full_like(m64, scale))], what="gaussian mean")
