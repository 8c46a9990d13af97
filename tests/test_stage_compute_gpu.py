"""The compute path of the VAE and of the T5 / CLIP encoders, element by element against fp64: the implicit-GEMM 3x3 convolution
(vc_conv3x3, CONV = true in gemm.hip) against F.conv2d, the batched per-head products (VcGemmArgs.batch) and the unfused attention
chains (vae.py _HipExec._attn, text.py _Exec._heads_attention) against fp64 softmax attention, with the budgets of tests/budget.py
(conv3x3_case, gemm_case, unfused_attention_case: each met by a torch emulation and missed by subtly wrong results in
tests/test_budget_cpu.py).  Outputs are column slices of wider sentinel buffers, NaN-filled; the pads must stay untouched."""
import math

import pytest
import torch

from tests import budget as B
from tests.helpers import sentinel, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


# ---------------------------------------------------------------- conv3x3 against a convolution
# (H, W) is the output map; the M-tile is 256 rows, BN = 128 for O <= 128 and 192 otherwise, BK = 64
CONV_SHAPES = [
    (0, 1, 1),       # eight of nine taps read the zero row
    (0, 257, 1),     # W = 1: every dx != 1 tap is out of the image; two M-tiles
    (0, 1, 264),     # H = 1; the tile boundary falls inside the only row
    (0, 16, 16),     # exactly one tile
    (0, 15, 17),     # M = 255
    (0, 13, 20),     # M = 260: four live rows in the last tile; boundary mid-row
    (1, 2, 2),       # 1x1 source
    (1, 18, 30),     # 9x15 source, M = 540, three tiles
    (2, 1, 1),       # 2x2 source; the pad row and column
    (2, 16, 17),     # 32x34 source, M = 272
    (2, 9, 29),      # M = 261, odd W
]
CONV_CO = [(64, 8), (64, 128), (64, 136), (64, 200), (512, 192), (512, 512)]


def src_shape(mode, H, W):
    return (H // 2, W // 2) if mode == 1 else (2 * H, 2 * W) if mode == 2 else (H, W)


def conv_call(hip, x, w, b, out, H, W, mode, res=None, gate=None):
    hip.conv3x3(x, w, b, out, H, W, up=mode == 1, down=mode == 2, res=res, gate=gate)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C,O", CONV_CO)
@pytest.mark.parametrize("mode,H,W", CONV_SHAPES)
def test_conv3x3_within_budget_of_conv2d(hip, mode, H, W, C, O):
    """out = bf16(conv + bias), or bf16(res + bf16(gate * bf16(conv + bias))), against F.conv2d in fp64 on the NCHW view of the
    bf16 inputs (mode 1: nearest 2x first; mode 2: pad (0, 1, 0, 1), stride 2), every element within budget.conv3x3_case =
    gemm_case over the fp64 im2col matrix with K = 9C.  x, w randn (w scaled by (9C)^-1/2), bias, res and the per-channel gate
    random; out has ldc = O + 8 and res ldres = O + 16 inside 7.0-filled buffers whose pads must stay untouched; out starts as
    NaN; two runs give the same bits.  All 11 shapes x 6 (C, O) x {plain, res}: nothing dropped."""
    hs, ws = src_shape(mode, H, W)
    M = H * W
    g = torch.Generator().manual_seed(100003 * mode + 1009 * H + 13 * W + C + O)
    x = torch.zeros(hs * ws + 1, C, dtype=BF)
    x[:-1] = torch.randn(hs * ws, C, generator=g).to(BF)
    w = (torch.randn(O, 9 * C, generator=g) * (9 * C) ** -0.5).to(BF)
    b, gate, res = torch.randn(O, generator=g).to(BF), torch.randn(O, generator=g).to(BF), torch.randn(M, O, generator=g).to(BF)
    xd, wd, bd, gd = x.to(DEV), w.to(DEV), b.to(DEV), gate.to(DEV)
    rbuf = sentinel((M, O + 16))
    rbuf[:, :O] = res.to(DEV)
    for with_res in (False, True):
        outs = []
        for _ in range(2):
            obuf = sentinel((M, O + 8))
            obuf[:, :O] = float("nan")
            conv_call(hip, xd, wd, bd, obuf[:, :O], H, W, mode, rbuf[:, :O] if with_res else None, gd if with_res else None)
            assert untouched(obuf[:, O:]), "pad columns of out written"
            outs.append(obuf[:, :O].cpu())
        assert B.bits_equal(outs[0], outs[1]), "two runs differ"
        ref, mags, f32 = B.conv3x3_case(x, w, b, H, W, mode, res if with_res else None, gate if with_res else None)
        what = f"conv3x3 mode={mode} {H}x{W} C={C} O={O} res={with_res}"
        print(what, "worst/budget", B.worst_ratio(outs[0], ref, len(mags), mags, f32))
        B.assert_within_budget(outs[0], ref, len(mags), mags, f32, what=what)
    assert untouched(rbuf[:, O:]) and B.bits_equal(rbuf[:, :O], res), "res written"
    assert not bool(xd[-1].any()), "zero row written"


def impulse_weight(O, C, mode):
    """[O, 9, C] bf16.  Modes 0 and 2 (one tap reaches an output pixel): element i holds the bit pattern 0x0080 + i mod 32512 -
    every normal positive bf16 in turn, distinct over any 32512 consecutive elements (56 output channels: all taps and channels
    of a row, and rows less than 56 apart).  Mode 1 (the 2x2 pixels of an upsampled impulse are reached by up to four taps, which
    the kernel adds): +-2^tap * 2^((o + 3c) % 97 - 48), so that the sum over any set of taps is exact in f32 and in bf16 (the
    taps of one output pixel span at most 5 bits) and names the set."""
    if mode != 1:
        i = torch.arange(O * 9 * C, dtype=torch.int32)
        return (0x0080 + i % 32512).to(torch.int16).view(BF).reshape(O, 9, C)
    o, t, c = torch.arange(O).reshape(O, 1, 1), torch.arange(9).reshape(1, 9, 1), torch.arange(C).reshape(1, 1, C)
    sign = torch.where((o + c) % 2 == 0, 1.0, -1.0)
    return (sign * torch.exp2((t + (o + 3 * c) % 97 - 48).double())).to(BF)


def impulse_expected(w3, H, W, mode, sy, sx, c0):
    """[H*W, O] fp64 from index arithmetic alone: output pixel (y, x) holds the sum of w[o, tap, c0] over the taps (dy, dx) whose
    source pixel is the impulse (sy, sx); the number of such taps per pixel is returned beside it."""
    O = w3.shape[0]
    exp, hits = torch.zeros(H * W, O, dtype=torch.float64), torch.zeros(H * W, dtype=torch.int64)
    for y in range(H):
        for x in range(W):
            for dy in range(3):
                for dx in range(3):
                    if mode == 2:
                        yy, xx = 2 * y + dy, 2 * x + dx                 # pad (0, 1, 0, 1): rows 2H and columns 2W are zero
                        ok = yy < 2 * H and xx < 2 * W
                    else:
                        yy, xx = y + dy - 1, x + dx - 1
                        ok = 0 <= yy < H and 0 <= xx < W
                        if mode == 1:
                            yy, xx = yy // 2, xx // 2
                    if ok and (yy, xx) == (sy, sx):
                        exp[y * W + x] += w3[:, dy * 3 + dx, c0].double()
                        hits[y * W + x] += 1
    return exp, hits


@pytest.mark.parametrize("c0", [0, 63])
@pytest.mark.parametrize("mode,H,W", [(0, 13, 20), (0, 18, 30), (0, 16, 17), (1, 18, 30), (2, 13, 20), (2, 18, 30), (2, 16, 17)])
def test_conv3x3_impulse_pins_the_gather_geometry(hip, mode, H, W, c0):
    """x is zero but for channel c0 of one pixel, which is 1.0; bias zero, no res: output pixel (y, x), channel o holds exactly
    w[o, tap, c0] for the tap that reaches the impulse and exactly +0 everywhere else - expected values from index arithmetic in
    this test, compared bit for bit.  A dy / dx swap, a wrong row or column of the gather, the channel order under the LDS swizzle
    or a tap read from the wrong side of the 255 / 256 tile boundary all move a value.  The impulse sits at the four corners of
    the source map and at flat source indices 255 and 256 (mode 1, whose 9x15 source has no such index: the source pixels of
    output pixels 255 and 256).  Mode 1 needs even H and W (odd ones are refused: see the refusals test), so of the three maps
    it runs at 18x30 only, and its weights are the exact-sum family of impulse_weight."""
    C, O = 64, 136
    hs, ws = src_shape(mode, H, W)
    w3 = impulse_weight(O, C, mode)
    wd, bd = w3.reshape(O, 9 * C).contiguous().to(DEV), torch.zeros(O, dtype=BF, device=DEV)
    if mode == 1:
        flat = [(255 // W // 2) * ws + (255 % W) // 2, (256 // W // 2) * ws + (256 % W) // 2]
    else:
        flat = [255, 256]
    spots = [0, ws - 1, (hs - 1) * ws, hs * ws - 1] + [f for f in flat if f < hs * ws]
    assert len(spots) == 6
    for s in spots:
        sy, sx = divmod(s, ws)
        x = torch.zeros(hs * ws + 1, C, dtype=BF, device=DEV)
        x[s, c0] = 1.0
        obuf = sentinel((H * W, O + 8))
        obuf[:, :O] = float("nan")
        conv_call(hip, x, wd, bd, obuf[:, :O], H, W, mode)
        exp, hits = impulse_expected(w3, H, W, mode, sy, sx, c0)
        assert int(hits.max()) == (4 if mode == 1 else 1) and int((hits > 0).sum()) >= (9 if mode == 1 else 1)
        assert torch.equal(exp.to(BF).double(), exp), "expected values are bf16 values"
        got = obuf[:, :O].cpu()
        bad = (got.view(torch.int16) != exp.to(BF).view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"mode={mode} {H}x{W} impulse ({sy},{sx}) c0={c0}: {bad.shape[0]} wrong, first (pixel, o) = {bad[0].tolist()}"
        assert untouched(obuf[:, O:])


def test_conv3x3_refusals_leave_out_untouched(hip):
    """C = 32, O = 12, mode 1 with an odd H, res without gate and ldc < O are refused, and nothing is written."""
    def operands(H, W, C, O, mode):
        hs, ws = src_shape(mode, H, W)
        return (torch.zeros(hs * ws + 1, C, dtype=BF, device=DEV), torch.zeros(O, 9 * C, dtype=BF, device=DEV),
                torch.zeros(O, dtype=BF, device=DEV), sentinel((H * W + 8, max(O, 16) + 8)))
    for H, W, C, O, mode in [(4, 4, 32, 16, 0), (4, 4, 64, 12, 0), (3, 4, 64, 16, 1)]:
        x, w, b, obuf = operands(H, W, C, O, mode)
        with pytest.raises(hip.VclozeHipError):
            conv_call(hip, x, w, b, obuf[:H * W, :O], H, W, mode)
        assert untouched(obuf)
    x, w, b, obuf = operands(4, 4, 64, 16, 0)
    res = torch.zeros(16, 16, dtype=BF, device=DEV)
    with pytest.raises(hip.VclozeHipError):
        conv_call(hip, x, w, b, obuf[:16, :16], 4, 4, 0, res=res, gate=None)
    with pytest.raises(hip.VclozeHipError):                                  # the C entry point itself: a res and a null gate
        hip._check(hip.lib().vc_conv3x3(x.data_ptr(), w.data_ptr(), b.data_ptr(), obuf.data_ptr(), obuf.stride(0), res.data_ptr(), 16,
                                        None, 4, 4, 64, 16, 0, hip.cur_stream()), "vc_conv3x3")
    with pytest.raises(hip.VclozeHipError):                                  # ldc = 8 < O = 16 (rows overlap inside the buffer)
        conv_call(hip, x, w, b, obuf.view(-1).as_strided((16, 16), (8, 1)), 4, 4, 0)
    torch.cuda.synchronize()
    assert untouched(obuf)


# ---------------------------------------------------------------- the batched per-head products
HEAD_SHAPES = [(8, 1, 64), (72, 3, 64), (136, 2, 128), (264, 2, 64)]    # one row-tile; N = 72; two tiles + 8 rows; three


@pytest.mark.parametrize("L,H,dh", HEAD_SHAPES)
def test_gemm_batched_head_products_within_budget(hip, L, H, dh):
    """VcGemmArgs.batch = H as _heads_attention uses it.  S_h = Q_h K_h^T (K = dh): instance h reads its dh columns of q and k and
    writes slab h of [H*L, L]; O_h = P_h V_h^T (K = L, padded with zero columns to a multiple of 64: the GEMM's K-tile): instance
    h writes its dh columns of [L, H*dh].  Every element within budget.gemm_case of ITS head's operands - a slab or a column range
    that took another head's operand, or none (the outputs start as NaN), fails."""
    Lp = (L + 63) // 64 * 64
    g = torch.Generator().manual_seed(L + H + dh)
    q, k, v = (torch.randn(L, H * dh, generator=g).to(BF) for _ in range(3))
    s = torch.full((H * L, L), float("nan"), dtype=BF, device=DEV)
    qd, kd = q.to(DEV), k.to(DEV)
    p = hip.make_problem(qd[:, :dh], kd[:, :dh], None, s[:L])
    p.a_zstride, p.w_zstride, p.c_zstride = dh, dh, L * s.stride(0)
    hip.gemm(p, batch=H)
    torch.cuda.synchronize()
    worst = 0.0
    for h in range(H):
        ref, mags, f32 = B.gemm_case(q[:, h * dh:(h + 1) * dh], k[:, h * dh:(h + 1) * dh], None, 0)
        worst = max(worst, B.assert_within_budget(s[h * L:(h + 1) * L], ref, len(mags), mags, f32, what=f"S L={L} H={H} dh={dh} head {h}"))
    print(f"batched S L={L} H={H} dh={dh} worst/budget", worst)
    pm = torch.zeros(H * L, Lp, dtype=BF)
    pm[:, :L] = torch.softmax(torch.randn(H * L, L, generator=g) * 3.0, dim=-1).to(BF)
    vt = torch.zeros(H * dh, Lp, dtype=BF)
    vt[:, :L] = v.reshape(L, H, dh).permute(1, 2, 0).reshape(H * dh, L)
    o = torch.full((L, H * dh), float("nan"), dtype=BF, device=DEV)
    pd, vd = pm.to(DEV), vt.to(DEV)
    p = hip.make_problem(pd[:L], vd[:dh], None, o[:, :dh])
    p.a_zstride, p.w_zstride, p.c_zstride = L * pd.stride(0), dh * vd.stride(0), dh
    hip.gemm(p, batch=H)
    torch.cuda.synchronize()
    worst = 0.0
    for h in range(H):
        ref, mags, f32 = B.gemm_case(pm[h * L:(h + 1) * L], vt[h * dh:(h + 1) * dh], None, 0)
        worst = max(worst, B.assert_within_budget(o[:, h * dh:(h + 1) * dh], ref, len(mags), mags, f32, what=f"PV L={L} H={H} dh={dh} head {h}"))
    print(f"batched PV L={L} H={H} dh={dh} worst/budget", worst)


def test_heads_attention_refuses_L_off_a_multiple_of_8(hip):
    from visualcloze_amd.text import _Exec
    L, H, dh = 12, 2, 64
    q = torch.zeros(L, H * dh, dtype=BF, device=DEV)
    with pytest.raises(hip.VclozeHipError):
        _Exec()._heads_attention(q, q, q, L, H, dh, 1.0, None, 0, "r")
    s = sentinel((H * L, L))
    p = hip.make_problem(q[:, :dh], q[:, :dh], None, s[:L])
    p.a_zstride, p.w_zstride, p.c_zstride = dh, dh, L * s.stride(0)
    with pytest.raises(hip.VclozeHipError):
        hip.gemm(p, batch=H)
    torch.cuda.synchronize()
    assert untouched(s)


# ---------------------------------------------------------------- the unfused attention chains
def judge_chain(got, q, k, v, scale, bias, causal, pad_to, what):
    ref, mags, f32 = B.unfused_attention_case(q, k, v, scale, bias, causal, pad_to)
    print(what, "worst/budget", B.worst_ratio(got, ref, 1, mags, f32))
    return B.assert_within_budget(got, ref, 1, mags, f32, what=what)


def poison(ex, names, n):
    """the scratch pool as a larger earlier call would have left it, at its worst: every buffer full of NaN"""
    for name in names:
        ex._scratch(torch.device(DEV), name, (n,)).fill_(float("nan"))


@pytest.mark.parametrize("C", [64, 512])
def test_vae_attention_chain_within_budget(hip, C):
    """AttnBlock through _HipExec._attn, the plan's own code: the bf16 q, k, v it produced (scratch aq, ak, av) go to
    budget.unfused_attention_case (scale C^-0.5, K of P.V = Lp) and its ao is judged element by element.  L = 257 (Lk = 264,
    Lp = 320), 64 and 35 (5x7: Lk = 40, Lp = 64) in that order on ONE scratch pool that starts full of NaN: the pad rows
    k[L:Lk] and the pad columns s[:, L:Lp] must be exactly zero after every call - stale data there is the fault to catch.
    The q convolution's weight is 4x a unit-gain one: logits q.k of ~ +-100 (C = 64) .. +-300 before the scale."""
    from visualcloze_amd.vae import AttnBlock, _HipExec
    g = torch.Generator().manual_seed(C)
    blk = AttnBlock(C)
    with torch.no_grad():
        blk.norm.weight.copy_(0.5 + torch.rand(C, generator=g)); blk.norm.bias.copy_(0.25 * torch.randn(C, generator=g))
        for conv, gain in ((blk.q, 4.0), (blk.k, 1.0), (blk.v, 1.0), (blk.proj_out, 1.0)):
            conv.weight.copy_(gain * C ** -0.5 * torch.randn(C, C, 1, 1, generator=g)); conv.bias.copy_(0.25 * torch.randn(C, generator=g))
    blk = blk.to(DEV).to(BF)
    ex = _HipExec()
    poison(ex, ("t0", "aq", "ak", "av", "as", "avt", "ao"), 330 * max(C, 330))
    for L in (257, 64, 35):
        Lk, Lp = (L + 7) // 8 * 8, (L + 63) // 64 * 64
        xz = ex._act(torch.device(DEV), "xin", L, C)
        xz[:L] = torch.randn(L, C, generator=g).to(BF).to(DEV)
        out = ex._attn(blk, xz, "a")
        torch.cuda.synchronize()
        pool = ex._pool
        q, v, o = (pool[n][:L * C].view(L, C).cpu() for n in ("aq", "av", "ao"))
        k = pool["ak"][:Lk * C].view(Lk, C).cpu()
        s = pool["as"][:L * Lp].view(L, Lp).cpu()
        assert bool(torch.isfinite(out[:L].float()).all())
        assert bool((k[L:].view(torch.int16) == 0).all()), "pad key rows not zero"
        assert bool((s[:, L:].view(torch.int16) == 0).all()), "pad score columns not zero"
        judge_chain(o, q, k[:L], v, float(C) ** -0.5, None, False, Lp, f"vae chain L={L} C={C}")


def head_inputs(L, H, dh):
    parts = [B.unfused_attention_inputs(L, dh, seed=h)[:3] for h in range(H)]
    return tuple(torch.cat([p[i] for p in parts], dim=1).contiguous() for i in range(3))


def run_heads(ex, q, k, v, L, H, dh, scale, bias, causal_period, tag):
    Lp = (L + 63) // 64 * 64
    poison(ex, ("S" + tag, "VT" + tag, "O" + tag), max(H * L * Lp, H * dh * Lp))
    o = ex._heads_attention(q.to(DEV), k.to(DEV), v.to(DEV), L, H, dh, scale, bias, causal_period, tag)
    torch.cuda.synchronize()
    s = ex._pool["S" + tag][:H * L * Lp].view(H * L, Lp).cpu()
    assert bool((s[:, L:].view(torch.int16) == 0).all()), "pad score columns not zero"
    return o.cpu(), Lp


@pytest.mark.parametrize("L,H,dh", [(8, 2, 64), (72, 3, 64), (264, 2, 64)])
def test_t5_attention_chain_within_budget(hip, L, H, dh):
    """_Exec._heads_attention as T5 calls it: scale 1.0 (no rounding of the scaled logit), the position bias of
    hip.t5_position_bias, no mask.  Every head is judged against ITS bias slab.  Inputs per head: budget.unfused_attention_inputs
    (q = 4 randn, flat rows, two rows on which two keys tie, one row of all-negative logits)."""
    from visualcloze_amd.text import _Exec
    q, k, v = head_inputs(L, H, dh)
    table = (2.0 * torch.randn(32, H, generator=torch.Generator().manual_seed(L + H))).to(BF)
    bias = hip.t5_position_bias(table.to(DEV), L, 128)
    o, Lp = run_heads(_Exec(), q, k, v, L, H, dh, 1.0, bias, 0, "t")
    bc = bias.cpu()
    for h in range(H):
        c = slice(h * dh, (h + 1) * dh)
        judge_chain(o[:, c], q[:, c], k[:, c], v[:, c], 1.0, bc[h * L:(h + 1) * L], False, Lp, f"t5 chain L={L} H={H} head {h}")


@pytest.mark.parametrize("L", [8, 80])
def test_clip_attention_chain_within_budget(hip, L):
    """_Exec._heads_attention as CLIP calls it: scale dh^-0.5, causal_period = L (row i sees the keys j <= i), no bias."""
    from visualcloze_amd.text import _Exec
    H, dh = 2, 64
    q, k, v = head_inputs(L, H, dh)
    o, Lp = run_heads(_Exec(), q, k, v, L, H, dh, dh ** -0.5, None, L, "c")
    for h in range(H):
        c = slice(h * dh, (h + 1) * dh)
        judge_chain(o[:, c], q[:, c], k[:, c], v[:, c], dh ** -0.5, None, True, Lp, f"clip chain L={L} head {h}")
    assert math.isfinite(float(o.float().abs().max()))
