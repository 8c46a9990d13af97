"""The kernels that take nearly all of a Flux step - gemm.hip, norm.hip, attention.hip, attention64.hip - against plain fp64
references, element by element, with the budgets of tests/budget.py (each derived from the kernel's header comment and its code,
and met by torch's CPU results and f32 emulations of the rounding sequences in tests/test_budget_cpu.py).  Every case prints its
worst error / budget ratio before asserting, pre-fills its outputs with NaN or a sentinel and checks that pads and strides stay
untouched, and runs twice where the route is documented as reproducible.  Shapes are the smallest at which the path exists."""

import pytest
import torch

from tests import attn_schedule as S
from tests import budget as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


def within(got, case, what):
    ref, mags, f32 = case
    ref, f32 = ref.cpu(), f32.cpu()
    mags = [tuple(x.cpu() if torch.is_tensor(x) else x for x in m) if isinstance(m, tuple) else (m.cpu() if torch.is_tensor(m) else m) for m in mags]
    print(what, "worst/budget", B.worst_ratio(got, ref, len(mags), mags, f32))
    return B.assert_within_budget(got, ref, len(mags), mags, f32, what=what)


def untouched(buf, value):
    return B.bits_equal(buf, torch.full(buf.shape, value, dtype=BF))


# ---------------------------------------------------------------- GEMM
GEMM_SHAPES = [(1, 8, 64), (37, 64, 128), (129, 200, 192), (257, 264, 320), (513, 64, 1024)]
KINDS = ["cancel", "same", "exact"]


def run_gemm(hip, a_pad, w, bias, res, gate, epi, cfg, ws=None):
    """C into the first N columns of a NaN-filled [M, N + 8] buffer (ldc != N), strided A; GATE_RES: the residual in place"""
    M, N = a_pad.shape[0], w.shape[0]
    K = w.shape[1]
    buf = torch.full((M, N + 8), 7.0 if epi == 2 else NAN, dtype=BF, device=DEV)
    out = buf[:, :N]
    if epi == 2:
        out.copy_(res)
    p = hip.make_problem(a_pad[:, :K], w, bias, out, res=out if epi == 2 else None, gate=gate if epi == 2 else None)
    hip.gemm(p, epi=epi, tile_cfg=cfg, splitk_ws=ws)
    torch.cuda.synchronize()
    assert untouched(buf[:, N:], 7.0 if epi == 2 else NAN), "pad columns of C written"
    return out


def gemm_all(hip, M, N, K, cfg, epis, ws=None, what="", on_dev=False, kinds=KINDS, row_step=1):
    """row_step > 1: every row_step-th row is compared (large M: all tiles, a fraction of the elements)"""
    worst = 0.0
    for kind in kinds:
        a, w, bias, res, gate = B.gemm_inputs(M, N, K, kind)
        if kind == "exact":
            assert float((a.double().abs() @ w.double().abs().t() + bias.double().abs()).max()) <= 255.0
        a_pad = torch.zeros(M, K + 64, dtype=BF, device=DEV)
        a_pad[:, :K] = a.to(DEV)
        a_pad[:, K:] = 3.0                                         # columns beyond K: read by nothing
        d = [t.to(DEV) for t in (w, bias, res, gate)]
        src = [t.to(DEV) for t in (a, w, bias, res, gate)] if on_dev else (a, w, bias, res, gate)
        for epi in epis:
            o1 = run_gemm(hip, a_pad, d[0], d[1], d[2], d[3], epi, cfg, ws)
            o2 = run_gemm(hip, a_pad, d[0], d[1], d[2], d[3], epi, cfg, ws)
            assert B.bits_equal(o1, o2), f"{what} {kind} epi {epi}: not reproducible"
            case = B.gemm_case(src[0][::row_step], src[1], src[2], epi, src[3][::row_step], src[4])
            o1 = o1[::row_step]
            worst = max(worst, within(o1, case, f"gemm {what} {M}x{N}x{K} {kind} epi {epi}"))
            if kind == "exact" and epi in (0, 4):                  # every partial sum an integer below 2^8: exact in any order
                assert torch.equal(o1.double().cpu(), case[0].cpu()), f"{what} exact epi {epi}"
    return worst


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 19, 20, 21, 34, 36])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_tile_families_within_budget(hip, cfg, M, N, K):
    """Every tile configuration x every epilogue (EPI_QKV without a vt: plain EPI_BIAS) x three input kinds (budget.gemm_inputs),
    per element against budget.gemm_case: half an ulp at t = acc + b (with the activation's fp64 derivative or the gate as gain),
    the epilogue's own roundings, and (K + 1) * 2^-23 * (sum |a w| + |b|) for the f32 sum in any order.  M, N and K each take every
    value of {1, 37, 129, 257, 513} x {8, 64, 200, 264} x {64, 128, 192, 320, 1024} with every tile family."""
    gemm_all(hip, M, N, K, cfg, (0, 1, 2, 3, 4), what=f"cfg {cfg}")


@pytest.mark.parametrize("route,M,N,K", [(r, 257, 264, 320) for r in ("splitk2", "splitk3", "streamk")] +
                         [(r, m, n, 1024) for r in ("splitk2", "splitk3", "splitk8", "streamk") for m, n in ((513, 64), (37, 200))])
def test_gemm_split_routes_within_budget(hip, route, M, N, K):
    """GEMM_SPLITK(S) and GEMM_STREAMK below one round of tiles (every tile a remainder tile): f32 partial tiles summed by the
    reduce launch - the same budget (it holds for every order of the K + 1 terms) and, on integer data, the same bits."""
    S = {"splitk2": 2, "splitk3": 3, "splitk8": 8}.get(route)      # (K = 320 has five K-tiles: no eight-way split)
    cfg = hip.GEMM_STREAMK if S is None else hip.GEMM_SPLITK(S)
    gemm_all(hip, M, N, K, cfg, (0, 1, 2, 3), ws=hip.splitk_workspace(DEV), what=route)


@pytest.mark.parametrize("route", ["splitk3", "streamk", "persist34", "persist36"])
def test_gemm_more_than_one_round_of_tiles(hip, route):
    """The remainder routes behind a whole round of 256x192 tiles, and the persistent loop walking more tiles than CUs: the smallest
    M x N with more tiles than the device has CUs (17 x 17 = 289 tiles of 256 x 192 at 256 CUs), K = 192 (three K-tiles); every seventh row is compared."""
    M, N, K = 4100, 3096, 192
    bn = 128 if route == "persist34" else 192
    assert ((M + 255) // 256) * ((N + bn - 1) // bn) > hip.device_cus()
    cfg = {"splitk3": hip.GEMM_SPLITK(3), "streamk": hip.GEMM_STREAMK, "persist34": 34 | hip.GEMM_PERSIST, "persist36": 36 | hip.GEMM_PERSIST}[route]
    epis = (0, 1, 3) if route.startswith("persist") else (0, 2)
    gemm_all(hip, M, N, K, cfg, epis, ws=hip.splitk_workspace(DEV), what=route, on_dev=True, kinds=("cancel", "exact"), row_step=7)


@pytest.mark.parametrize("route", ["nosplit", "cut1", "cfg36", "splitk3", "streamk"])
def test_gemm_grouped_batch_strided_gated_residual(hip, route):
    """The DoubleStream proj launch: two streams of two samples in one grid, A rows read batch-strided out of a joint buffer, per-sample
    gates picked by a device step counter, the residual in place - under GEMM_NO_SPLIT, a forced cut (1 << 8), the loader-wave tile
    and both remainder routes.  Each output row against budget.gemm_case with ITS sample's gate of ITS step."""
    Bn, Nn, T, D, NO = 2, 136, 40, 128, 192
    L = Nn + T
    cfg = {"nosplit": hip.GEMM_NO_SPLIT, "cut1": 1 << 8, "cfg36": 36, "splitk3": hip.GEMM_SPLITK(3), "streamk": hip.GEMM_STREAMK}[route]
    g = torch.Generator().manual_seed(5)
    joint = torch.randn(Bn * L, NO + 64, generator=g).to(BF)
    w2, b2 = (torch.randn(D, NO, generator=g) * NO ** -0.5).to(BF), torch.randn(D, generator=g).to(BF)
    gates = torch.randn(3, Bn, D, generator=g).to(BF)
    ri, rt = torch.randn(Bn * Nn, D, generator=g).to(BF), torch.randn(Bn * T, D, generator=g).to(BF)
    jd, wd, bd, gd = joint.to(DEV), w2.to(DEV), b2.to(DEV), gates.to(DEV)
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    ld = jd.stride(0)
    outs = []
    for _ in range(2):
        bi, bt = torch.full((Bn * Nn + 1, D), 7.0, dtype=BF, device=DEV), torch.full((Bn * T + 1, D), 7.0, dtype=BF, device=DEV)
        oi, ot = bi[:Bn * Nn], bt[:Bn * T]
        oi.copy_(ri); ot.copy_(rt)
        ps = [hip.make_problem(jd[T:, :NO], wd, bd, oi, res=oi, gate=gd[0], rows_per_batch=Nn, gate_bstride=D, M=Bn * Nn, a_rpb=Nn, a_bstride=L * ld),
              hip.make_problem(jd[:T, :NO], wd, bd, ot, res=ot, gate=gd[0], rows_per_batch=T, gate_bstride=D, M=Bn * T, a_rpb=T, a_bstride=L * ld)]
        hip.gemm(ps, epi=hip.EPI_GATE_RES, tile_cfg=cfg, step_ptr=step, gate_step_stride=Bn * D, splitk_ws=hip.splitk_workspace(DEV))
        torch.cuda.synchronize()
        assert untouched(bi[Bn * Nn:], 7.0) and untouched(bt[Bn * T:], 7.0), "row behind the last written"
        outs.append((oi, ot))
    assert B.bits_equal(outs[0][0], outs[1][0]) and B.bits_equal(outs[0][1], outs[1][1])
    for b in range(Bn):
        ai, at = joint[b * L + T:(b + 1) * L, :NO], joint[b * L:b * L + T, :NO]
        within(outs[0][0][b * Nn:(b + 1) * Nn], B.gemm_case(ai, w2, b2, 2, ri[b * Nn:(b + 1) * Nn], gates[2, b]), f"grouped {route} img sample {b}")
        within(outs[0][1][b * T:(b + 1) * T], B.gemm_case(at, w2, b2, 2, rt[b * T:(b + 1) * T], gates[2, b]), f"grouped {route} txt sample {b}")


# ---------------------------------------------------------------- ln_modulate
@pytest.mark.parametrize("D", [8, 256, 3072, 4096])
@pytest.mark.parametrize("rows", [1, 3, 10])
def test_ln_modulate_within_budget(hip, rows, D):
    """y = bf16(bf16(1 + scale) * LN(x) + shift) against budget.ln_modulate_case; rows with a DC offset of 16 standard deviations
    alternating in sign plus one zero-mean row (budget.norm_inputs: the offset at which plain F.layer_norm meets the same budget,
    test_budget_cpu.py); per-batch modulation rows (rows_per_batch = 2: row r reads modulation row r // 2); ldx, ldy = D + 8."""
    x, w, b = B.norm_inputs(rows, D)
    nb = (rows + 1) // 2
    g = torch.Generator().manual_seed(rows + D)
    scale = ((w.float() - 1.25)[None] + 0.1 * torch.randn(nb, D, generator=g)).to(BF)
    shift = (b.float()[None] + 0.1 * torch.randn(nb, D, generator=g)).to(BF)
    xb = torch.full((rows, D + 8), 3.0, dtype=BF, device=DEV)
    xb[:, :D] = x.to(DEV)
    outs = []
    for _ in range(2):
        yb = torch.full((rows, D + 8), NAN, dtype=BF, device=DEV)
        hip.ln_modulate(xb[:, :D], shift.to(DEV), scale.to(DEV), out=yb[:, :D], rows_per_batch=2, mod_bstride=D)
        torch.cuda.synchronize()
        assert untouched(yb[:, D:], NAN)
        outs.append(yb[:, :D])
    assert B.bits_equal(outs[0], outs[1])
    idx = torch.arange(rows) // 2
    within(outs[0], B.ln_modulate_case(x, shift[idx], scale[idx]), f"ln_modulate rows={rows} D={D}")


@pytest.mark.parametrize("rows_a,rows_b,D", [(10, 7, 256), (3, 1, 3072), (5, 10, 4096), (1, 3, 8)])
def test_ln_modulate_two_streams_within_budget(hip, rows_a, rows_b, D):
    """ln_modulate2: two row sets in one launch whose row counts leave a 4-row block straddling the boundary; each set its own
    modulation rows (the first per batch element), rows behind each set untouched."""
    xa, w, b = B.norm_inputs(rows_a, D)
    xb_, _, _ = B.norm_inputs(rows_b + 1, D)
    xb_ = xb_[1:]                                                   # starts with an offset row
    rpb = (rows_a + 1) // 2
    sa = torch.stack([(w.float() - 1.25), (1.0 - w.float())]).to(BF)
    ha = torch.stack([b.float(), -b.float()]).to(BF)
    sb, hb = (0.5 * (w.float() - 1.25)).to(BF), (0.5 * b.float()).to(BF)
    outs = []
    for _ in range(2):
        oa, ob = torch.full((rows_a + 1, D), 7.0, dtype=BF, device=DEV), torch.full((rows_b + 1, D), 7.0, dtype=BF, device=DEV)
        hip.ln_modulate2([(xa.to(DEV), ha.to(DEV), sa.to(DEV), oa[:rows_a], rpb), (xb_.to(DEV), hb.to(DEV), sb.to(DEV), ob[:rows_b], rows_b)], mod_bstride=D)
        torch.cuda.synchronize()
        assert untouched(oa[rows_a:], 7.0) and untouched(ob[rows_b:], 7.0)
        outs.append((oa, ob))
    assert B.bits_equal(outs[0][0], outs[1][0]) and B.bits_equal(outs[0][1], outs[1][1])
    idx = torch.arange(rows_a) // rpb
    within(oa[:rows_a], B.ln_modulate_case(xa, ha[idx], sa[idx]), f"ln_modulate2 first set {rows_a}+{rows_b} D={D}")
    within(ob[:rows_b], B.ln_modulate_case(xb_, hb, sb), f"ln_modulate2 second set {rows_a}+{rows_b} D={D}")


# ---------------------------------------------------------------- QKNorm + RoPE
def qkn_case_inputs(Bn, L, H, extra):
    g = torch.Generator().manual_seed(11 * L + H + Bn)
    qkv = torch.randn(Bn * L, 3 * H * 128 + extra, generator=g)
    qkv[L // 2, :128] *= 1e-4                                       # one head row of very small values against the 1e-6 epsilon
    sc = [(1 + 0.1 * torch.randn(128, generator=g)).to(BF) for _ in range(4)]
    rope = torch.stack([B.rope_angles(L, seed=s) for s in range(Bn)]).contiguous()
    return qkv.to(BF), sc, rope


@pytest.mark.parametrize("parts", ["q", "k", "qk", "qk_pre", "all"])
@pytest.mark.parametrize("L,H,split,Bn", [(1, 1, 0, 1), (40, 3, 16, 2), (64, 1, 64, 1), (333, 9, 128, 2), (64, 3, 0, 2)])
def test_qknorm_rope_within_budget(hip, L, H, split, Bn, parts):
    """vc_qknorm_rope_vt: qknorm_rope_rows_kernel (parts without V^T) and qknorm_rope_vt_kernel ("all") against
    budget.qknorm_rope_case: the two roundings of t = bf16(bf16(x rrms) scale) carried through the rotation, the store (with
    QKN_QPRE the rotated value times 128^-0.5 log2(e), rounded once), and 2 * 2^-24 (|cos t0| + |sin t1|) for a rotation whose
    products cancel.  split at 0, inside and at L; per-sample rope with rows at angle 0, pi / 2 and pi; 8 trailing columns, the
    unselected parts, V and (without QKN_VT) vt untouched; with QKN_VT V^T exact and the pad keys zero."""
    extra = 8
    D = H * 128
    qkv, (qs, ks, qs2, ks2), rope = qkn_case_inputs(Bn, L, H, extra)
    flags = {"q": hip.QKN_Q, "k": hip.QKN_K, "qk": hip.QKN_Q | hip.QKN_K, "qk_pre": hip.QKN_Q | hip.QKN_K | hip.QKN_QPRE,
             "all": hip.QKN_Q | hip.QKN_K | hip.QKN_VT}[parts]
    Lpad = (L + 63) // 64 * 64
    outs = []
    for _ in range(2):
        work = qkv.to(DEV)
        vt = torch.full((Bn, H, 128, Lpad), 3.0, dtype=BF, device=DEV)
        hip.qknorm_rope_vt(work, qs.to(DEV), ks.to(DEV), rope.to(DEV) if Bn > 1 else rope[0].to(DEV), vt, L, H, q_scale2=qs2.to(DEV), k_scale2=ks2.to(DEV),
                           split=split, B=Bn, parts=flags)
        torch.cuda.synchronize()
        outs.append((work.cpu(), vt.cpu()))
    assert B.bits_equal(outs[0][0], outs[1][0]) and B.bits_equal(outs[0][1], outs[1][1])
    work, vt = outs[0]
    assert B.bits_equal(work[:, 2 * D:], qkv[:, 2 * D:]), "V or trailing columns written"
    rowsc = lambda s1, s2: torch.where((torch.arange(L) < split)[:, None, None], s1.float()[None, None], s2.float()[None, None]).to(BF)  # noqa: E731
    for b in range(Bn):
        x = qkv[b * L:(b + 1) * L, :3 * D].reshape(L, 3, H, 128)
        got = work[b * L:(b + 1) * L, :3 * D].reshape(L, 3, H, 128)
        for part, bit, s1, s2 in ((0, hip.QKN_Q, qs, qs2), (1, hip.QKN_K, ks, ks2)):
            if not flags & bit:
                assert B.bits_equal(got[:, part], x[:, part]), "unselected part written"
                continue
            pre = part == 0 and bool(flags & hip.QKN_QPRE)
            within(got[:, part], B.qknorm_rope_case(x[:, part], rowsc(s1, s2), rope[b], prescale=pre), f"qknorm_rope {parts} L={L} H={H} b={b} part={part}")
        if flags & hip.QKN_VT:
            assert B.bits_equal(vt[b, :, :, :L], x[:, 2].permute(1, 2, 0).contiguous()), "V^T is pure data movement"
            assert float(vt[b, :, :, L:].float().abs().sum()) == 0.0, "pad keys zero"
    if not flags & hip.QKN_VT:
        assert untouched(vt, 3.0)


# ---------------------------------------------------------------- attention
ATTN_CASES = [(1, None, None), (63, None, None), (64, None, None), (65, None, None), (200, None, None), (333, 301, None),
              (320, 320, (0, 128)), (512, 470, (100, 230))]
C32 = torch.tensor(B.QK_PRESCALE, dtype=torch.float32)


def attn_setup(L, H, Bn, kind, masks):
    """qkv rows [Bn * L, 3 H 128 + 8], V^T, the per-(sample, head) CPU inputs and the per-sample live masks"""
    extra = 8
    D = H * 128
    qkv = torch.zeros(Bn * L, 3 * D + extra, dtype=BF)
    qkv[:, 3 * D:] = 5.0
    Lpad = (L + 63) // 64 * 64
    vt = torch.zeros(Bn, H, 128, Lpad, dtype=BF)
    heads = {}
    for b in range(Bn):
        for h in range(H):
            q, k, v = B.attn_inputs(L, kind, seed=7 * b + h)
            heads[(b, h)] = (q, k, v)
            r = slice(b * L, (b + 1) * L)
            qkv[r, h * 128:(h + 1) * 128], qkv[r, D + h * 128:D + (h + 1) * 128], qkv[r, 2 * D + h * 128:2 * D + (h + 1) * 128] = q, k, v
            vt[b, h, :, :L] = v.t()
    live = [B.live_mask(L, *m) for m in masks]
    return qkv, vt, heads, live


@pytest.mark.parametrize("kind", ["normed", "peaked"])
@pytest.mark.parametrize("L,kv_len,gap", ATTN_CASES)
def test_attention_within_budget(hip, L, kv_len, gap, kind):
    """Variants 0, 1, 2, 3, 7 (attention.hip: the stored queries, the scale on the f32 logit) and 8, 12, 28 (attention64.hip: the
    queries scaled and rounded once, or prescaled), the latter with a running max and with bounded logits, per element against
    budget.attention_case.  H = 1 .. 3; two samples with different kv_len and gap; 8 trailing qkv columns; out rows of stride
    H 128 + 8 whose pad stays NaN; masked query rows exactly zero; twice, bit for bit."""
    H, Bn = 1 + L % 3, 2
    masks = [(kv_len, gap), second_mask(kv_len, gap)]
    qkv, vt, heads, live = attn_setup(L, H, Bn, kind, masks)
    D = H * 128
    qkv_pre = qkv.clone()
    qkv_pre[:, :D] = (qkv[:, :D].float() * C32).to(BF)                     # what QKN_QPRE stores: the finished query times c, rounded once
    kvl = gp = None
    if kv_len is not None:
        kvl = torch.tensor([m[0] for m in masks], dtype=torch.int32, device=DEV)
    if gap is not None:
        gp = torch.tensor([list(m[1]) for m in masks], dtype=torch.int32, device=DEV)
    cases, bound = {}, 0.0
    for (b, h), (q, k, v) in heads.items():
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        cases[(b, h, "stored")] = B.attention_case(qd, kd, vd, live[b], B.attention_route("stored"))
        cases[(b, h, "scale")] = B.attention_case(qd, kd, vd, live[b], B.attention_route("scale"))
        cases[(b, h, "prescaled")] = B.attention_case(qkv_pre[b * L:(b + 1) * L, h * 128:(h + 1) * 128].to(DEV), kd, vd, live[b], B.attention_route("prescaled"))
        bound = max(bound, float((qd.double() @ kd.double().t()).abs().max()) * B.QK_PRESCALE * 1.01)
    assert bound <= 100.0
    qd, qpd, vtd = qkv.to(DEV), qkv_pre.to(DEV), vt.to(DEV)
    routes = [(v, 0.0, "stored") for v in (0, 1, 2, 3, 7)]
    for v in (8, 12, 28):
        routes += [(v, 0.0, "scale"), (v, bound, "scale"), (v, 0.0, "prescaled"), (v, bound, "prescaled")]
    for variant, lb, route in routes:
        outs = []
        for _ in range(2):
            buf = torch.full((Bn * L, D + 8), NAN, dtype=BF, device=DEV)
            hip.attention(qpd if route == "prescaled" else qd, vtd, buf[:, :D], L, H, kv_len=kvl, kv_gap=gp, variant=variant, B=Bn,
                          logit_bound=lb, q_prescaled=route == "prescaled")
            torch.cuda.synchronize()
            assert untouched(buf[:, D:], NAN), "pad columns of out written"
            outs.append(buf[:, :D].cpu())
        assert B.bits_equal(outs[0], outs[1]), (variant, lb, route)
        for (b, h) in heads:
            got = outs[0][b * L:(b + 1) * L, h * 128:(h + 1) * 128]
            lv = live[b]
            assert float(got[~lv].float().abs().sum()) == 0.0, "masked query rows must be exactly zero"
            ref, mags, f32 = cases[(b, h, route)]
            within(got[lv], (ref[lv.to(ref.device)], mags, f32[lv.to(ref.device)]), f"attention v{variant} lb={lb:.1f} {route} {kind} L={L} b={b} h={h}")


def second_mask(kv_len, gap):
    """the other sample's masks: a shorter kv_len, a narrower gap"""
    return (None if kv_len is None else max(1, kv_len - 7), None if gap is None else (gap[0] + 3, gap[1] - 5))


@pytest.mark.parametrize("variant", [8, 12, 28])
@pytest.mark.parametrize("L,kv_len,gap", ATTN_CASES)
def test_attention_in_kernel_query_norm_within_budget(hip, variant, L, kv_len, gap):
    """q_norm=: QKNorm + RoPE of the RAW query rows inside attention64.hip, which rounds the rotated value once with the scale folded
    in - over the same lengths and masks as the other routes (two samples, kv_len and gap per sample), with a running max and
    bounded, twice bit for bit, out rows of stride H 128 + 8 whose pad stays NaN, masked query rows exactly zero.  The reference is
    independent of the pre-pass's query arithmetic: q is the fp64 QKNorm + RoPE of the raw rows times c
    (budget.qknorm_rope_case(prescale=True)) and its per-element budget enters the logit term (attention_case q_err).  K and V^T are
    what the pre-pass kernel stored (parts = K | VT): the values the attention kernel reads."""
    H, Bn = 1 + L % 3, 2
    split = L // 3
    D = H * 128
    masks = [(kv_len, gap), second_mask(kv_len, gap)]
    live = [B.live_mask(L, *m) for m in masks]
    qkv, (qs, ks, qs2, ks2), rope = qkn_case_inputs(Bn, L, H, 8)
    Lpad = (L + 63) // 64 * 64
    rd = rope.to(DEV)
    vt = torch.zeros(Bn, H, 128, Lpad, dtype=BF, device=DEV)
    w2 = qkv.to(DEV)
    hip.qknorm_rope_vt(w2, qs.to(DEV), ks.to(DEV), rd, vt, L, H, q_scale2=qs2.to(DEV), k_scale2=ks2.to(DEV), split=split, B=Bn, parts=hip.QKN_K | hip.QKN_VT)
    torch.cuda.synchronize()
    assert B.bits_equal(w2[:, :D], qkv[:, :D]), "the pre-pass without QKN_Q must leave the raw queries"
    kvl = None if kv_len is None else torch.tensor([m[0] for m in masks], dtype=torch.int32, device=DEV)
    gp = None if gap is None else torch.tensor([list(m[1]) for m in masks], dtype=torch.int32, device=DEV)
    rowsc = torch.where((torch.arange(L) < split)[:, None, None], qs.float()[None, None], qs2.float()[None, None]).to(BF)
    cases = {}
    for b in range(Bn):
        x = qkv[b * L:(b + 1) * L, :3 * D].reshape(L, 3, H, 128)
        qref, mags, f32 = B.qknorm_rope_case(x[:, 0], rowsc, rope[b], prescale=True)
        qerr = B.budget(qref, len(mags), mags, f32)
        for h in range(H):
            r = slice(b * L, (b + 1) * L)
            k, v = w2[r, D + h * 128:D + (h + 1) * 128], w2[r, 2 * D + h * 128:2 * D + (h + 1) * 128]
            assert float((qref[:, h].to(DEV) @ k.double().t()).abs().max()) < 40.0
            cases[(b, h)] = B.attention_case(qref[:, h].to(DEV), k, v, live[b], B.attention_route("prescaled"), q_err=qerr[:, h].to(DEV))
    for lb in (0.0, 40.0):
        outs = []
        for _ in range(2):
            buf = torch.full((Bn * L, D + 8), NAN, dtype=BF, device=DEV)
            hip.attention(w2, vt, buf[:, :D], L, H, kv_len=kvl, kv_gap=gp, variant=variant, B=Bn, q_norm=(qs.to(DEV), qs2.to(DEV), split, rd), logit_bound=lb)
            torch.cuda.synchronize()
            assert untouched(buf[:, D:], NAN), "pad columns of out written"
            outs.append(buf[:, :D].cpu())
        assert B.bits_equal(outs[0], outs[1]), (variant, lb)
        for (b, h), (ref, mags, f32) in cases.items():
            got = outs[0][b * L:(b + 1) * L, h * 128:(h + 1) * 128]
            lv = live[b]
            assert float(got[~lv].float().abs().sum()) == 0.0, "masked query rows must be exactly zero"
            within(got[lv], (ref[lv.to(ref.device)], mags, f32[lv.to(ref.device)]), f"attention v{variant} q_norm lb={lb} L={L} b={b} h={h}")


def tail_plan(hip, L, H, variant, prescaled, Bn=1):
    a = hip.Attention()
    a.qkv = a.vt = a.out = a.scratch = 0x1000                              # never dereferenced by the planner
    a.B, a.L, a.Lpad, a.H, a.variant = Bn, L, (L + 63) // 64 * 64, H, variant
    a.ld, a.bstride, a.ldo, a.out_bstride = 3 * H * 128, L * 3 * H * 128, H * 128, L * H * 128
    a.scratch_bytes = hip.lib().vc_attention_scratch_bytes()
    a.q_prescaled, a.logit_bound = int(prescaled), 0.0
    return hip.attention_plan(a)


@pytest.mark.parametrize("variant", [7, 12, 28])
@pytest.mark.parametrize("which", ["all_tail", "after_full_round"])
def test_attention_tail_split_within_budget(hip, variant, which):
    """The tail split at H = 24: the smallest L at which vc_attention_plan reports one at this device's CU count (every item is then
    a tail item), and the smallest L with a whole round in front of the tail.  fp64 over three heads (0, H - 1 and a seeded one) and
    at most 512 query rows per head: rows 0, 255, 256, L - 1, one row of every 64-query block (every wave of every item, so every
    piece's query block), the rest seeded.  attention64 stores each piece normalised as f16; attention.hip keeps f32 partials."""
    H = 24
    pre = variant != 7
    Ls = range(65, 4000) if which == "all_tail" else range(1025, 6000, 1)
    L = next(L for L in Ls if (lambda p: p[8] >= (0 if which == "all_tail" else 1) and p[9] > 0)(tail_plan(hip, L, H, variant, pre)))
    plan = tail_plan(hip, L, H, variant, pre)
    assert plan[8] >= 0 and plan[9] > 0, plan
    if which == "all_tail":
        assert plan[8] == 0 and plan[9] == plan[7], plan
    print(f"tail split variant {variant} {which}: L = {L}, plan {plan[:13]}")
    g = torch.Generator().manual_seed(L)
    x = torch.randn(L, 3, H, 128, generator=g)
    x[:, :2] = x[:, :2] / x[:, :2].pow(2).mean(-1, keepdim=True).sqrt()
    qkv = x.reshape(L, 3 * H * 128).to(BF)
    if pre:
        qkv[:, :H * 128] = (qkv[:, :H * 128].float() * C32).to(BF)
    qd = qkv.to(DEV)
    vt = torch.zeros(1, H, 128, (L + 63) // 64 * 64, dtype=BF, device=DEV)
    vt[0, :, :, :L] = qd[:, 2 * H * 128:].reshape(L, H, 128).permute(1, 2, 0)
    outs = []
    for lb in ((0.0, 40.0) if pre else (0.0,)):
        for _ in range(2):
            out = torch.full((L, H * 128), NAN, dtype=BF, device=DEV)
            hip.attention(qd, vt, out, L, H, variant=variant, q_prescaled=pre, logit_bound=lb)
            torch.cuda.synchronize()
            outs.append(out)
        assert B.bits_equal(outs[-1], outs[-2]), "the tail split is reproducible from launch to launch"
    must = sorted({0, min(255, L - 1), min(256, L - 1), L - 1} | set(range(0, L, 64)))
    extra = torch.randperm(L, generator=g)[:max(0, 512 - len(must))].tolist()
    rows = torch.tensor(sorted(set(must) | set(extra))[:max(512, len(must))])
    assert set(must) <= set(rows.tolist())
    live = torch.ones(L, dtype=torch.bool)
    route = B.attention_route("prescaled" if pre else "stored", "f16" if pre else "f32")
    for h in sorted({0, H - 1, int(torch.randint(0, H, (1,), generator=g))}):
        q, k, v = qd[:, h * 128:(h + 1) * 128], qd[:, (H + h) * 128:(H + h + 1) * 128], qd[:, (2 * H + h) * 128:(2 * H + h + 1) * 128]
        assert float((q.double() @ k.double().t()).abs().max()) * (1.0 if pre else B.QK_PRESCALE) < 40.0
        case = B.attention_case(q, k, v, live, route, rows=rows.to(DEV))
        for i, out in enumerate(outs[::2]):
            within(out[rows.to(DEV), h * 128:(h + 1) * 128], case, f"attention tail split v{variant} {which} L={L} lb#{i} h={h}")


ALL_ROUTES = [(v, 0.0, "stored") for v in (0, 1, 2, 3, 7)] + [(v, lb, r) for v in (8, 12, 28) for lb in (0.0, 100.0) for r in ("scale", "prescaled")]


def one_hot_run(hip, L, H, Bn, masks, routes, kvl, gp):
    """budget.one_hot_inputs per sample (q, k shared by the heads, V per head), V^T with 64.0 in the pad keys of the last tile; every
    route twice: live rows equal the partner's V row bit for bit, masked query rows are exactly zero, the out pad stays NaN"""
    D = H * 128
    Lpad = (L + 63) // 64 * 64
    qkv = torch.full((Bn * L, 3 * D + 8), 5.0, dtype=BF)
    vt = torch.full((Bn, H, 128, Lpad), 64.0, dtype=BF)
    live = [B.live_mask(L, *m) for m in masks]
    want = torch.zeros(Bn * L, D, dtype=BF)
    for b in range(Bn):
        assert bool(live[b].any()), "never mask every key of a sample"
        q, k, partner, vf = B.one_hot_inputs(L, live[b], seed=b)
        assert B.one_hot_stray_weight(q.to(DEV), k.to(DEV), live[b], partner) <= 2.0 ** -12
        assert sorted(partner[live[b]].tolist()) == live[b].nonzero().flatten().tolist()      # every live key is used: key 0, 63, 64, kv_len - 1, gap edges, piece edges
        r = slice(b * L, (b + 1) * L)
        for h in range(H):
            v = vf(h)
            qkv[r, h * 128:(h + 1) * 128], qkv[r, D + h * 128:D + (h + 1) * 128], qkv[r, 2 * D + h * 128:2 * D + (h + 1) * 128] = q, k, v
            vt[b, h, :, :L] = v.t()
            want[r, h * 128:(h + 1) * 128] = torch.where(live[b][:, None], v[partner], torch.zeros_like(v))
    qkv_pre = qkv.clone()
    qkv_pre[:, :D] = (qkv[:, :D].float() * C32).to(BF)
    qd, qpd, vtd = qkv.to(DEV), qkv_pre.to(DEV), vt.to(DEV)
    for variant, lb, route in routes:
        for rep in range(2):
            buf = torch.full((Bn * L, D + 8), NAN, dtype=BF, device=DEV)
            hip.attention(qpd if route == "prescaled" else qd, vtd, buf[:, :D], L, H, kv_len=kvl, kv_gap=gp, variant=variant, B=Bn,
                          logit_bound=lb, q_prescaled=route == "prescaled")
            torch.cuda.synchronize()
            assert untouched(buf[:, D:], NAN), "pad columns of out written"
            got = buf[:, :D].cpu()
            lv = torch.cat(live)
            assert float(got[~lv].float().abs().sum()) == 0.0, f"one-hot v{variant} lb={lb} {route} L={L}: masked query rows must be exactly zero (of either sign)"
            bad = ((got.view(torch.int16) != want.view(torch.int16)).any(-1) & lv).nonzero().flatten()
            assert bad.numel() == 0, f"one-hot v{variant} lb={lb} {route} L={L} run {rep}: {bad.numel()} rows differ from their V row, first {bad[:8].tolist()}"


@pytest.mark.parametrize("L,kv_len,gap", ATTN_CASES)
def test_attention_one_hot_returns_the_v_row_bit_for_bit(hip, L, kv_len, gap):
    """q_i = 4 u_partner(i), k_j = u_j (budget.one_hot_inputs): each live row puts all but 2^-12 of its weight (asserted in fp64; in
    fact 2^-40) on ONE key, through a permutation that uses every live key - key 0, 63, 64, kv_len - 1, gap_lo - 1, gap_hi - so the
    output row is that key's V row bit for bit on every route, and a key lost or shifted by one is a wrong row.  Every masked key
    (beyond kv_len, inside the gap, the pad of the last tile) carries V = 64 and - those with a K row - a K row aligned with a live
    query above its true partner: any leak is a gross error.  Bounded routes run at logit_bound = 100 (aligned logit 65.5, masked
    98.25).  Two samples with their own masks, H = 1 .. 3."""
    H, Bn = 1 + L % 3, 2
    masks = [(kv_len, gap), second_mask(kv_len, gap)]
    kvl = None if kv_len is None else torch.tensor([m[0] for m in masks], dtype=torch.int32, device=DEV)
    gp = None if gap is None else torch.tensor([list(m[1]) for m in masks], dtype=torch.int32, device=DEV)
    one_hot_run(hip, L, H, Bn, masks, ALL_ROUTES, kvl, gp)


@pytest.mark.parametrize("variant", [7, 12, 28])
@pytest.mark.parametrize("which", ["all_tail", "after_full_round"])
def test_attention_one_hot_tail_split(hip, variant, which):
    """The same at the tail-split lengths of test_attention_tail_split_within_budget, H = 24, ALL rows of all heads: every key is some
    row's partner, the first and last key of every tail piece included, so a key lost at a piece boundary - 0.04 % of a row of normed
    data at L = 2561, invisible to any budget - is a wrong V row here.  The pad keys of the last tile carry V = 64."""
    H = 24
    pre = variant != 7
    Ls = range(65, 4000) if which == "all_tail" else range(1025, 6000)
    L = next(L for L in Ls if (lambda p: p[8] >= (0 if which == "all_tail" else 1) and p[9] > 0)(tail_plan(hip, L, H, variant, pre)))
    plan = tail_plan(hip, L, H, variant, pre)
    assert plan[8] >= 0 and plan[9] > 0, plan
    routes = [(variant, lb, "prescaled") for lb in (0.0, 100.0)] if pre else [(7, 0.0, "stored")]
    one_hot_run(hip, L, H, 1, [(None, None)], routes, None, None)


# ---------------------------------------------------------------- attention: the tail split at uneven, sparse and batched schedules
# (name, family, (B, H) candidates, classes of tests/attn_schedule.py the geometry must have, the pick at 256 CUs as (B, L, H))
EDGE_GEOMS = [
    ("uneven_sparse", 64, [(1, 1), (1, 3)], {"uneven", "xcd_without_tail", "empty_chunks"}, (1, 321, 1)),
    ("uneven_sparse_sample_1", 64, [(2, 1), (2, 3)], {"uneven", "xcd_without_tail", "empty_chunks", "tail_sample_ge1"}, (2, 321, 1)),
    ("nine_pieces_uneven", 64, [(1, 1), (1, 3)], {"uneven", "pieces_ge_9"}, (1, 513, 1)),
    ("w_pieces", 64, [(1, 1), (1, 2)], {"pieces_eq_W"}, (1, 1985, 1)),
    ("uneven_behind_a_round_batch", 64, [(3, 11), (3, 7), (2, 11)], {"uneven", "behind_whole_round", "batch", "tail_sample_ge1"}, (3, 2049, 11)),
    ("even_behind_a_round_batch", 64, [(3, 24), (2, 24)], {"even", "behind_whole_round", "batch", "tail_sample_ge1"}, (3, 769, 24)),
    ("v7_sparse", 32, [(1, 1), (1, 3)], {"empty_chunks"}, (1, 257, 1)),
    ("v7_sparse_batch", 32, [(2, 1), (2, 3)], {"empty_chunks", "batch", "tail_sample_ge1"}, (2, 257, 1)),
]
EDGE_NAMES = [g[0] for g in EDGE_GEOMS]
_edge_cache = {}


def edge_geometry(hip, name):
    """(B, L, H, family, largest piece count) of an edge class at THIS device's CU count: the first (B, H) candidate, and the
    smallest L <= 3000 with it, whose classes (tests/attn_schedule.py, run for this CU count) include the wanted ones and for which
    vc_attention_plan reports a split.  None is a failure, not a skip; only a CU count that is no multiple of 8 skips (the
    planner never splits the 64-query family there, and the classes are defined on the per-XCD schedule)."""
    n_cu = hip.device_cus(DEV)
    if n_cu % 8:
        pytest.skip(f"{n_cu} CUs: no multiple of 8, no per-XCD schedule")
    if name not in _edge_cache:
        _, family, cands, want, at256 = next(g for g in EDGE_GEOMS if g[0] == name)
        pick = next(((Bn, L, H) for Bn, H in cands for L in range(65, 3001) if want <= S.classes(Bn, L, H, n_cu, family)), None)
        assert pick is not None, f"{name}: no geometry with L <= 3000 has the classes {sorted(want)} at {n_cu} CUs"
        if n_cu == 256:
            assert pick == at256, (name, pick, at256)
        Bn, L, H = pick
        g = S.geom(Bn, L, H, n_cu, family)
        rs = (S.plan64 if family == 64 else S.plan32)(g)
        for v in ((12, 28) if family == 64 else (7,)):
            plan = tail_plan(hip, L, H, v, v != 7, Bn)
            assert plan[8:11] == [rs["full_rounds"], rs["tail_items"], rs["tail_units"]] and plan[11] == (v == 28), (name, v, plan, rs)
            assert plan[12] == (0 if v == 28 else rs["merge_grid"]), (name, v, plan, rs)
            print(f"edge class {name}: (B, L, H) = {pick} at {n_cu} CUs, variant {v} plan {plan[:13]}")
        assert want <= S.classes(Bn, L, H, n_cu, family)
        _edge_cache[name] = (Bn, L, H, family, S.max_pieces(g, family))
        print(f"edge class {name}: items {g.items}, {g.nkt} tiles, classes {sorted(S.classes(Bn, L, H, n_cu, family))}, at most {_edge_cache[name][4]} pieces per item")
    return _edge_cache[name]


def flags_all_zero(hip, plan):
    """the flag words of the in-launch combine: from plan word 13 to the end of the attention scratch"""
    return int(hip.attention_scratch(torch.device(DEV))[plan[13]:].to(torch.int32).sum()) == 0


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_attention_one_hot_edge_schedules(hip, name):
    """The one-hot test (every live key is some row's partner: ALL rows of all heads and samples, bit for bit) at the schedules that
    H = 24 and B = 1 never produce: XCDs with different shares or no tail at all, fewer (item, tile) units than workgroups - empty
    chunks, and workgroups of variant 28 that own a combine task but no work - , 9 and W pieces per item, tail items of samples 1 and
    2.  A tile lost, doubled or given to the wrong item, head or sample is a wrong V row (V differs by head and sample).  Variants
    12 and 28 prescaled, with a running max and at logit_bound 100, and 12 with the scale route (the per-item kernel's writer);
    variant 7 stored.  Twice each (one_hot_run); the flag words are zero afterwards."""
    Bn, L, H, family, _ = edge_geometry(hip, name)
    if family == 64:
        routes = [(v, lb, "prescaled") for v in (12, 28) for lb in (0.0, 100.0)] + [(12, 0.0, "scale")]
    else:
        routes = [(7, 0.0, "stored")]
    one_hot_run(hip, L, H, Bn, [(None, None)] * Bn, routes, None, None)
    assert flags_all_zero(hip, tail_plan(hip, L, H, routes[0][0], family == 64, Bn)), "flag words left set"


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_attention_edge_schedules_within_budget(hip, name):
    """Normed data at the same geometries against budget.attention_case, ALL heads of all samples; all rows where L <= 1024, else the
    512-row rule of test_attention_tail_split_within_budget.  The route's piece count is the restatement's largest.  Variant 28
    equals variant 12 bit for bit, every route twice with the same bits, the out pad stays NaN, the flag words end zero."""
    Bn, L, H, family, pieces = edge_geometry(hip, name)
    pre = family == 64
    D = H * 128
    g = torch.Generator().manual_seed(L + 7 * Bn + H)
    x = torch.randn(Bn * L, 3, H, 128, generator=g)
    x[:, :2] = x[:, :2] / x[:, :2].pow(2).mean(-1, keepdim=True).sqrt()
    qkv = x.reshape(Bn * L, 3 * D).to(BF)
    if pre:
        qkv[:, :D] = (qkv[:, :D].float() * C32).to(BF)
    qd = qkv.to(DEV)
    vt = torch.zeros(Bn, H, 128, (L + 63) // 64 * 64, dtype=BF, device=DEV)
    vt[:, :, :, :L] = qd[:, 2 * D:].reshape(Bn, L, H, 128).permute(0, 2, 3, 1)
    outs = {}
    for variant in ((12, 28) if pre else (7,)):
        for lb in ((0.0, 40.0) if pre else (0.0,)):
            two = []
            for _ in range(2):
                buf = torch.full((Bn * L, D + 8), NAN, dtype=BF, device=DEV)
                hip.attention(qd, vt, buf[:, :D], L, H, variant=variant, B=Bn, q_prescaled=pre, logit_bound=lb)
                torch.cuda.synchronize()
                assert untouched(buf[:, D:], NAN), "pad columns of out written"
                two.append(buf[:, :D].cpu())
            assert B.bits_equal(two[0], two[1]), f"{name} v{variant} lb={lb}: not reproducible from launch to launch"
            outs[(variant, lb)] = two[0]
        assert flags_all_zero(hip, tail_plan(hip, L, H, variant, pre, Bn)), "flag words left set"
    if pre:
        for lb in (0.0, 40.0):
            assert B.bits_equal(outs[(28, lb)], outs[(12, lb)]), f"{name} lb={lb}: the in-launch combine differs from the merge kernel"
    if L <= 1024:
        rows = torch.arange(L)
    else:
        must = sorted({0, 255, 256, L - 1} | set(range(0, L, 64)))
        extra = torch.randperm(L, generator=g)[:max(0, 512 - len(must))].tolist()
        rows = torch.tensor(sorted(set(must) | set(extra))[:max(512, len(must))])
        assert set(must) <= set(rows.tolist())
    live = torch.ones(L, dtype=torch.bool)
    route = B.attention_route("prescaled" if pre else "stored", "f16" if pre else "f32", pieces=pieces)
    worst = {}
    for b in range(Bn):
        for h in range(H):
            r = slice(b * L, (b + 1) * L)
            q, k, v = qd[r, h * 128:(h + 1) * 128], qd[r, (H + h) * 128:(H + h + 1) * 128], qd[r, (2 * H + h) * 128:(2 * H + h + 1) * 128]
            assert float((q.double() @ k.double().t()).abs().max()) * (1.0 if pre else B.QK_PRESCALE) < 40.0
            case = B.attention_case(q, k, v, live, route, rows=rows.to(DEV))
            for (variant, lb), out in outs.items():
                if variant == 28:
                    continue                                                # the bits of variant 12, asserted above
                w = within(out[r][rows, h * 128:(h + 1) * 128], case, f"attention {name} v{variant} lb={lb} (B, L, H)=({Bn}, {L}, {H}) b={b} h={h}")
                worst[(variant, lb)] = max(worst.get((variant, lb), 0.0), w)
    print(f"edge class {name} (B, L, H) = ({Bn}, {L}, {H}): worst error / budget per route {worst}")
