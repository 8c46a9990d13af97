"""vc_image_compare on the MI355X against the float64 restatement of its rule (tests/image_metrics_ref.py).

Geometries (tile side T = 32): 11x11 (one window), 11x12, 12x11, 42x42 (exactly one tile), 43x73 (a second, partial tile on each
axis), 43x75 with C = 3, 43x48 on the 16-byte path, and the last two again with the base pointer moved by one element, which forces
the element-wise path.  Both forms.  Inputs: seeded random bytes / floats, and a smooth ramp plus noise.

8-bit form: sse, max_abs, n_diff EXACTLY numpy's integers, one case past 2^32.  F32 sums and the mean SSIM: within the budget the
reference module derives from the header's order of operations (nothing fitted); the measured share of the budget is printed.
Properties: identical images, swapped operands, repeated runs, a captured and replayed call, the refusal of H = 10, and
pipeline.compare_images on both forms of one vc_pixels_out result.  Every test here fails on a library without vc_image_compare."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import image_metrics_ref as R

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 11, 11), (3, 11, 12), (1, 12, 11), (3, 42, 42), (1, 43, 73), (3, 43, 75), (3, 43, 48)]
_cache = {}


def _images(form, Cn, H, W, kind):
    """(a, b) numpy: seeded; "random": independent; "ramp": a smooth ramp, b = a plus small noise"""
    g = np.random.default_rng(1000 * H + 10 * W + Cn + (7 if kind == "ramp" else 0))
    if kind == "random":
        a, b = g.random((Cn, H, W)), g.random((Cn, H, W))
    else:
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(0.2 + 0.6 * (x + (c + 1) * y) / (W + (c + 1) * H)) for c in range(Cn)])
        b = np.clip(a + 0.02 * g.standard_normal((Cn, H, W)), 0.0, 1.0)
        b[:, ::3, ::2] = a[:, ::3, ::2]                                   # some elements stay equal: n_diff < n
    if form == "u8":
        return tuple(np.ascontiguousarray((v * 255.0).astype(np.uint8).transpose(1, 2, 0)) for v in (a, b))
    a, b = a.astype(np.float32), b.astype(np.float32)
    if kind == "ramp":
        b[:, ::3, ::2] = a[:, ::3, ::2]
    return a, b


def _ref(form, Cn, H, W, kind):
    key = (form, Cn, H, W, kind)
    if key not in _cache:
        a, b = _images(form, Cn, H, W, kind)
        _cache[key] = (a, b, R.compare(a, b))
    return _cache[key]


def _dev(x, offset=False):
    """the array on the device; offset: at a base one ELEMENT past a 256-byte aligned address (the element-wise path)"""
    t = torch.from_numpy(x)
    if not offset:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 != 0 and d.is_contiguous()
    return d


def _raw(a, b):
    from visualcloze_amd import hip
    r = hip.image_compare_raw(a, b)
    torch.cuda.synchronize()
    return r.cpu().numpy().tobytes()


def _check_against_ref(got, ref, what):
    assert got["n"] == ref["n"] and got["n_windows"] == ref["n_windows"], what
    assert got["n_diff"] == ref["n_diff"], what
    if got["form"] == 0:
        assert got["sse"] == ref["sse"] and got["max_abs"] == ref["max_abs"], (what, got, ref)
        assert got["psnr_db"] == pytest.approx(ref["psnr_db"], rel=1e-14), what
    else:
        e_sse, e_max = abs(got["sse"] - ref["sse"]), abs(got["max_abs"] - ref["max_abs"])
        print(f"{what}: sse err {e_sse:.3e} of budget {ref['sse_budget']:.3e}; max_abs err {e_max:.3e} of {ref['max_abs_budget']:.3e}")
        assert e_sse <= ref["sse_budget"] and e_max <= ref["max_abs_budget"], what
    e = abs(got["ssim"] - ref["ssim"])
    print(f"{what}: ssim {got['ssim']:.9f} ref {ref['ssim']:.12f} err {e:.3e} budget {ref['ssim_budget']:.3e} (x{e / ref['ssim_budget']:.3f})")
    assert e <= ref["ssim_budget"], (what, e, ref["ssim_budget"])
    return e / ref["ssim_budget"]


@pytest.mark.parametrize("kind", ["random", "ramp"])
@pytest.mark.parametrize("form", ["u8", "f32"])
def test_matches_the_fp64_restatement(form, kind):
    from visualcloze_amd import hip
    worst = 0.0
    for Cn, H, W in GEOMETRIES:
        a, b, ref = _ref(form, Cn, H, W, kind)
        got = hip.image_compare(_dev(a), _dev(b))
        worst = max(worst, _check_against_ref(got, ref, f"{form} {kind} {Cn}x{H}x{W}"))
    print(f"{form} {kind}: worst share of the ssim budget {worst:.3f}")


@pytest.mark.parametrize("form", ["u8", "f32"])
def test_element_path_equals_the_wide_path_bit_for_bit(form):
    """43x48 is 16-aligned: the 16-byte path; the same images one element off alignment run element-wise - same bits.  43x75 has a
    W that is no multiple of 16 and runs element-wise at either base."""
    from visualcloze_amd import hip
    for Cn, H, W in ((3, 43, 48), (3, 43, 75)):
        a, b, ref = _ref(form, Cn, H, W, "ramp")
        aligned, moved = _raw(_dev(a), _dev(b)), _raw(_dev(a, True), _dev(b, True))
        assert aligned == moved, (form, H, W)
        _check_against_ref(hip.image_compare(_dev(a, True), _dev(b, True)), ref, f"{form} offset base {Cn}x{H}x{W}")


def test_u8_sse_past_32_bits():
    """a 3 x 384 x 1152 row image, all 0 against all 255: sse = 255^2 * 1 327 104 = 8.6e10 > 2^32"""
    from visualcloze_amd import hip
    a = torch.zeros(384, 1152, 3, dtype=torch.uint8, device="cuda")
    b = torch.full((384, 1152, 3), 255, dtype=torch.uint8, device="cuda")
    m = hip.image_compare(a, b)
    n = 3 * 384 * 1152
    assert m["sse"] == 255 * 255 * n > 2 ** 32 and m["n_diff"] == n and m["max_abs"] == 255.0 and m["n"] == n
    assert m["psnr_db"] == 0.0 and m["mse"] == 255.0 * 255.0
    c1 = R.constants(255.0)[0]                                # constant images: ssim = C1 / (255^2 + C1) times a sigma factor near 1
    assert 0.0 < m["ssim"] < 2 * c1 / (255.0 * 255.0)


@pytest.mark.parametrize("form", ["u8", "f32"])
def test_properties(form):
    from visualcloze_amd import hip
    for Cn, H, W in ((3, 43, 75), (3, 43, 48), (1, 11, 11)):
        a, b, _ = _ref(form, Cn, H, W, "random")
        da, db = _dev(a), _dev(b)
        same = hip.image_compare(da, da.clone())
        assert same["ssim"] == 1.0 and same["sse"] == 0 and same["psnr_db"] == math.inf and same["n_diff"] == 0 and same["max_abs"] == 0.0
        assert hip.image_compare(da, da)["ssim"] == 1.0                      # the same buffer twice
        ab, ba = _raw(da, db), _raw(db, da)
        assert ab == ba, "swapping the operands changes bits"
        assert _raw(da, db) == ab, "two runs differ"


def test_captured_and_replayed_call_gives_the_same_bits():
    from visualcloze_amd import hip
    a, b, _ = _ref("f32", 3, 43, 75, "ramp")
    da, db = _dev(a), _dev(b)
    eager = _raw(da, db)
    out = torch.zeros(C.sizeof(hip.ImageMetrics), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(hip.image_compare_scratch_bytes(3, 43, 75), dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with hip.Graph(st.cuda_stream) as g:
        hip.image_compare_raw(da, db, out=out, scratch=scratch, stream=st.cuda_stream)
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.launch()
        st.synchronize()
        assert out.cpu().numpy().tobytes() == eager


def test_h_10_is_refused():
    from visualcloze_amd import hip
    a = torch.zeros(3, 10, 64, device="cuda")
    out = torch.zeros(48, dtype=torch.uint8, device="cuda")
    rc = hip.lib().vc_image_compare(a.data_ptr(), a.data_ptr(), hip.IMG_F32_CHW, 3, 10, 64, out.data_ptr(), out.data_ptr(), 48, None)
    assert rc == -1 and "11..65535" in hip.lib().vc_last_error().decode()
    with pytest.raises(ValueError, match="11 x 11"):
        hip.image_compare(a, a)
    u = torch.zeros(64, 10, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="11 x 11"):
        hip.image_compare(u, u)
    with pytest.raises(ValueError, match="one form"):
        hip.image_compare(torch.zeros(3, 16, 16, device="cuda"), torch.zeros(3, 16, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="shapes differ"):
        hip.image_compare(torch.zeros(3, 16, 16, device="cuda"), torch.zeros(3, 16, 17, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        hip.image_compare(torch.zeros(3, 16, 32, device="cuda")[:, :, ::2], torch.zeros(3, 16, 16, device="cuda"))
    with pytest.raises(ValueError, match="uint8 or float32"):
        hip.image_compare(torch.zeros(3, 16, 16, device="cuda", dtype=torch.bfloat16), torch.zeros(3, 16, 16, device="cuda", dtype=torch.bfloat16))


def test_pipeline_compare_images_on_both_forms_of_a_pixels_out_result():
    """two decoded images through vc_pixels_out: the 8-bit form, and the F32 form truncated to 8 bits on the host, give the same
    8-bit metrics; compare_images agrees with the direct calls, for tensors and for lists"""
    from visualcloze_amd import hip, pipeline
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(3, 48, 80, generator=g) * 2.2 - 1.1)
    y = (x + 0.05 * torch.randn(3, 48, 80, generator=g))
    x, y = x.to(torch.bfloat16).cuda(), y.to(torch.bfloat16).cuda()
    fx, fy = hip.pixels_out(x), hip.pixels_out(y)
    ux, uy = hip.pixels_out(x, uint8=True), hip.pixels_out(y, uint8=True)
    hx, hy = (f.mul(255).to(torch.uint8).permute(1, 2, 0).contiguous() for f in (fx, fy))       # the truncating rule, on the host side
    assert torch.equal(hx, ux) and torch.equal(hy, uy)
    keys = ("psnr_db", "ssim", "mse", "max_abs", "n_diff")
    m8, mh, mf = pipeline.compare_images(ux, uy), pipeline.compare_images(hx, hy), pipeline.compare_images(fx, fy)
    assert set(m8) == set(keys) and m8 == mh
    d8, df = hip.image_compare(ux, uy), hip.image_compare(fx, fy)
    assert m8 == {k: d8[k] for k in keys} and mf == {k: df[k] for k in keys}
    ref8 = R.compare(ux.cpu().numpy(), uy.cpu().numpy())
    assert d8["sse"] == ref8["sse"] and d8["n_diff"] == ref8["n_diff"] and abs(d8["ssim"] - ref8["ssim"]) <= ref8["ssim_budget"]
    both = pipeline.compare_images([fx, ux], [fy, uy])
    assert both == [mf, m8]
