"""vc_image_compare without a GPU: the float64 restatement of the rule (tests/image_metrics_ref.py) checked on its own - the weights
against the header's list, symmetry, identical images, one closed form - and the host-only surface of the library: the symbols
declared, exported and bound, sizeof(VcImageMetrics), vc_image_compare_scratch_bytes, vc_image_psnr and every argument refusal of
vc_image_compare (all found before the device is touched).  The ABI checks fail on a library without the feature."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import image_metrics_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vc_image_struct_sizes", "vc_image_compare_scratch_bytes", "vc_image_compare", "vc_image_psnr")
P = 0x10000          # a non-null, 16-byte aligned address no refused call ever touches


def _hdr():
    return open(os.path.join(REPO, "include", "vcloze_hip.h")).read()


# ---------------------------------------------------------------------------------------------- 1. the restatement
def test_weights_equal_the_headers_list():
    m = re.search(r"#define VC_SSIM_WEIGHTS \{([^}]*)\}", _hdr())
    listed = np.array([np.float32(x.strip().rstrip("f")) for x in m.group(1).replace("\\", " ").split(",")], dtype=np.float32)
    w = R.weights()
    assert listed.shape == (11,) and w.dtype == np.float32
    assert np.array_equal(listed.view(np.uint32), w.view(np.uint32))
    assert np.array_equal(w, w[::-1]) and abs(float(w.astype(np.float64).sum()) - 1.0) < 11 * 2.0 ** -25
    k = np.arange(11) - 5.0
    assert np.allclose(w, np.exp(-k * k / (2 * 1.5 ** 2)) / np.exp(-k * k / (2 * 1.5 ** 2)).sum(), rtol=1e-7)     # sigma = 1.5


def _pair(form, C_, H, W, seed):
    g = np.random.default_rng(seed)
    if form == "u8":
        return g.integers(0, 256, (H, W, C_), dtype=np.uint8), g.integers(0, 256, (H, W, C_), dtype=np.uint8)
    return g.random((C_, H, W), dtype=np.float32), g.random((C_, H, W), dtype=np.float32)


@pytest.mark.parametrize("form", ["u8", "f32"])
def test_symmetric_in_the_operands(form):
    a, b = _pair(form, 3, 19, 23, 1)
    x, y = R.compare(a, b), R.compare(b, a)
    assert x == y and 0.0 < x["ssim_budget"] < 1e-4 and x["n_windows"] == 3 * 9 * 13


@pytest.mark.parametrize("form", ["u8", "f32"])
def test_identical_images_give_exactly_one_and_inf(form):
    a, _ = _pair(form, 3, 17, 31, 2)
    m = R.compare(a, a.copy())
    assert m["ssim"] == 1.0 and m["psnr_db"] == math.inf and m["sse"] == 0 and m["n_diff"] == 0 and m["max_abs"] == 0


@pytest.mark.parametrize("form,la,lb,tol", [("u8", 1, 2, 1e-15), ("u8", 0, 3, 1e-15), ("f32", 0.0078125, 0.015625, 1e-15),
                                            ("u8", 40, 200, None), ("u8", 0, 255, None), ("f32", 0.25, 0.75, None), ("f32", 0.0, 1.0, None)])
def test_constant_images_match_the_closed_form(form, la, lb, tol):
    """two constant images: the sigma terms vanish and SSIM = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1).  Hand-computable levels hold
    the closed form to 1e-15.  At large levels the restatement's own float64 roundings show: e_aa and mu_a^2 are level^2-sized and
    cancel to ~0, each carrying the ~24 roundings of its two passes, against C2 - the bound there is 100 * 2^-53 * level^2 / C2."""
    if form == "u8":
        a, b, L = np.full((13, 14, 2), la, np.uint8), np.full((13, 14, 2), lb, np.uint8), 255.0
    else:
        a, b, L = np.full((2, 13, 14), la, np.float32), np.full((2, 13, 14), lb, np.float32), 1.0
    c1, c2 = R.constants(L)
    wsum = float(R.weights().astype(np.float64).sum()) ** 2                # the window's total weight, both passes: 1 - 2.8e-9
    ma, mb = wsum * float(la), wsum * float(lb)
    m = R.compare(a, b)
    # the weights are rounded to F32 AFTER the normalisation, so the window's weight is 1 - eps and the sigma terms of a constant
    # image are eps-sized, not 0: E[a^2] - mu_a^2 = wsum (1 - wsum) la^2.  Kept, the closed form holds to 1e-15 ...
    va, vb, cab = wsum * la * la - ma * ma, wsum * lb * lb - mb * mb, wsum * la * lb - ma * mb
    closed = ((2 * ma * mb + c1) * (2 * cab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    assert abs(m["ssim"] - closed) <= (tol if tol is not None else 1e-15 + 100 * 2.0 ** -53 * max(la, lb) ** 2 / c2)
    # ... and dropped, SSIM = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1) up to the factor (2 cab + C2) / (va + vb + C2) = 1 - eps (la - lb)^2 / C2
    eps = wsum * (1.0 - wsum)
    plain = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
    assert 0.0 < eps < 4e-9 and abs(closed - plain) <= 1.01 * eps * (float(la) - float(lb)) ** 2 / c2 + 1e-15
    d = float(lb) - float(la)
    assert m["sse"] == pytest.approx(d * d * a.size, rel=1e-15) and m["n_diff"] == a.size
    assert m["psnr_db"] == pytest.approx(10 * math.log10(L * L / (d * d)), abs=1e-12)


def test_tiles_partition_every_extent():
    """the header's ownership rule: the owned ranges of the tiles along an axis cover [0, extent) once"""
    for extent in list(range(11, 140)) + [384, 1152, 1024, 65535]:
        T = R.tiles(extent)
        covered = 0
        for t in range(T):
            halo = min(42, extent - 32 * t)
            assert 11 <= halo <= 42 and 1 <= halo - 10 <= 32
            own = halo if t == T - 1 else 32
            assert 32 * t == covered
            covered += own
        assert covered == extent and sum(min(42, extent - 32 * t) - 10 for t in range(T)) == extent - 10


# ---------------------------------------------------------------------------------------------- 2. the host-only surface
def test_abi_surface():
    from visualcloze_amd import hip
    L = hip.lib()
    hdr = _hdr()
    declared = set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NEW_SYMBOLS:
        assert name in declared and name in hip.SYMBOLS and name in exported, name
        m = re.search(r"^(?:int|void|double) " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m and len(hip.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    assert declared == set(hip.SYMBOLS)
    assert L.vc_abi_version() == 11 == hip.ABI_VERSION and re.search(r"#define VC_ABI_VERSION 11\b", hdr)      # pinned by earlier tests: not bumped
    size = (C.c_int32 * 1)()
    L.vc_image_struct_sizes(size)
    assert size[0] == 48 == C.sizeof(hip.ImageMetrics)
    for name, val in (("VC_IMG_U8_HWC", hip.IMG_U8_HWC), ("VC_IMG_F32_CHW", hip.IMG_F32_CHW), ("VC_IMG_TILE", hip.IMG_TILE),
                      ("VC_IMG_RECORD_BYTES", hip.IMG_RECORD_BYTES)):
        assert int(re.search(r"#define " + name + r" (\d+)", hdr).group(1)) == val
    assert hip.IMG_TILE == R.TILE


def _refused(rc, L, *words):
    assert rc == -1, rc                                   # VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert all(w in msg for w in words), msg


def test_scratch_bytes_without_a_device():
    from visualcloze_amd import hip
    L = hip.lib()
    n = C.c_int64()
    for geo in ((1, 11, 11), (3, 11, 12), (3, 42, 42), (3, 43, 73), (3, 43, 75), (3, 384, 1152), (3, 1024, 1024), (65535, 65535, 65535)):
        assert L.vc_image_compare_scratch_bytes(*geo, C.byref(n)) == 0
        assert n.value == R.scratch_bytes(*geo) == hip.image_compare_scratch_bytes(*geo), geo
    assert R.scratch_bytes(3, 42, 42) == 3 * 32 and R.scratch_bytes(3, 43, 73) == 3 * 4 * 32
    _refused(L.vc_image_compare_scratch_bytes(3, 10, 64, C.byref(n)), L, "11..65535")
    _refused(L.vc_image_compare_scratch_bytes(3, 64, 10, C.byref(n)), L, "11..65535")
    _refused(L.vc_image_compare_scratch_bytes(3, 65536, 64, C.byref(n)), L, "11..65535")
    _refused(L.vc_image_compare_scratch_bytes(0, 64, 64, C.byref(n)), L, "C = 0")
    _refused(L.vc_image_compare_scratch_bytes(65536, 64, 64, C.byref(n)), L, "C = 65536")
    _refused(L.vc_image_compare_scratch_bytes(3, 64, 64, None), L, "null")


def test_image_compare_argument_errors_without_a_device():
    from visualcloze_amd import hip
    L = hip.lib()
    ok = dict(a=P, b=P + 4096, form=hip.IMG_F32_CHW, C=3, H=43, W=75, out=P, scratch=P, nbytes=R.scratch_bytes(3, 43, 75))

    def call(**k):
        v = dict(ok, **k)
        return L.vc_image_compare(v["a"], v["b"], v["form"], v["C"], v["H"], v["W"], v["out"], v["scratch"], v["nbytes"], None)

    for k in ("a", "b", "out", "scratch"):
        _refused(call(**{k: None}), L, "null")
    _refused(call(form=2), L, "unknown form 2")
    _refused(call(form=-1), L, "unknown form")
    _refused(call(H=10), L, "11..65535", "10x75")
    _refused(call(W=10), L, "11..65535")
    _refused(call(H=0), L, "11..65535")
    _refused(call(W=65536), L, "11..65535")
    _refused(call(C=0), L, "C = 0")
    _refused(call(a=P + 2), L, "4 bytes")
    _refused(call(b=P + 1), L, "4 bytes")
    _refused(call(out=P + 8), L, "16 bytes")
    _refused(call(scratch=P + 4), L, "16 bytes")
    _refused(call(nbytes=R.scratch_bytes(3, 43, 75) - 1), L, "smaller")
    _refused(call(form=hip.IMG_U8_HWC, H=10), L, "11..65535")
    _refused(call(form=hip.IMG_U8_HWC, a=P + 1, nbytes=0), L, "smaller")          # a byte image needs no alignment: the next check answers


def test_psnr_host_helper():
    from visualcloze_amd import hip
    L = hip.lib()
    out = C.c_double()

    def psnr(s):
        assert L.vc_image_psnr(C.byref(s), C.byref(out)) == 0
        return out.value
    n = 3 * 384 * 1152
    m = hip.ImageMetrics(n=n, n_windows=1, sse_u64=255 * 255 * n, n_diff=n, sse_f32=0.0, max_abs=255.0, ssim_mean=0.0, form=hip.IMG_U8_HWC)
    assert m.sse_u64 > 2 ** 32 and psnr(m) == 0.0
    m.sse_u64 = 0
    assert psnr(m) == math.inf
    m.sse_u64 = 12345
    assert psnr(m) == pytest.approx(10 * math.log10(255.0 * 255.0 * n / 12345), rel=1e-15)
    f = hip.ImageMetrics(n=1000, n_windows=1, sse_u64=0, n_diff=5, sse_f32=0.25, max_abs=0.5, ssim_mean=0.5, form=hip.IMG_F32_CHW)
    assert psnr(f) == pytest.approx(10 * math.log10(1000 / 0.25), rel=1e-15)
    f.sse_f32 = 0.0
    assert psnr(f) == math.inf
    _refused(L.vc_image_psnr(None, C.byref(out)), L, "null")
    _refused(L.vc_image_psnr(C.byref(f), None), L, "null")


def test_python_wrappers_refuse_with_value_errors():
    import torch
    from visualcloze_amd import hip, pipeline
    a = torch.zeros(3, 16, 16)
    with pytest.raises(ValueError, match="CUDA"):
        hip.image_compare(a, a)
    with pytest.raises(ValueError, match="torch tensor"):
        hip.image_compare(a.numpy(), a)
    with pytest.raises(ValueError, match="one length"):
        pipeline.compare_images([a], [a, a])
    with pytest.raises(ValueError, match="one length"):
        pipeline.compare_images([a], a)
