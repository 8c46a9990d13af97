"""GPU: vc_resample_u8, vc_pixels_in and vc_mask_fill (csrc/resample.hip, csrc/pixels_in.hip).

* vc_resample_u8 against Pillow's recorded outputs (tests/golden/resample_golden.npz; tests/test_resample_cpu.py holds the rule alone
  to live PIL): 0 mismatching bytes, every fixture shape, both filters.  A differing byte is reported with its output index and the
  integer weights of that index.
* vc_pixels_in bit for bit against the torch expression (u8.float() / 255 - 0.5) / 0.5 [.to(bf16)].  ToTensor runs on the host in the
  reference, where torch divides; on the device torch multiplies by the reciprocal when the divisor is a Python number, which is
  another function, so the device evaluation here divides by a 0-dim device tensor (a true division) - and the host evaluation of
  all 256 bytes is held to it.
* vc_pixels_out with bytes out -> vc_pixels_in round trip on a 32x48 image."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_golden.npz")


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def expected(u8: torch.Tensor, dtype) -> torch.Tensor:
    """the torch expression on the device, [.., 3] bytes -> same shape"""
    v = (u8.float() / torch.tensor(255.0, device=u8.device) - 0.5) / 0.5
    return v.to(dtype)


@pytest.mark.parametrize("flt", ["bicubic", "lanczos"])
@pytest.mark.parametrize("i", range(10))
def test_resample_u8_equals_pillow_byte_for_byte(hip, golden, i, flt):
    W, H, w, h = (int(v) for v in golden["rs_shapes"][i])
    src = torch.from_numpy(golden[f"rs_in_{i}"]).to(DEV)
    want = torch.from_numpy(golden[f"rs_{flt}_{i}"]).to(DEV)
    got = hip.resample_u8(src, (w, h), flt)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (h, w, 3)
    bad = (got != want).nonzero()
    if len(bad):
        y, x, c = (int(v) for v in bad[0])
        tabs = {}
        if W != w:
            xmin, ln, ki = hip.resample_coeffs(W, w, flt)
            tabs["horizontal"] = (int(xmin[x]), ki[x, :int(ln[x])].tolist())
        if H != h:
            xmin, ln, ki = hip.resample_coeffs(H, h, flt)
            tabs["vertical"] = (int(xmin[y]), ki[y, :int(ln[y])].tolist())
        pytest.fail(f"{len(bad)} bytes differ; first at (y, x, c) = {(y, x, c)}: got {int(got[y, x, c])}, Pillow {int(want[y, x, c])}; "
                    f"(xmin, weights) {tabs}")


def test_the_host_and_the_device_evaluation_of_the_expression_agree(hip):
    b = torch.arange(256, dtype=torch.uint8)
    host = (b.float() / 255 - 0.5) / 0.5
    assert torch.equal(expected(b.to(DEV), torch.float32).cpu(), host)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", [
    dict(size=(16, 16), left=3, top=5, x0=0, Wrow=16),           # inside, aligned
    dict(size=(13, 9), left=7, top=2, x0=5, Wrow=31),            # inside, odd x0 / w / Wrow
    dict(size=(20, 12), left=-6, top=4, x0=16, Wrow=48),         # over the left edge
    dict(size=(20, 12), left=30, top=4, x0=1, Wrow=48),          # over the right edge
    dict(size=(12, 20), left=5, top=-7, x0=0, Wrow=12),          # over the top edge
    dict(size=(12, 20), left=5, top=20, x0=3, Wrow=17),          # over the bottom edge
    dict(size=(60, 50), left=-10, top=-9, x0=2, Wrow=64),        # larger than the image on every side
    dict(size=(8, 8), left=100, top=100, x0=0, Wrow=8),          # entirely outside
], ids=["inside", "inside_odd", "left", "right", "top", "bottom", "around", "outside"])
def test_pixels_in_equals_the_torch_expression(hip, case, dtype):
    H, W = 33, 41                                                  # more than one block of 256 threads in most cases
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(DEV)
    w, h = case["size"]
    left, top, x0, Wrow = case["left"], case["top"], case["x0"], case["Wrow"]
    out = torch.full((3, h, Wrow), 7.0, dtype=dtype, device=DEV)
    hip.pixels_in(img, (w, h), left, top, out=out, x0=x0)
    torch.cuda.synchronize()
    P = 128                                                       # Image.crop: outside reads 0
    big = torch.zeros(H + 2 * P, W + 2 * P, 3, dtype=torch.uint8, device=DEV)
    big[P:P + H, P:P + W] = img
    crop = big[P + top:P + top + h, P + left:P + left + w]
    want = torch.full_like(out, 7.0)
    want[:, :, x0:x0 + w] = expected(crop, dtype).permute(2, 0, 1)
    assert torch.equal(out, want)                                 # the window bit for bit, nothing outside it written


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_blank_cell_and_mask_fill(hip, dtype):
    out = torch.full((3, 16, 40), 7.0, dtype=dtype, device=DEV)
    hip.pixels_in(None, (11, 16), out=out, x0=9)
    mask = torch.full((16, 40), 7.0, dtype=torch.bfloat16, device=DEV)
    hip.mask_fill(mask, 9, 11, 1)
    hip.mask_fill(mask, 0, 9, 0)
    torch.cuda.synchronize()
    assert bool((out[:, :, 9:20] == -1.0).all()) and bool((out[:, :, :9] == 7.0).all()) and bool((out[:, :, 20:] == 7.0).all())
    assert bool((mask[:, 9:20] == 1.0).all()) and bool((mask[:, :9] == 0.0).all()) and bool((mask[:, 20:] == 7.0).all())


def test_pixels_out_then_pixels_in_round_trip(hip):
    """a decoded image -> bytes (truncating) -> back: what comes back is the normalised byte, bit for bit"""
    from tests.procedural import ptensor
    img = ptensor((3, 32, 48), 77, q=7).to(DEV, torch.bfloat16)
    u8 = hip.pixels_out(img, uint8=True)
    back = hip.pixels_in(u8, (48, 32))
    part = hip.pixels_in(hip.pixels_out(img, x0=16, w=16, uint8=True), (16, 32))
    torch.cuda.synchronize()
    want = expected(((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0).mul(255).to(torch.uint8).permute(1, 2, 0), torch.bfloat16).permute(2, 0, 1)
    assert back.dtype == torch.bfloat16 and torch.equal(back, want) and torch.equal(part, want[:, :, 16:32])
    assert float((back.float() - img.float()).abs().max()) <= 2.0 / 255 + 2.0 ** -7    # one byte step and bf16's rounding of [-1, 1]
