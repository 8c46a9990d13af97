"""vc_pixels_out (csrc/pixels_out.hip) on the GPU, BIT FOR BIT against the torch expressions it replaces at the end of both pipeline
stages: ((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0), pipeline.to_uint8_image's .mul(255).to(torch.uint8) and the crop of a cell.
Sizes: one pixel; 16x24 (no 16-column run: element-wise); 32x112 (seven 16-column cells: the 16-byte path, several workgroups of
runs); windows: the whole image, an aligned middle cell, a cell with odd x0 and odd width."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1
SIZES = [(1, 1), (16, 24), (32, 112)]


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


def image(H, W, dtype):
    """values all over [-1, 1] and beyond, the exact ends, and values whose v * 255 lies within one ulp of an integer"""
    g = torch.Generator().manual_seed(1000 * H + W)
    x = torch.rand(3, H, W, generator=g) * 2.6 - 1.3
    flat = x.view(-1)
    k = torch.arange(0, 256, dtype=torch.float64)
    edge = []
    for d in (-1, 0, 1):                      # v = k / 255 one f32 ulp below / at / above: x = 2 v - 1
        v = (k / 255.0).to(torch.float32)
        v = torch.nextafter(v, torch.full_like(v, 2.0 if d > 0 else -2.0)) if d else v
        edge.append(v * 2 - 1)
    special = torch.cat([torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, -0.0, 1.0000001, -0.99999994]), *edge])
    n = min(special.numel(), flat.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = special[:n]
    return x.to(DEV, dtype)


def windows(W):
    out = [(0, W)]
    if W >= 48:
        out.append((W // 16 // 2 * 16, 16))                 # an aligned middle cell
    if W >= 8:
        out.append((3, W - 3 - 2 if (W - 5) % 2 else W - 3 - 3))   # odd x0, odd width
    return out


def reference(img, x0, w):
    v = ((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0)                       # pipeline.generate_grid, :431-432
    u8 = v.mul(255).to(torch.uint8).permute(1, 2, 0).contiguous()           # pipeline.to_uint8_image
    return v[:, :, x0:x0 + w].contiguous(), u8[:, x0:x0 + w].contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixels_out_equals_the_torch_expressions_bitwise(hip, size, dtype):
    H, W = size
    img = image(H, W, dtype)
    for x0, w in windows(W):
        assert w % 2 == 1 or (x0, w) == (0, W) or (x0 % 16 == 0 and w == 16)
        want_f, want_u = reference(img, x0, w)
        got_f = hip.pixels_out(img, x0, w)
        got_u = hip.pixels_out(img, x0, w, uint8=True)
        torch.cuda.synchronize()
        assert got_f.shape == (3, H, w) and got_f.dtype == torch.float32 and got_u.shape == (H, w, 3) and got_u.dtype == torch.uint8
        assert torch.equal(got_f.view(torch.int32), want_f.view(torch.int32)), (size, x0, w)
        assert torch.equal(got_u, want_u), (size, x0, w, (got_u.int() - want_u.int()).abs().max())
    if H * W >= 256:
        u = reference(img, 0, W)[1]
        assert int(u.min()) == 0 and int(u.max()) == 255


def test_the_window_writes_nothing_outside_its_output(hip):
    """both paths into the middle of a guarded buffer: the bytes before and after stay"""
    H, W = 32, 112
    img = image(H, W, torch.bfloat16)
    for x0, w in ((32, 16), (3, 21)):
        n = H * w * 3
        buf = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device=DEV)
        out = buf[256:256 + n].view(H, w, 3)
        hip.pixels_out(img, x0, w, uint8=True, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, reference(img, x0, w)[1]) and bool((buf[:256] == 0x5A).all()) and bool((buf[256 + n:] == 0x5A).all())


def test_argument_errors_come_back_before_any_device_work(hip):
    L = hip.lib()
    img = image(16, 24, torch.bfloat16)
    out = torch.full((3, 16, 24), 7.0, device=DEV)
    st = hip.cur_stream()
    call = lambda H, W, x0, w, form=0, i=img.data_ptr(), o=out.data_ptr(): L.vc_pixels_out(i, 0, H, W, x0, w, o, form, st)  # noqa: E731
    for args, word in (((16, 24, 20, 5), b"window"), ((16, 24, -1, 5), b"window"), ((16, 24, 0, 0), b"window"), ((0, 24, 0, 1), b"size"),
                       ((16, 70000, 0, 1), b"size")):
        assert call(*args) == ERR_ARG and word in L.vc_last_error(), (args, L.vc_last_error())
    assert call(16, 24, 0, 24, form=2) == ERR_ARG and b"out_form" in L.vc_last_error()
    assert call(16, 24, 0, 24, o=None) == ERR_ARG and call(16, 24, 0, 24, i=None) == ERR_ARG
    assert call(16, 24, 0, 24, o=img.data_ptr() + 64) == ERR_ARG and b"overlaps" in L.vc_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(16, 24, 0, 24) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, reference(img, 0, 24)[0])
