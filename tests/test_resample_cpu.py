"""CPU: the host side of the photo front end (csrc/resample.hip, csrc/grid_rules.hip, csrc/pixels_in.hip's formula).

* vc_resample_coeffs, applied with numpy as the header states the rule, against live PIL.Image.resize: BIT-IDENTICAL, both filters,
  up- and down-scaling, one axis unchanged, the copy, 1x1 on either side and a scale above 20 (large kmax);
* vc_fit_size / vc_grid_layout / vc_upsampling_size against the recorded results of the reference's own functions
  (tests/golden/resample_golden.npz) and against a direct Python evaluation of the same expressions;
* the vc_pixels_in formula restated on the host against torch, all 256 bytes;
* every argument error: VC_ERR_ARG with a message, no device touched (there is none here); the struct sizes; the C99 demo links.
"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "resample_golden.npz")
ERR_ARG = -1
SHAPES = [(37, 53, 16, 32), (48, 80, 112, 64), (301, 203, 96, 64), (64, 64, 64, 48), (50, 70, 160, 224), (97, 33, 16, 16),
          (16, 16, 16, 16), (1, 1, 16, 16), (16, 16, 1, 1), (333, 17, 16, 48)]          # (W, H, w, h)
PLAN_FIELDS = ("present", "fit_w", "fit_h", "cover_w", "cover_h", "crop_left", "crop_top", "cell_w", "cell_h", "final_w", "final_h", "mask")


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        h.build()
    h.lib()
    return h


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def apply_axis(hip, a: np.ndarray, n_out: int, flt: str) -> np.ndarray:
    """the rule of include/vcloze_hip.h along axis 1 of a [lines, n_in, 3], from the library's tables"""
    n_in = a.shape[1]
    if n_in == n_out:
        return a
    xmin, ln, ki = (t.numpy() for t in hip.resample_coeffs(n_in, n_out, flt))
    assert (xmin >= 0).all() and (ln >= 1).all() and (xmin + ln <= n_in).all()         # every tap inside the image
    assert all((ki[i, ln[i]:] == 0).all() for i in range(n_out))
    out = np.empty((a.shape[0], n_out, 3), np.uint8)
    for xx in range(n_out):
        acc = (a[:, xmin[xx]:xmin[xx] + ln[xx]].astype(np.int64) * ki[xx, :ln[xx], None].astype(np.int64)).sum(1) + (1 << 21)
        assert np.abs(acc).max() < 2 ** 31                                              # it fits int32
        out[:, xx] = np.clip(acc >> 22, 0, 255)
    return out


def resize_by_tables(hip, a, w, h, flt):
    t = apply_axis(hip, a, w, flt)                                                      # horizontal first, 8-bit intermediate
    return apply_axis(hip, np.ascontiguousarray(t.transpose(1, 0, 2)), h, flt).transpose(1, 0, 2)


@pytest.mark.parametrize("flt", ["bicubic", "lanczos"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_tables_reproduce_pil_resize_bit_for_bit(hip, shape, flt):
    from PIL import Image
    W, H, w, h = shape
    a = np.random.default_rng(W * 1000 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((w, h), Image.BICUBIC if flt == "bicubic" else Image.LANCZOS))
    got = resize_by_tables(hip, a, w, h, flt)
    assert got.shape == want.shape and int((got != want).sum()) == 0
    kmax = hip.lib().vc_resample_kmax(W, w, hip.FILTERS[flt])
    S = 2 if flt == "bicubic" else 3
    assert kmax == int(np.ceil(S * max(W / w, 1.0))) * 2 + 1
    if shape == (333, 17, 16, 48):
        assert kmax > 80 if flt == "bicubic" else kmax > 120                            # scale 20.8


def test_fixture_holds_the_same_pil_results(hip, golden):
    """the GPU tests read only the fixture: it must be what the tables give too"""
    assert golden["rs_shapes"].tolist() == [list(s) for s in SHAPES]
    for i, (W, H, w, h) in enumerate(SHAPES):
        a = golden[f"rs_in_{i}"]
        assert a.shape == (H, W, 3) and a.dtype == np.uint8
        for flt in ("bicubic", "lanczos"):
            assert np.array_equal(resize_by_tables(hip, a, w, h, flt), golden[f"rs_{flt}_{i}"]), (i, flt)


def test_fit_size_and_upsampling_size_equal_the_reference_and_python(hip, golden):
    from visualcloze_amd import pipeline
    fin, fout = golden["fit_in"], golden["fit_out"]
    assert len(fin) >= 200 and (fin[:, :2].min(1) < 16).any() and (fin[:, 0] != fin[:, 1]).any()
    for (w, h, r), want in zip(fin.tolist(), fout.tolist()):
        assert list(hip.fit_size(w, h, r)) == want == list(pipeline.fit_size(w, h, r)), (w, h, r)
    uin, uout = golden["ups_in"], golden["ups_out"]
    assert (uin[:, 0].astype(np.int64) * uin[:, 1] > 1024 * 1024).any()                 # the area cap is exercised
    for (w, h), want in zip(uin.tolist(), uout.tolist()):
        size = None if (w, h) == (0, 0) else (w, h)
        got = hip.upsampling_size(size)
        assert list(got) == list(pipeline.upsampling_size(size)), (w, h)
        if want != [-1, -1]:                                                            # (-1, -1): the reference raised, nothing recorded
            assert list(got) == want, (w, h)
    assert hip.upsampling_size(None) == (1024, 1024)


def test_grid_layout_equals_the_reference_loop(hip, golden):
    L = hip.lib()
    seen = dict(negative=False, second=False, refused=0, default384=False)
    for c in range(int(golden["lay_count"])):
        sizes, res = golden[f"lay_{c}_sizes"], int(golden[f"lay_{c}_res"])
        grid = [[None if tuple(s) == (0, 0) else tuple(int(v) for v in s) for s in row] for row in sizes]
        if not int(golden[f"lay_{c}_ok"]):
            with pytest.raises(hip.VclozeHipError):
                hip.grid_layout(grid, res)
            assert L.vc_last_error()
            seen["refused"] += 1
            continue
        got = [[getattr(p, f) for f in PLAN_FIELDS] for row in hip.grid_layout(grid, res) for p in row]
        want = golden[f"lay_{c}_plan"].tolist()
        assert got == want, (c, got, want)
        seen["negative"] |= any(p[5] < 0 or p[6] < 0 for p in got)
        seen["second"] |= any(p[9:11] != p[7:9] for p in got)
        seen["default384"] |= any(p[9] == 384 for p in got)
    assert seen["negative"] and seen["second"] and seen["default384"] and seen["refused"] >= 2, seen


def test_grid_layout_follows_the_python_expressions(hip):
    """a direct evaluation of the reference's expressions (pipeline.fit_size and Python's own // and int) on seeded grids"""
    from visualcloze_amd import pipeline
    rng = np.random.default_rng(7)
    for _ in range(60):
        gw, res = int(rng.integers(1, 4)), int(rng.choice([32, 64, 96]))
        grid = [[tuple(int(v) for v in rng.integers(8, 400, 2)) for _ in range(gw)] for _ in range(2)]
        for j in range(gw):
            if rng.random() < 0.4:
                grid[1][j] = None
        plans = hip.grid_layout(grid, res)
        for row, prow in zip(grid, plans):
            first = next((s for s in row if s is not None), None)
            ref = (res, res) if first is None else pipeline.fit_size(*first, res)
            for s, p in zip(row, prow):
                assert (p.cell_w, p.cell_h) == ref and p.present == int(s is not None) and p.mask == int(s is None)
                if s is None:
                    continue
                tw, th = pipeline.fit_size(*s, res)
                cover = (ref[0], int(ref[0] / tw * th)) if tw <= th else (int(ref[1] / th * tw), ref[1])
                assert (p.fit_w, p.fit_h, p.cover_w, p.cover_h) == (tw, th, *cover)
                assert (p.crop_left, p.crop_top) == ((cover[0] - ref[0]) // 2, (cover[1] - ref[1]) // 2)


def test_preprocess_grid_with_pil_gives_the_reference_cells(golden):
    """the PIL path of pipeline.preprocess_grid against the cells the reference's process_images made of the same photographs"""
    from visualcloze_amd import pipeline
    a, b = (torch.from_numpy(golden[f"photo_{j}"]) for j in range(2))
    rows, masks = pipeline.preprocess_grid([[a, b], [b, None]], 32, device="cpu")
    cells = [(torch.from_numpy(golden[f"photo_cell_{k}"].copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5 for k in range(4)]
    for i in range(2):
        assert torch.equal(rows[i], torch.cat(cells[2 * i:2 * i + 2], dim=2).to(torch.bfloat16))
    assert not masks[0].any() and masks[1].shape == (1, 1, 16, 64) and not masks[1][..., :32].any() and bool((masks[1][..., 32:] == 1).all())


def test_pixels_in_formula_on_the_host():
    """v = (f32(byte) / 255 - 0.5) / 0.5, each operation rounded in f32, then bf16: numpy's f32 arithmetic against torch's"""
    b = np.arange(256, dtype=np.uint8)
    v = ((b.astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)
    want = (torch.from_numpy(b).float() / 255 - 0.5) / 0.5
    assert torch.equal(torch.from_numpy(v), want)
    assert float(want[0]) == -1.0 and float(want[255]) == 1.0
    bf = want.to(torch.bfloat16)
    assert float(bf[0]) == -1.0 and float(bf[255]) == 1.0 and len(set(bf.tolist())) > 200
    # the division is a true one: multiplying by the rounded reciprocal differs for some bytes, so the kernel must divide
    rec = torch.from_numpy(b).float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert not torch.equal(rec, torch.from_numpy(b).float() / 255)


def test_argument_errors_have_a_message_and_touch_no_device(hip):
    L = hip.lib()
    i32 = lambda n: (C.c_int32 * n)()  # noqa: E731
    bad = lambda rc, word: rc == ERR_ARG and word in L.vc_last_error()  # noqa: E731
    assert bad(L.vc_resample_kmax(0, 4, 0), b"1..65535") and bad(L.vc_resample_kmax(4, 65536, 0), b"1..65535")
    assert bad(L.vc_resample_kmax(4, 4, 2), b"filter")
    assert bad(L.vc_resample_coeffs(8, 4, 0, None, i32(4), i32(36), 9), b"null")
    assert bad(L.vc_resample_coeffs(8, 4, 0, i32(4), i32(4), i32(36), 7), b"kmax") and L.vc_resample_kmax(8, 4, 0) == 9
    assert L.vc_resample_tmp_bytes(0, 4, 4, 4, 0) == ERR_ARG and L.vc_resample_tmp_bytes(4, 4, 4, 4, 9) == ERR_ARG
    need = L.vc_resample_tmp_bytes(8, 8, 4, 4, 0)
    assert need > 0 and need % 256 == 0 and L.vc_resample_tmp_bytes(8, 8, 8, 8, 1) == 256
    A, B, T = 0x10000, 0x20000, 0x30000                     # never dereferenced: every check comes first
    rs = lambda src=A, H=8, W=8, dst=B, h=4, w=4, f=0, tmp=T, n=need: L.vc_resample_u8(src, H, W, dst, h, w, f, tmp, n, None)  # noqa: E731
    assert bad(rs(src=None), b"null") and bad(rs(dst=None), b"null") and bad(rs(tmp=None), b"null")
    assert bad(rs(H=0), b"1..65535") and bad(rs(w=70000), b"1..65535") and bad(rs(f=5), b"filter")
    assert bad(rs(n=need - 1), b"too small") and bad(rs(tmp=T + 8), b"aligned")
    assert bad(rs(dst=A + 16), b"overlap") and bad(rs(tmp=A), b"overlap") and bad(rs(dst=T + 256, tmp=T, n=need + 4096), b"overlap")
    px = lambda src=A, H=8, W=8, l=0, t=0, out=B, f32=0, h=8, Wr=16, x0=0, w=8: L.vc_pixels_in(src, H, W, l, t, out, f32, h, Wr, x0, w, None)  # noqa: E731,E741
    assert bad(px(out=None), b"null") and bad(px(h=0), b"window") and bad(px(x0=9), b"window") and bad(px(x0=-1), b"window")
    assert bad(px(w=0), b"window") and bad(px(H=0), b"1..65535") and bad(px(l=70000), b"crop") and bad(px(out=B + 1), b"aligned")
    assert bad(px(out=B + 2, f32=1), b"aligned") and bad(px(out=A + 8), b"overlap")
    mf = lambda m=A, h=8, Wr=16, x0=0, w=8, v=1: L.vc_mask_fill(m, h, Wr, x0, w, v, None)  # noqa: E731
    assert bad(mf(m=None), b"null") and bad(mf(x0=12), b"window") and bad(mf(v=2), b"0 or 1") and bad(mf(m=A + 1), b"aligned")
    a, b_ = C.c_int32(7), C.c_int32(7)
    assert bad(L.vc_fit_size(0, 4, 32, C.byref(a), C.byref(b_)), b"1..65535") and bad(L.vc_fit_size(4, 4, 32, None, C.byref(b_)), b"null")
    assert bad(L.vc_upsampling_size(0, 5, C.byref(a), C.byref(b_)), b"0x0") and bad(L.vc_upsampling_size(-1, -1, C.byref(a), C.byref(b_)), b"0x0")
    assert (a.value, b_.value) == (7, 7)                    # nothing was written
    plan = (hip.CellPlan * 4)()
    w4, h4 = (C.c_int32 * 4)(40, 70, 70, 0), (C.c_int32 * 4)(56, 50, 50, 0)
    assert L.vc_grid_layout(2, 2, w4, h4, 32, plan) == 0
    assert bad(L.vc_grid_layout(0, 2, w4, h4, 32, plan), b"rows and columns") and bad(L.vc_grid_layout(2, 2, None, h4, 32, plan), b"null")
    assert bad(L.vc_grid_layout(2, 2, w4, h4, 0, plan), b"resolution")
    assert bad(L.vc_grid_layout(2, 2, (C.c_int32 * 4)(40, 0, 70, 0), (C.c_int32 * 4)(56, 0, 50, 0), 32, plan), b"absent")
    assert bad(L.vc_grid_layout(2, 2, (C.c_int32 * 4)(40, 70, 70, 0), (C.c_int32 * 4)(56, 50, 0, 0), 32, plan), b"0x0")
    # the handle calls refuse a null handle / job before anything else
    n64 = C.c_int64(0)
    assert bad(L.vc_grid_generate_photos(None, None, None, 0, None, None), b"null handle")
    assert bad(L.vc_grid_sdedit_u8(None, None, None, 0, None, None), b"null handle")
    assert bad(L.vc_grid_photos_workspace_bytes(None, None, C.byref(n64)), b"null handle")
    assert bad(L.vc_grid_sdedit_u8_workspace_bytes(None, None, C.byref(n64)), b"null handle")


def test_photo_struct_sizes_and_symbols(hip):
    sizes = (C.c_int32 * 3)()
    hip.lib().vc_photo_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(hip.CellPlan), C.sizeof(hip.GridPhotos), C.sizeof(hip.GridSdeditU8)]
    R = hip.GRID_MAX_ROWS
    assert C.sizeof(hip.CellPlan) == 12 * 4
    assert C.sizeof(hip.GridPhotos) == 4 * 4 + 3 * 8 + R * 4 + 2 * 8 + 2 * 4 + 3 * 8 + 4 * 4 + 8
    assert C.sizeof(hip.GridSdeditU8) == 6 * 4 + R * 8 + 2 * 8 + 2 * 4 + 3 * 8 + 4 * 4 + 8
    assert hip.lib().vc_abi_version() == 11 and hasattr(hip.lib(), "vc_resample_u8")   # detected by symbol, no ABI bump


def test_device_resize_is_off_by_default():
    import inspect
    from visualcloze_amd import pipeline
    for fn in (pipeline.upsample_images, pipeline.generate_and_upsample, pipeline.preprocess_grid):
        assert inspect.signature(fn).parameters["device_resize"].default is False


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_photo_demo_compiles_and_links_as_c99(hip, tmp_path):
    from tests.photo_demo_build import build_photo_demo
    assert os.path.getsize(build_photo_demo(tmp_path)) > 0
