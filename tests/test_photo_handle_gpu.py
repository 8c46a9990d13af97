"""The photo front end of the grid handle on the GPU (vc_grid_generate_photos, vc_grid_sdedit_u8; pipeline.preprocess_grid and the
`device_resize` switches).  Everything is BIT FOR BIT: the resampler gives Pillow's bytes (tests/test_resample_gpu.py), the rest is the
path tests/test_grid_handle_gpu.py already holds to the pipeline.  The tiny model of that file; a 2x2 grid of photographs of 40x56 and
70x50 pixels at resolution 32 (rows of 32x32 and 16x64 pixels, one cell to generate); Pillow's cells and Pillow's resized
intermediate come from tests/golden/resample_golden.npz."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests.test_grid_handle_gpu import CFG, SEED, STEPS, data, gh, hip, mods, same  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_golden.npz")
RES = 32


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def photos(golden):
    a, b = (torch.from_numpy(golden[f"photo_{j}"]).to(DEV) for j in range(2))
    return [[a, b], [b, None]]


def normalised(u8: np.ndarray) -> torch.Tensor:
    """ToTensor + Normalize(0.5, 0.5) on the host, as the pipeline does it: [H, W, 3] bytes -> f32 [3, H, W]"""
    return (torch.from_numpy(u8.copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5


@pytest.fixture(scope="module")
def pillow_rows(golden):
    """the row tensors and masks the reference builds from Pillow's cells (visualcloze.py:363-374)"""
    cells = [golden[f"photo_cell_{k}"] for k in range(4)]
    rows = [torch.cat([normalised(c) for c in cells[i * 2:i * 2 + 2]], dim=2).to(DEV, torch.bfloat16) for i in range(2)]
    h, w = cells[2].shape[:2]
    masks = [torch.zeros(1, 1, *rows[0].shape[-2:], device=DEV, dtype=torch.bfloat16),
             torch.cat((torch.zeros(1, 1, h, w), torch.ones(1, 1, h, w)), -1).to(DEV, torch.bfloat16)]
    assert [tuple(r.shape) for r in rows] == [(3, 32, 32), (3, 16, 64)]
    return rows, masks


def test_generate_photos_is_bit_identical_to_generate_grid_on_pillows_cells(gh, mods, data, photos, pillow_rows):
    from visualcloze_amd import pipeline
    rows, masks = pillow_rows
    rng = pipeline.NoiseStream(SEED, offset=5)
    want = pipeline.generate_grid(*mods, rows, masks, data["t5_ids"], data["clip_ids"], SEED, cfg=CFG, steps=STEPS, rng=rng, use_grid_handle=True)
    torch.cuda.synchronize()
    got, off = gh.generate_photos(photos, RES, data["t5_ids"], data["clip_ids"], SEED, 5, cfg=CFG, steps=STEPS)
    torch.cuda.synchronize()
    assert off == rng.offset and len(got) == 2
    for g, w in zip(got, want):
        assert same(g, w) and float(g.std()) > 0
    # a second job of the same geometry captures nothing, and repeats the bits
    counts = (gh.vae.plan_count(), gh.t5.plan_count(), gh.clip.plan_count())
    again, off2 = gh.generate_photos(photos, RES, data["t5_ids"], data["clip_ids"], SEED, 5, cfg=CFG, steps=STEPS)
    torch.cuda.synchronize()
    assert (gh.vae.plan_count(), gh.t5.plan_count(), gh.clip.plan_count()) == counts and off2 == off
    assert all(same(a, b) for a, b in zip(again, want))


def test_preprocess_grid_on_the_device_gives_pillows_rows(hip, photos, pillow_rows):
    """the op-by-op twin of the handle's front end, fed decoded bytes: no image library in the path"""
    from visualcloze_amd import pipeline
    rows, masks = pipeline.preprocess_grid(photos, RES, device_resize=True, device=DEV)
    torch.cuda.synchronize()
    assert len(rows) == len(masks) == 2
    for r, m, wr, wm in zip(rows, masks, *pillow_rows):
        assert same(r, wr) and same(m, wm)


def test_sdedit_u8_is_bit_identical_to_sdedit_on_pillows_intermediate(gh, data, golden):
    cell = torch.from_numpy(golden["up_cell"]).to(DEV)              # 32 x 16 (h x w)
    resized = golden["up_resized"]                                  # Pillow's bicubic resize to 48 x 32 (w x h)
    assert resized.shape == (32, 48, 3)
    px = normalised(resized).to(DEV, torch.bfloat16)
    want, want_off = gh.sdedit([px, px], data["t5_ids"], data["clip_ids"], SEED, 3, cfg=CFG, steps=3, strength=0.4)
    torch.cuda.synchronize()
    got, off = gh.sdedit_u8([cell, cell], (48, 32), data["t5_ids"], data["clip_ids"], SEED, 3, cfg=CFG, steps=3, strength=0.4)
    torch.cuda.synchronize()
    assert off == want_off and len(got) == 2
    assert all(same(g, w) and float(g.std()) > 0 for g, w in zip(got, want))
    counts = (gh.vae.plan_count(), gh.t5.plan_count(), gh.clip.plan_count())
    again, _ = gh.sdedit_u8([cell, cell], (48, 32), data["t5_ids"], data["clip_ids"], SEED, 3, cfg=CFG, steps=3, strength=0.4)
    torch.cuda.synchronize()
    assert (gh.vae.plan_count(), gh.t5.plan_count(), gh.clip.plan_count()) == counts and all(same(a, b) for a, b in zip(again, want))
    # strength >= 1: the resized bytes themselves, nothing drawn
    u8, off1 = gh.sdedit_u8([cell], (48, 32), data["t5_ids"], data["clip_ids"], SEED, 9, steps=3, strength=1.0, uint8=True)
    torch.cuda.synchronize()
    assert off1 == 9 and torch.equal(u8[0].cpu(), torch.from_numpy(resized.copy()))
    with pytest.raises(hip_error(), match="VC_PIXELS_U8"):
        gh.sdedit_u8([cell], (48, 32), data["t5_ids"], data["clip_ids"], SEED, 9, steps=3, strength=1.0)
    with pytest.raises(hip_error(), match="multiples of 16"):
        gh.sdedit_u8([cell], (40, 32), data["t5_ids"], data["clip_ids"], SEED, 9, steps=3)


def hip_error():
    from visualcloze_amd.hip import VclozeHipError
    return VclozeHipError


@pytest.mark.parametrize("use_grid_handle", [True, False], ids=["handle", "ops"])
def test_generate_and_upsample_device_resize_gives_the_same_bits(mods, data, pillow_rows, use_grid_handle):
    """both stages chained with a REAL resize between them (a 16x32 cell to 48x32): the default path resizes with PIL on the host,
    the switch keeps the quantised row on the device and resizes there"""
    from visualcloze_amd import pipeline
    rows, masks = pillow_rows
    outs = {}
    for on in (False, True):
        rng = pipeline.NoiseStream(SEED)
        outs[on] = (pipeline.generate_and_upsample(*mods, rows, masks, data["t5_ids"], data["clip_ids"], SEED, grid_w=2, mask_position=[False, True],
                                                   target_size=(48, 32), cfg=CFG, steps=STEPS, upsampling_steps=3, rng=rng,
                                                   use_grid_handle=use_grid_handle, device_resize=on), rng.offset)
        torch.cuda.synchronize()
    assert outs[True][1] == outs[False][1] and len(outs[True][0]) == len(outs[False][0]) == 1
    assert outs[True][0][0].shape == (3, 32, 48) and same(outs[True][0][0], outs[False][0][0]) and float(outs[True][0][0].std()) > 0


def test_argument_errors_come_before_the_device(hip, gh, data, photos):  # noqa: F811
    with pytest.raises(hip.VclozeHipError, match="absent"):
        gh.generate_photos([[photos[0][0], None], [photos[0][1], None]], RES, data["t5_ids"], data["clip_ids"], SEED)
    with pytest.raises(hip.VclozeHipError, match="n_points"):
        gh.generate_photos(photos, RES, data["t5_ids"], data["clip_ids"], SEED, steps=1)
    with pytest.raises(hip.VclozeHipError, match="multiples of 16"):
        gh.generate_photos([[None]], 40, data["t5_ids"], data["clip_ids"], SEED)          # a blank cell of 40x40 pixels
    # ... and the handle still serves
    got, _ = gh.generate_photos(photos, RES, data["t5_ids"], data["clip_ids"], SEED, 5, cfg=CFG, steps=STEPS, decode_rows=[1], uint8=True)
    torch.cuda.synchronize()
    assert got[0].shape == (16, 64, 3) and got[0].dtype == torch.uint8


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_host_program_goes_from_bytes_to_bytes_bit_identically(hip, gh, mods, data, golden, photos, tmp_path):  # noqa: F811
    """tests/c_abi/photo_demo.c - no Python in its process - against the same two calls made here through ctypes"""
    from tests.photo_demo_build import build_photo_demo, write_handles
    exe = build_photo_demo(tmp_path)
    with open(tmp_path / "in.bin", "wb") as f:
        write_handles(f, gh, mods)
        f.write(struct.pack("<3i", 2, 2, RES))
        for row in photos:
            for t in row:
                if t is None:
                    f.write(struct.pack("<2i", 0, 0))
                else:
                    f.write(struct.pack("<2i", t.shape[0], t.shape[1]) + t.cpu().numpy().tobytes())
        for ids in (data["t5_ids"], data["clip_ids"]):
            a = ids[0].cpu().numpy().astype(np.int32)
            f.write(struct.pack("<i", a.size) + a.tobytes())
        f.write(struct.pack("<2Qf2id", SEED, 5, CFG, STEPS, 0, 1.0))
        f.write(struct.pack("<3id", 48, 32, 3, 0.4))
    row, off = gh.generate_photos(photos, RES, data["t5_ids"], data["clip_ids"], SEED, 5, cfg=CFG, steps=STEPS, decode_rows=[1], uint8=True)
    cell = row[0][:, 32:64].contiguous()
    want, want_off = gh.sdedit_u8([cell], hip.upsampling_size((48, 32)), data["t5_ids"], data["clip_ids"], SEED, off, cfg=CFG, steps=3,
                                  strength=0.4, uint8=True)
    torch.cuda.synchronize()
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint8)
    h, w = (int(v) for v in raw[:8].view(np.int32))
    assert (h, w) == (32, 48) and raw.size == 8 + h * w * 3 + 8
    assert int(raw[8 + h * w * 3:].view(np.uint64)[0]) == want_off
    got = torch.from_numpy(raw[8:8 + h * w * 3].reshape(h, w, 3).copy())
    assert torch.equal(got, want[0].cpu()) and float(got.float().std()) > 0
