"""Generate tests/golden/resample_golden.npz: what Pillow and the REFERENCE's own size rules give for the photo front end
(vc_resample_u8, vc_fit_size, vc_grid_layout, vc_upsampling_size, vc_grid_generate_photos, vc_grid_sdedit_u8).  Runs only where the
reference tree (VC_REFERENCE) and Pillow are; only the vectors travel.  The reference's `visualcloze` module is imported with its
absent dependencies stubbed; what is called are its own `resize_with_aspect_ratio`, `center_crop` and - for the upsampling size -
`VisualClozeModel.upsampling` with upsampling_noise = 1.0, which returns right after its `Image.resize` (visualcloze.py:166-182).
The grid loop is `VisualClozeModel.process_images` itself (:247-374), run with a stub `self` whose `image_transform` keeps the
processed images and stops the method before it reaches the model; `reference_grid` below only watches what it calls.

    rs_shapes [n, 4]            (W, H, w, h) of the resampling cases
    rs_in_<i>                   seeded random uint8 [H, W, 3]
    rs_bicubic_<i>, rs_lanczos_<i>   PIL.Image.resize((w, h), BICUBIC / LANCZOS) of it
    fit_in [m, 3], fit_out [m, 2]     (w, h, resolution) -> the size resize_with_aspect_ratio returns
    ups_in [k, 2], ups_out [k, 2]     target_size (0, 0 = None) -> the size `upsampling` resizes to; (-1, -1) where it raises
    lay_<c>_sizes [gh, gw, 2], lay_<c>_res, lay_<c>_plan [gh * gw, 12] (VcCellPlan's fields; absent where the reference raises),
    lay_<c>_ok                  the layout cases
    photo_<j>                   the photographs of the handle test (40x56 and 70x50 pixels), photo_cell_<k> the four cells of the
                                2x2 grid at resolution 32 as Pillow makes them (the absent one black)
    up_cell, up_resized         a 16x32 cell and its bicubic resize to 48x32 (w x h)

    python tests/golden/make_resample_golden.py     # rewrites tests/golden/resample_golden.npz
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("VC_REFERENCE", "/root/reference")

RS_SHAPES = [(37, 53, 16, 32), (48, 80, 112, 64), (301, 203, 96, 64), (64, 64, 64, 48), (50, 70, 160, 224), (97, 33, 16, 16),
             (16, 16, 16, 16), (1, 1, 16, 16), (16, 16, 1, 1), (333, 17, 16, 48)]


def import_reference():
    class _Any(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return _Any(self.__name__ + "." + name)

        def __call__(self, *a, **k):
            return None
    for name in ("einops", "diffusers", "diffusers.models", "torchvision", "torchvision.transforms", "torchvision.transforms.functional",
                 "models", "models.sampling", "models.util", "transport", "util", "util.imgproc"):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = _Any(name)
    sys.path.insert(0, REFERENCE)
    import visualcloze
    return visualcloze


class _Stop(Exception):
    pass


def reference_grid(vc, images, resolution):
    """The reference's own `VisualClozeModel.process_images` (:247-374) run on `images` up to the point where it would touch the
    model: `self` is a stub that carries the grid size and the resolution, and its `image_transform` keeps every processed PIL
    image and stops the method at the last one.  What the method does on the way is only WATCHED - the sizes its calls of
    `resize_with_aspect_ratio` return, the image and the target size each `center_crop` call receives with the box that call crops,
    the size of every blank it makes - nothing of it is restated here.  Returns (processed cells, VcCellPlan rows); raises what the
    method raises."""
    import torch
    from PIL import Image
    gh, gw = len(images), len(images[0])
    cells, events, fits = [], [], []

    def transform(img):
        cells.append(img.copy())
        if len(cells) == gh * gw:
            raise _Stop()
        return torch.zeros(3, img.height, img.width)

    real_fit, real_centre, real_crop, real_new = vc.resize_with_aspect_ratio, vc.center_crop, Image.Image.crop, Image.new

    def fit(*a, **k):
        out = real_fit(*a, **k)
        fits.append(out.size)
        return out

    def centre(image, size):
        boxes = []

        def crop(self, box=None):
            boxes.append(box)
            return real_crop(self, box)
        Image.Image.crop = crop
        try:
            out = real_centre(image, size)
        finally:
            Image.Image.crop = real_crop
        events.append([1, *fits[-1], *image.size, boxes[0][0], boxes[0][1], *out.size, 0, 0, 0])
        return out

    def new(mode, size, *a, **k):
        events.append([0, 0, 0, 0, 0, 0, 0, *size, 0, 0, 1])
        return real_new(mode, size, *a, **k)

    stub = types.SimpleNamespace(sampler=types.SimpleNamespace(sample_ode=lambda **k: None), solver="euler", atol=1e-6, rtol=1e-3,
                                 time_shifting_factor=1, grid_h=gh, grid_w=gw, resolution=resolution, dtype=torch.bfloat16, device="cpu",
                                 image_transform=transform)
    vc.resize_with_aspect_ratio, vc.center_crop, Image.new = fit, centre, new
    try:
        vc.VisualClozeModel.process_images(stub, [list(r) for r in images], ["", "", ""], seed=1)
    except _Stop:
        pass
    finally:
        vc.resize_with_aspect_ratio, vc.center_crop, Image.new = real_fit, real_centre, real_new
    assert len(cells) == len(events) == gh * gw
    for c, p in zip(cells, events):
        p[9], p[10] = c.size
    return cells, events


def main():
    from PIL import Image
    vc = import_reference()
    rng = np.random.default_rng(20240607)
    out = {"rs_shapes": np.asarray(RS_SHAPES, np.int32)}
    for i, (W, H, w, h) in enumerate(RS_SHAPES):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out[f"rs_in_{i}"] = a
        out[f"rs_bicubic_{i}"] = np.asarray(Image.fromarray(a).resize((w, h), Image.BICUBIC))
        out[f"rs_lanczos_{i}"] = np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))

    # the size rules: about 200 seeded sizes - non-square, tiny, large - at several resolutions
    sizes = [(640, 480, 384), (480, 640, 384), (5, 9, 384), (15, 15, 32), (3, 200, 64), (1600, 1200, 384), (1, 1, 16), (4000, 30, 160)]
    while len(sizes) < 200:
        w, h = (int(v) for v in rng.integers(1, 1400, 2))
        sizes.append((w, h, int(rng.choice([16, 32, 64, 160, 256, 384, 512]))))
    out["fit_in"] = np.asarray(sizes, np.int32)
    out["fit_out"] = np.asarray([vc.resize_with_aspect_ratio(Image.new("L", (w, h)), r).size for w, h, r in sizes], np.int32)
    ups = [(0, 0), (1024, 1024), (1025, 1024), (2000, 1500), (1500, 2000), (4000, 300), (40, 56), (70, 50), (8, 8), (1024, 1040)]
    ups += [tuple(int(v) for v in rng.integers(1, 3000, 2)) for _ in range(60)]
    res = []
    for w, h in ups:
        try:
            res.append(vc.VisualClozeModel.upsampling(None, Image.new("L", (16, 16)), None if (w, h) == (0, 0) else (w, h), 0, 0, 1.0, None, "").size)
        except ValueError:                          # a side of 0: Pillow refuses the resize, nothing is recorded
            res.append((-1, -1))
    out["ups_in"], out["ups_out"] = np.asarray(ups, np.int32), np.asarray(res, np.int32)

    # layouts: plain, portrait against landscape (crop), an image smaller than its row's reference size (negative crop), two
    # masked cells (second pass), no image in the last row (384), the second pass that comes to nothing (an error), a missing
    # in-context image (an error)
    layouts = [
        ([[(40, 56), (70, 50)], [(70, 50), None]], 32),
        ([[(640, 480), (300, 500)], [(500, 400), None]], 96),
        ([[(300, 100), (40, 300)], [(40, 300), None]], 64),
        ([[(100, 60), (30, 90), (64, 64)], [(90, 40), None, None]], 48),
        ([[(50, 50), (60, 40)], [None, None]], 32),
        ([[(4000, 30), (4000, 30)], [(64, 64), None]], 160),
        ([[(4000, 30), (4000, 30), (4000, 30)], [(64, 64), None, None]], 160),
        ([[(50, 50), None], [(60, 40), None]], 32),
        ([[(37, 91)]], 64), ([[None]], 32),
        ([[(40, 300), (64, 64)], [(40, 300), None]], 64), ([[(40, 300), (30, 40)], [(64, 64), None]], 64),
    ]
    for c, (sz, r) in enumerate(layouts):
        imgs = [[None if s is None else Image.new("RGB", s) for s in row] for row in sz]
        out[f"lay_{c}_sizes"] = np.asarray([[(0, 0) if s is None else s for s in row] for row in sz], np.int32)
        out[f"lay_{c}_res"] = np.int32(r)
        try:
            _, plans = reference_grid(vc, imgs, r)
            out[f"lay_{c}_ok"], out[f"lay_{c}_plan"] = np.int32(1), np.asarray(plans, np.int32)
        except ValueError:                          # what the reference raises: a missing in-context image, a resize to nothing
            out[f"lay_{c}_ok"] = np.int32(0)
    out["lay_count"] = np.int32(len(layouts))

    photos = [rng.integers(0, 256, (56, 40, 3), dtype=np.uint8), rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)]
    pil = [Image.fromarray(p) for p in photos]
    cells, _ = reference_grid(vc, [[pil[0], pil[1]], [pil[1], None]], 32)
    for j, p in enumerate(photos):
        out[f"photo_{j}"] = p
    for k, cimg in enumerate(cells):
        out[f"photo_cell_{k}"] = np.asarray(cimg)
    cell = rng.integers(0, 256, (32, 16, 3), dtype=np.uint8)
    out["up_cell"] = cell
    out["up_resized"] = np.asarray(vc.VisualClozeModel.upsampling(None, Image.fromarray(cell), (48, 32), 0, 0, 1.0, None, ""))
    path = os.path.join(HERE, "resample_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
