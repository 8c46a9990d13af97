"""The stage boundary of generate_and_upsample, host against device, in ONE process: from the decoded last row of a two-cell
grid, f32 [3, 384, 768] in [0, 1] on the device, to the bf16 [3, 1024, 1024] tensor the SDEdit stage encodes for its second cell.
Both sides are the statements `pipeline.generate_and_upsample` / `upsample_images` run between the stages, with the pipeline's
own helpers; the functions themselves are not called (everything else in them is the model):

    host    the default path: `to_uint8_image` (quantise, bytes to the host), PIL crop, PIL bicubic resize, ToTensor / Normalize on
            the CPU, bf16 to the device
    device  device_resize=True: `_u8_tensor` (quantise on the device), the cell's column window made dense, vc_resample_u8,
            vc_pixels_in

Wall time per boundary with the device synchronised before and after, median and min of --reps after --warmup; the two results
are compared bit for bit first.  python tools/stage_boundary.py [--cell 384] [--target 1024] [--reps 30]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from visualcloze_amd import hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=384)
    ap.add_argument("--target", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    hip.require_gpu()
    dev = "cuda:0"
    from visualcloze_amd import pipeline
    g = torch.Generator().manual_seed(1)
    row = torch.rand(3, a.cell, 2 * a.cell, generator=g).to(dev)       # the decoded last row, two cells
    size = (a.target, a.target)
    x0, x1 = a.cell, 2 * a.cell

    def host():
        img = pipeline.to_uint8_image(row).crop((x0, 0, x1, a.cell)).convert("RGB").resize(size)
        px = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
        return ((px - 0.5) / 0.5).to(dev, torch.bfloat16)

    def device():
        cell = pipeline._u8_tensor(row)[:, x0:x1].contiguous()
        return hip.pixels_in(hip.resample_u8(cell, size), size)

    assert torch.equal(host(), device())
    out = {"cell": a.cell, "target": a.target, "reps": a.reps}
    for name, fn in (("host", host), ("device", device)):
        ms = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms_median"], out[name + "_ms_min"] = round(statistics.median(ms), 4), round(min(ms), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
