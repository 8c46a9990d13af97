"""Euler, midpoint and the Adams-Bashforth orders 2 to 4 at EQUAL model-evaluation counts on one workload of bench.py (default:
configuration 2 of BASELINE.json, 384-grid 2x3, one MI355X), through the C handle (vc_flux_sample_ode / vc_flux_sample_multistep), from
the same start state on the sampler's own time grid: Euler and the multistep orders take E steps, midpoint E / 2.  The yardstick is
an Euler run at 8 E steps.  Each final latent is compared to the yardstick's with `pipeline.compare_images` (PSNR / SSIM, on the
device) - on a RENDERING OF THE LATENT, not a decoded image: channels 0..2 of the unpacked latent row, mapped to [0, 1] by the affine
map that puts the yardstick's range on [0, 1] - and by max |difference|.  Written to profiles/multistep_compare.json.
ONE run on RANDOM-INIT weights: it demonstrates the instrument and describes that vector field, not FLUX.1-Fill's.  No quality claim,
no recommendation of an order, and no threshold on any of these numbers.
    python tools/multistep_compare.py [--workload 384-grid-2x3] [--evals 8] [--out profiles/multistep_compare.json]"""
import argparse
import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from visualcloze_amd import hip, packing, pipeline  # noqa: E402
from visualcloze_amd.transport import solver_time_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--evals", type=int, default=8, help="model evaluations per run (even: midpoint takes evals / 2 steps)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multistep_compare.json"))
    a = ap.parse_args()
    if a.evals < 2 or a.evals % 2:
        ap.error("--evals must be even and at least 2")
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[a.workload]
    model, _ = bench.build_model(dev, 0, 1)
    model.prepare(free_parameters=True)
    x, kw = bench.make_inputs(dev, wl, seed=0, B=1)
    h, st = model.handle(), model.engine().stream
    E = a.evals
    grid = lambda steps: solver_time_grid(steps + 1, x.shape[1], wl.get("t0", 0.0), 1, wl.get("do_shift", True), 1)  # noqa: E731
    runs = [("euler_ref", "euler", 8 * E, 8 * E), ("euler", "euler", E, E), ("midpoint", "midpoint", E // 2, E),
            ("ab2", 2, E, E), ("ab3", 3, E, E), ("ab4", 4, E, E)]
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), weights="random-init", B=1, evaluations=E,
               yardstick="euler at 8x the steps", rendering="channels 0..2 of the unpacked latent, affine map of the yardstick's range to [0, 1]",
               methods={})
    final = {}
    with torch.cuda.stream(st):
        s = st.cuda_stream
        for multistep in (False, True):
            h.set_multistep(multistep)
            try:
                h.prepare(kw["txt"], kw["y"], kw["guidance"], True, kw["img_ids"], kw["txt_ids"], 8 * E, stream=s)
                for name, method, steps, evals in runs:
                    if isinstance(method, int) != multistep:
                        continue
                    xs = x.clone()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if multistep:
                        h.sample_multistep(method, xs, kw["cond"], grid(steps), True, s)
                    else:
                        h.sample_ode(method, xs, kw["cond"], grid(steps), True, s)
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0           # includes the capture of the method's step: one run, not a rate
                    final[name] = xs.float()
                    res["methods"][name] = dict(steps=steps, evaluations=evals, wall_s_with_capture=round(wall, 3),
                                                finite=bool(torch.isfinite(xs.float()).all()))
                    print(f"{name}: {steps} steps, {evals} evaluations, {wall:.1f} s", file=sys.stderr, flush=True)
            finally:
                h.set_multistep(False)
    torch.cuda.synchronize()
    ref = final["euler_ref"]
    hw = [tuple(r) for r in wl["row_latents"]]
    lo, hi = float(ref.min()), float(ref.max())

    def render(z):
        rows = packing.unpack_rows(z, hw)                    # [1, 16, h, w] per grid row
        return [((r[0, :3].float() - lo) / (hi - lo)).clamp_(0.0, 1.0).contiguous() for r in rows]

    want = render(ref)
    for name, z in final.items():
        m = pipeline.compare_images(render(z), want)
        res["methods"][name].update(max_abs_diff_to_ref=float((z - ref).abs().max()),
                                    psnr_db=[r["psnr_db"] if math.isfinite(r["psnr_db"]) else None for r in m],   # identical: null
                                    ssim=[r["ssim"] for r in m])
    res["final_latent_range"] = [lo, hi]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
