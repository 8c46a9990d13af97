"""What the three adaptive solves cost on the flagship workload (configuration 2 of BASELINE.json: 384-grid 2x3, one MI355X): ONE run
each of dopri5, bosh3 and adaptive_heun through the C handle (vc_flux_sample_dopri5 / vc_flux_sample_rk) at the same rtol / atol, from
the same start state, to the same 30 output times - attempts, rejected attempts, model evaluations, wall seconds, and max |difference|
of each final latent to a dopri5 run at a tight tolerance.  The weights are RANDOM-INIT: every count describes that vector field, not
FLUX.1-Fill's.  Measured, not claimed: no threshold is set on any of these numbers.
    python tools/adaptive_compare.py [--workload 384-grid-2x3] [--rtol 1e-3] [--atol 1e-6] [--ref-rtol 1e-6] [--outputs 30]"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from visualcloze_amd import hip  # noqa: E402
from visualcloze_amd.transport import solver_time_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--atol", type=float, default=1e-6)
    ap.add_argument("--ref-rtol", type=float, default=1e-6)
    ap.add_argument("--outputs", type=int, default=30)
    ap.add_argument("--max-attempts", type=int, default=4000)
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[a.workload]
    model, _ = bench.build_model(dev, 0, 1)
    model.prepare(free_parameters=True)
    x, kw = bench.make_inputs(dev, wl, seed=0, B=1)
    h, st = model.handle(), model.engine().stream
    t = solver_time_grid(a.outputs + 1, x.shape[1], wl.get("t0", 0.0), 1, wl.get("do_shift", True), 1)
    runs = [("dopri5_ref", "dopri5", a.ref_rtol), ("dopri5", "dopri5", a.rtol), ("bosh3", "bosh3", a.rtol),
            ("adaptive_heun", "adaptive_heun", a.rtol)]
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), weights="random-init", B=1, outputs=a.outputs, rtol=a.rtol,
               atol=a.atol, ref_rtol=a.ref_rtol, evaluations_per_attempt=dict(dopri5=6, bosh3=3, adaptive_heun=2), methods={})
    final = {}
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.set_adaptive(True)
        try:
            h.prepare(kw["txt"], kw["y"], kw["guidance"], True, kw["img_ids"], kw["txt_ids"], 7, stream=s)
            for name, method, rtol in runs:
                failed = None
                for timed in (False, True):                # a one-attempt call captures the method's step; the second call is measured
                    xs = x.clone()
                    traj = torch.empty(a.outputs, *x.shape, dtype=x.dtype, device=dev)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    limit = a.max_attempts if timed else 1
                    try:
                        if method == "dopri5":
                            h.sample_dopri5(xs, kw["cond"], t, True, s, rtol, a.atol, limit, trajectory=traj)
                        else:
                            h.sample_rk(method, xs, kw["cond"], t, True, s, rtol, a.atol, limit, trajectory=traj)
                    except hip.VclozeHipError as e:        # recorded, not hidden: e.g. more than max_attempts attempts
                        if not timed:
                            continue                       # the warm-up is meant to stop after its first attempt
                        failed = str(e)
                        break
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                log = h.rk_log()
                if failed is not None:
                    res["methods"][name] = dict(rtol=rtol, error=failed, attempts=len(log["attempts"]), evaluations=log["evaluations"])
                    continue
                final[name] = xs.float()
                print(f"{name}: {len(log['attempts'])} attempts, {log['evaluations']} evaluations, {wall:.1f} s", file=sys.stderr, flush=True)
                res["methods"][name] = dict(rtol=rtol, attempts=len(log["attempts"]), rejected=log["rejected"], evaluations=log["evaluations"],
                                            wall_s=round(wall, 3), finite=bool(torch.isfinite(xs.float()).all()))
        finally:
            h.set_adaptive(False)
    torch.cuda.synchronize()
    if "dopri5_ref" in final:
        for name in final:
            res["methods"][name]["max_abs_diff_to_ref"] = float((final[name] - final["dopri5_ref"]).abs().max())
        res["final_latent_absmax"] = float(final["dopri5_ref"].abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
