"""ms per SOLVER STEP of the fused loop for "euler", "midpoint" and "rk4" on one workload, in ONE process on one box: HIP events
around `vc_flux_sample_steps(n)` on the engine stream, the methods interleaved round by round, next to E x the Euler step of the
same build (boxes differ more than code does - README).  The expectation is E x Euler plus microseconds for the vc_ode_stage
launches; more than ~1 % above it means the stage boundary broke the graph replay.
    python tools/solver_cost.py [--workload 384-grid-2x3] [--steps 6] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from visualcloze_amd import hip  # noqa: E402
from visualcloze_amd.transport import solver_time_grid  # noqa: E402

METHODS = ("euler", "midpoint", "rk4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--steps", type=int, default=6, help="solver steps per timed call")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[a.workload]
    model, _ = bench.build_model(dev, 0, 1)
    model.prepare(free_parameters=True)
    x, kw = bench.make_inputs(dev, wl, seed=0)
    h, st = model.handle(), model.engine().stream
    S = a.steps + 1                                   # one warm step, then the timed ones
    t = solver_time_grid(S + 1, x.shape[1], wl.get("t0", 0.0), 1, wl.get("do_shift", True), 1)
    ms = {m: [] for m in METHODS}
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(kw["txt"], kw["y"], kw["guidance"], True, kw["img_ids"], kw["txt_ids"], S * 4, stream=s)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for r in range(a.rounds + 1):                 # round 0 captures the three graphs and warms the clocks
            for m in METHODS:
                h.sample_begin(x, kw["cond"], t, True, s, method=m)
                h.sample_steps(1, s)
                ev[0].record(st)
                h.sample_steps(a.steps, s)
                ev[1].record(st)
                ev[1].synchronize()
                if r:
                    ms[m].append(ev[0].elapsed_time(ev[1]) / a.steps)
        out = torch.empty_like(x)
        h.sample_end(out, s)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    med = {m: statistics.median(v) for m, v in ms.items()}
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), steps_per_call=a.steps, rounds=a.rounds)
    for m in METHODS:
        E = hip.solver_evals(m)
        res[m] = dict(evals_per_step=E, ms_per_step_median=round(med[m], 3), ms_per_step_min=round(min(ms[m]), 3),
                      ms_per_step_max=round(max(ms[m]), 3), E_x_euler_ms=round(E * med["euler"], 3),
                      over_E_x_euler_pct=round(100 * (med[m] / (E * med["euler"]) - 1), 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
