"""ms per Euler step of the fused loop with the first-block step cache off, on but never reusing, and reusing every
step, on one workload (cfg 2 by default), in ONE process on one box: HIP events around `vc_flux_sample_steps(n)` on the engine
stream, the three legs interleaved round by round (boxes differ more than code does - README).
  off     one graph replay per step, no host read;
  never   threshold below every metric: head graph + host read + tail-compute graph, i.e. the full evaluation plus what the cache
          costs when it never pays - the head / tail split, one stream synchronisation and five elementwise passes over N * D;
  reused  threshold inf, no limit: after the first step every step is head + tail-reuse - img_in, double block 0, the metric, the
          residual apply, the last layer and the Euler update.
The cache changes results; this tool measures time only.
    python tools/step_cache_rate.py [--workload 384-grid-2x3] [--steps 6] [--rounds 5]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from visualcloze_amd import hip  # noqa: E402
from visualcloze_amd.transport import StepCache, solver_time_grid  # noqa: E402

LEGS = {"off": None, "never": StepCache(1e-30, -1), "reused": StepCache(math.inf, -1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--steps", type=int, default=6, help="Euler steps per timed call")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[a.workload]
    model, _ = bench.build_model(dev, 0, 1)
    model.prepare(free_parameters=True)
    x, kw = bench.make_inputs(dev, wl, seed=0)
    h, st = model.handle(), model.engine().stream
    S = a.steps + 1                                   # one warm step (it always computes), then the timed ones
    t = solver_time_grid(S + 1, x.shape[1], wl.get("t0", 0.0), 1, wl.get("do_shift", True), 1)
    ms = {leg: [] for leg in LEGS}
    counts = {}
    with torch.cuda.stream(st):
        s = st.cuda_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        out = torch.empty_like(x)
        for r in range(a.rounds + 1):                 # round 0 captures the graphs and warms the clocks
            for leg, cache in LEGS.items():
                h.set_step_cache(cache)               # the workspace differs with the cache on: prepare per leg, outside the timing
                h.prepare(kw["txt"], kw["y"], kw["guidance"], True, kw["img_ids"], kw["txt_ids"], S, stream=s)
                h.sample_begin(x, kw["cond"], t, True, s)
                h.sample_steps(1, s)
                ev[0].record(st)
                h.sample_steps(a.steps, s)
                ev[1].record(st)
                ev[1].synchronize()
                if r:
                    ms[leg].append(ev[0].elapsed_time(ev[1]) / a.steps)
                stats = h.step_cache_stats(S)
                counts[leg] = (stats["computed"], stats["reused"])
                h.sample_end(out, s)
        h.set_step_cache(None)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert counts == {"off": (S, 0), "never": (S, 0), "reused": (1, S - 1)}, counts
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), steps_per_call=a.steps, rounds=a.rounds)
    off = statistics.median(ms["off"])
    for leg in LEGS:
        med = statistics.median(ms[leg])
        res[leg] = dict(ms_per_step_median=round(med, 3), ms_per_step_min=round(min(ms[leg]), 3), ms_per_step_max=round(max(ms[leg]), 3),
                        vs_off_pct=round(100 * (med / off - 1), 2), computed_reused=counts[leg])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
