"""What true CFG (vc_flux_set_cfg: one more launch per evaluation, vc_cfg_combine over the velocity's two halves) costs in the fused
loop: steps/s of a B = 2 Euler trajectory with CFG on and off, in ONE process on one box - HIP events around
`vc_flux_sample_steps(n)` on the engine stream, the two settings interleaved round by round (boxes differ more than code does -
README) - with the board's power and clock during the rounds.  The combine moves 3 * (B/2) * N * 128 bytes per evaluation.
    python tools/cfg_cost.py [--workload 384-grid-2x3] [--steps 6] [--rounds 5] [--cfg-scale 3.5]"""
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
from visualcloze_amd.board import BoardSampler, pci_bus_id_of  # noqa: E402
from visualcloze_amd.transport import solver_time_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--steps", type=int, default=6, help="solver steps per timed call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfg-scale", type=float, default=3.5)
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[a.workload]
    model, _ = bench.build_model(dev, 0, 1)
    model.prepare(free_parameters=True)
    x, kw = bench.make_inputs(dev, wl, seed=0, B=2)   # sample 0 conditional, sample 1 unconditional
    h, st = model.handle(), model.engine().stream
    S = a.steps + 1                                   # one warm step, then the timed ones
    t = solver_time_grid(S + 1, x.shape[1], wl.get("t0", 0.0), 1, wl.get("do_shift", True), 1)
    settings = (("off", None), ("on", a.cfg_scale))
    ms = {name: [] for name, _ in settings}
    board = BoardSampler(pci_bus_id_of(0), index=0, hz=10.0)
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(kw["txt"], kw["y"], kw["guidance"], True, kw["img_ids"], kw["txt_ids"], S, stream=s)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        out = {}
        for r in range(a.rounds + 1):                 # round 0 captures the two graphs and warms the clocks
            if r == 1:
                board.__enter__()
            for name, scale in settings:
                h.set_cfg(scale)
                h.sample_begin(x, kw["cond"], t, True, s)
                h.sample_steps(1, s)
                ev[0].record(st)
                h.sample_steps(a.steps, s)
                ev[1].record(st)
                ev[1].synchronize()
                if r:
                    ms[name].append(ev[0].elapsed_time(ev[1]) / a.steps)
                out[name] = torch.empty_like(x)
                h.sample_end(out[name], s)
        board.__exit__(None, None, None)
        h.set_cfg(None)
    torch.cuda.synchronize()
    assert all(torch.isfinite(o.float()).all() for o in out.values())
    assert torch.equal(out["on"][1], out["off"][1]) and not torch.equal(out["on"][0], out["off"][0])   # only the conditional half moves
    med = {k: statistics.median(v) for k, v in ms.items()}
    N = x.shape[1]
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), B=2, steps_per_call=a.steps, rounds=a.rounds,
               cfg_scale=a.cfg_scale, combine_bytes_per_evaluation=3 * N * 64 * 2)
    for k in ms:
        res[k] = dict(ms_per_step_median=round(med[k], 3), ms_per_step_min=round(min(ms[k]), 3), ms_per_step_max=round(max(ms[k]), 3),
                      steps_per_s=round(1e3 / med[k], 3))
    res["on_over_off_pct"] = round(100 * (med["on"] / med["off"] - 1), 3)
    res["off_spread_pct"] = round(100 * (max(ms["off"]) / min(ms["off"]) - 1), 3)
    b = board.summary()
    res["board"] = {k: b.get(k) for k in ("power_w_avg", "power_cap_w", "sclk_mhz_avg", "source")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
