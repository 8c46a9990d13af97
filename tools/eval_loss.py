"""The flow-matching validation loss (Transport.training_losses, fused: vc_flux_eval_loss) as an instrument: the loss of ONE geometry at
one fixed (t-set, seed) on bench.py's RANDOM-INIT model under the numerics switches whose effect on the model was so far unmeasured -
lora_merge "torch" vs "hip", merged vs lora_mode "ref" (run by the handle), bounded vs running-max attention softmax.  (The step cache
does not enter: the loss is a single evaluation.)  Random-init weights: the table demonstrates the instrument and makes no quality claim.
With --timing also vc_flux_eval_loss against vc_flux_forward, back to back in ONE process: HIP events, the two calls interleaved round by
round, with the board's power and clock during the rounds.
    python tools/eval_loss.py [--workload 384-grid-2x3] [--times 0.1,0.35,0.6,0.85] [--seed 1234] [--timing] [--rounds 10]"""
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
from visualcloze_amd.pipeline import NoiseStream  # noqa: E402
from visualcloze_amd.transport import create_transport  # noqa: E402

SETTINGS = (          # name, lora_merge, lora_mode, bounded softmax
    ("merged, lora_merge=torch, bounded softmax", "torch", "merged", True),
    ("merged, lora_merge=torch, running-max softmax", "torch", "merged", False),
    ("merged, lora_merge=hip, bounded softmax", "hip", "merged", True),
    ("lora_mode=ref (handle), bounded softmax", "torch", "ref", True),
)


def losses(model, x, kw, times, seed):
    tr = create_transport()
    loss_kw = {k: v for k, v in kw.items() if k != "cond"}
    out = []
    for i, t in enumerate(times):
        rng = NoiseStream(seed, i * x.numel(), device=x.device)
        terms = tr.training_losses(model.forward, x, loss_kw, {"cond": kw["cond"]}, t=torch.tensor([t]), rng=rng)
        out.append(float(terms["loss"][0]))
    return out


def timing(model, x, kw, rounds):
    h, st = model.handle(), model.plan().stream
    img = torch.cat((x, kw["cond"]), dim=-1).contiguous()
    out = torch.empty_like(x)
    ms = {"forward": [], "eval_loss": []}
    board = BoardSampler(pci_bus_id_of(0), index=0, hz=10.0)
    h.set_eval_loss(True)
    try:
        with torch.cuda.stream(st):
            s = st.cuda_stream
            h.prepare(kw["txt"], kw["y"], kw["guidance"], True, kw["img_ids"], kw["txt_ids"], 1, stream=s)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for r in range(rounds + 2):               # two warm rounds: kernel attributes, clocks
                if r == 2:
                    board.__enter__()
                ev[0].record(st)
                h.forward(img, [0.5], True, out, stream=s)
                ev[1].record(st)
                loss = h.eval_loss(x, kw["cond"], [0.5], seed=1, offset=0, stream=s)
                ev[2].record(st)
                ev[2].synchronize()
                if r >= 2:
                    ms["forward"].append(ev[0].elapsed_time(ev[1]))
                    ms["eval_loss"].append(ev[1].elapsed_time(ev[2]))
            board.__exit__(None, None, None)
    finally:
        h.set_eval_loss(False)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {k: dict(ms_median=round(med[k], 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3)) for k, v in ms.items()}
    res["eval_loss_over_forward"] = round(med["eval_loss"] / med["forward"], 4)
    res["forward_spread_pct"] = round(100 * (max(ms["forward"]) / min(ms["forward"]) - 1), 3)
    b = board.summary()
    res["board"] = {k: b.get(k) for k in ("power_w_avg", "power_cap_w", "sclk_mhz_avg", "source")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--times", default="0.1,0.35,0.6,0.85")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[a.workload]
    times = [float(v) for v in a.times.split(",")]
    model, _ = bench.build_model(dev, 0, 1)
    x, kw = bench.make_inputs(dev, wl, seed=0, B=1)
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), weights="random-init (bench.build_model)", times=times,
               seed=a.seed, tokens=x.shape[1], settings=[])
    for name, merge, mode, bounded in SETTINGS:
        if (merge, mode) != (model.lora_merge, model.lora_mode):
            model.lora_merge, model.lora_mode, model.ref_plan = merge, mode, "handle"
            model.invalidate_engine()
        model.engine().bounded_softmax = bounded
        ls = losses(model, x, kw, times, a.seed)
        res["settings"].append(dict(name=name, loss=[round(v, 6) for v in ls], mean=round(sum(ls) / len(ls), 6)))
        print(f"{name:50s} " + " ".join(f"{v:.6f}" for v in ls) + f"   mean {sum(ls) / len(ls):.6f}", flush=True)
        if a.timing and name == SETTINGS[0][0]:
            res["timing"] = timing(model, x, kw, a.rounds)
            print(json.dumps(res["timing"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
