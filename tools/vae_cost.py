"""What the autoencoder handle (vc_vae_decode / vc_vae_encode: the launch plan of csrc/vae_engine.hip as ONE hipGraph launch) costs
beside the Python-ordered plan of visualcloze_amd/vae.py (the same kernels issued launch by launch from Python) at a workload's
row-image size: ms per decode and per encode of one row, FLUX AutoEncoder geometry with procedural weights, in ONE process on one
box - HIP events around whole calls on one stream, the two paths interleaved round by round (boxes differ more than code does -
README), one warm round first (it captures the plans), with the board's power and clock during the timed rounds.  The outputs of
the two paths are compared bit for bit.  No threshold: the handle is kept for the capability; this records the difference.
    python tools/vae_cost.py [--workload 384-grid-2x3] [--rounds 7] [--calls 3]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from tests.procedural import procedural_ae_param, ptensor_torch  # noqa: E402
from visualcloze_amd import hip  # noqa: E402
from visualcloze_amd.board import BoardSampler, pci_bus_id_of  # noqa: E402
from visualcloze_amd.vae import FLUX_AE, AutoEncoder, AutoEncoderParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="384-grid-2x3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    h, w = bench.WORKLOADS[a.workload]["row_latents"][0]
    H, W = 8 * h, 8 * w
    ae = AutoEncoder(AutoEncoderParams(**FLUX_AE))
    ae.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in ae.state_dict().items()})
    ae = ae.to(dev).to(torch.bfloat16)
    z = ptensor_torch((1, 16, h, w), 21, q=5, kmax=96, device=dev, dtype=torch.bfloat16)
    img = ptensor_torch((1, 3, H, W), 41, q=7, kmax=127, device=dev, dtype=torch.bfloat16)
    noise = ptensor_torch((1, 16, h, w), 43, q=5, kmax=80, device=dev, dtype=torch.bfloat16)
    hd = ae.handle()
    st = torch.cuda.Stream(dev)

    def python_decode():
        return ae.decode(z)[0]

    def python_encode():
        return ae.encode(img, noise=noise)[0]

    def handle_decode():
        return hd.decode(z[0])

    def handle_encode():
        return hd.encode(img[0], noise=noise[0])

    legs = (("decode", "python", python_decode), ("decode", "handle", handle_decode),
            ("encode", "python", python_encode), ("encode", "handle", handle_encode))
    ms = {(op, path): [] for op, path, _ in legs}
    out = {}
    board = BoardSampler(pci_bus_id_of(0), index=0, hz=10.0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(st):
        for r in range(a.rounds + 1):                 # round 0 warms every kernel, captures the two plans and warms the clocks
            if r == 1:
                board.__enter__()
            for op, path, fn in legs:
                ev[0].record(st)
                for _ in range(a.calls):
                    out[(op, path)] = fn()
                ev[1].record(st)
                ev[1].synchronize()
                if r:
                    ms[(op, path)].append(ev[0].elapsed_time(ev[1]) / a.calls)
        board.__exit__(None, None, None)
    torch.cuda.synchronize()
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), image=[H, W], latent=[h, w], rounds=a.rounds, calls_per_window=a.calls,
               captured_plans=hd.plan_count(), decoder_workspace_bytes=hd.workspace_bytes(H, W, hip.VAE_DECODER),
               encoder_workspace_bytes=hd.workspace_bytes(H, W, hip.VAE_ENCODER))
    for op in ("decode", "encode"):
        same = bool(torch.equal(out[(op, "python")], out[(op, "handle")]))
        assert same and torch.isfinite(out[(op, "handle")].float()).all(), op
        med = {p: statistics.median(ms[(op, p)]) for p in ("python", "handle")}
        res[op] = {p: dict(ms_median=round(med[p], 3), ms_min=round(min(ms[(op, p)]), 3), ms_max=round(max(ms[(op, p)]), 3))
                   for p in ("python", "handle")}
        res[op]["handle_over_python_pct"] = round(100 * (med["handle"] / med["python"] - 1), 2)
        res[op]["python_spread_pct"] = round(100 * (max(ms[(op, "python")]) / min(ms[(op, "python")]) - 1), 2)
        res[op]["bit_identical"] = same
    b = board.summary()
    res["board"] = {k: b.get(k) for k in ("power_w_avg", "power_cap_w", "sclk_mhz_avg", "source")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
