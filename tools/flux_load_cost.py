#!/usr/bin/env python3
"""What preparing the weights costs, three ways, at the bench's full geometry (FLUX.1-Fill-dev, 19 + 38 blocks, LoRA rank 256, random
init): vc_flux_load_finish (the library alone: one vc_lora_merge_qkv launch per Linear, the scale launch, one read-back) against
Flux.prepare() with lora_merge="hip" and with lora_merge="torch".  Wall time, the device synchronised either side; the first run of
each route is reported apart from the best of the following ones (kernel attributes, allocator).  A measurement, not a gate.

    python tools/flux_load_cost.py [--repeat 3] [--tiny] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_model(dev, rank, params):
    from visualcloze_amd.model import FluxLoraWrapper, FluxParams
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("meta"):
            model = FluxLoraWrapper(lora_rank=rank, lora_scale=1.0, params=FluxParams(**params))
    finally:
        torch.set_default_dtype(old)
    model.to_empty(device=dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("norm.scale"):
                p.fill_(1.0)
            elif name.endswith(".bias"):
                p.zero_()
            else:
                p.normal_(0.0, 0.02, generator=g)
    return model


def timed(fn, dev) -> float:
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the tests' tiny geometry (a dry run of the tool)")
    ap.add_argument("--rank", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from visualcloze_amd import hip
    from visualcloze_amd.handle import FluxHandle
    from visualcloze_amd.model import FLUX_DEV_FILL
    hip.require_gpu()
    dev = torch.device("cuda:0")
    params = dict(FLUX_DEV_FILL)
    if a.tiny:
        params.update(vec_in_dim=64, context_in_dim=128, hidden_size=256, num_heads=2, depth=2, depth_single_blocks=2)
    model = build_model(dev, a.rank, params)
    rec = {"geometry": "tiny" if a.tiny else "FLUX.1-Fill-dev 19+38", "rank": a.rank, "device": torch.cuda.get_device_name(dev),
           "cus": hip.device_cus(dev), "repeat": a.repeat}
    try:
        from visualcloze_amd.board import BoardSampler, pci_bus_id_of
        with BoardSampler(pci_bus_id_of(0), index=0, hz=10.0) as board:
            rec.update(measure(model, a, dev, FluxHandle))
        rec["board"] = board.summary()
    except ImportError:
        rec.update(measure(model, a, dev, FluxHandle))
    b = rec.get("board") or {}
    print(f"board: {rec['device']}, {rec['cus']} CUs, power avg {b.get('power_w_avg')} W, cap {b.get('power_cap_w')} W, "
          f"sclk avg {b.get('sclk_mhz_avg')} MHz ({b.get('source')})")
    for k in ("load_finish", "prepare_hip", "prepare_torch"):
        print(f"{k:14s} first {rec[k]['first_ms']:9.1f} ms   best of {a.repeat} after {rec[k]['best_ms']:9.1f} ms")
    print(json.dumps(rec))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


def measure(model, a, dev, FluxHandle) -> dict:
    out = {}
    box = {}
    sd = model.state_dict()
    first = timed(lambda: box.update(h=FluxHandle.from_state_dict(model.params, sd, 1.0, dev)), dev)
    h = box.pop("h")
    runs = [timed(lambda: h.reload(1.0), dev) for _ in range(a.repeat)]
    out["load_finish"] = {"first_ms": first, "best_ms": min(runs), "arena_gb": h._arena.numel() / 1e9,
                          "note": "first = from_state_dict: every vc_flux_load_tensor, the arena's allocation, the first vc_flux_load_finish "
                                  "and the torch views; after = vc_flux_load_finish alone, into the same arena"}
    del h
    torch.cuda.empty_cache()
    for backend in ("hip", "torch"):
        model.lora_merge = backend
        runs = []
        for _ in range(a.repeat + 1):
            model.invalidate_engine()
            torch.cuda.empty_cache()
            runs.append(timed(model.prepare, dev))
        out["prepare_" + backend] = {"first_ms": runs[0], "best_ms": min(runs[1:])}
    return out


if __name__ == "__main__":
    main()
