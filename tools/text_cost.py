"""What the text-encoder handle (vc_text_encode: the launch plan of csrc/text_engine.hip as ONE hipGraph launch per prompt) costs
beside the Python-ordered plan of visualcloze_amd/text.py (T5: the same launches captured from Python into one hipGraph; CLIP: issued
launch by launch from Python) at the product's widths: ms per prompt of T5-XXL (24 layers, 512 ids) and CLIP-L (12 layers, 77 ids)
with procedural weights, in ONE process on one box - HIP events around windows of whole calls on one stream, the two paths
interleaved round by round (boxes differ more than code does - README), one warm round first (it captures the plans), with the
board's power and clock during the timed rounds.  The outputs of the two paths are compared bit for bit.  No threshold and no claim:
both T5 paths are single graph launches of the same kernels; the handle is kept for the capability; this records the difference.
    python tools/text_cost.py [--rounds 7] [--calls 3] [--t5-layers 24] [--clip-layers 12] [--vocab 4096]
--vocab: rows of the procedural embedding tables (the lookups read one row per id, so the table's height does not enter the time)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests.procedural import key_seed, ptensor_torch, tiny_ids  # noqa: E402
from visualcloze_amd import hip  # noqa: E402
from visualcloze_amd.board import BoardSampler, pci_bus_id_of  # noqa: E402
from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel  # noqa: E402


def fill(model, dev):
    """tests/procedural.py::procedural_text_param's value classes, evaluated on the device (4.7 B parameters)"""
    import math
    model = model.to_empty(device=dev).to(torch.bfloat16)
    with torch.no_grad():
        for k, p in model.state_dict().items():
            seed = key_seed("txt:" + k)
            if "layer_norm" in k and k.endswith(".weight"):
                kw = dict(q=8, kmax=64, offset=1.0)
            elif k.endswith(".bias"):
                kw = dict(q=8, kmax=32)
            elif "relative_attention_bias" in k:
                kw = dict(q=5, kmax=64)
            elif "embedding" in k or k.startswith("shared") or "embed_tokens" in k:
                kw = dict(q=6, kmax=96)
            else:
                kw = dict(q=int(round(math.log2(73.0 * math.sqrt(p.shape[-1])))), kmax=127)
            p.copy_(ptensor_torch(tuple(p.shape), seed, device=dev, dtype=torch.bfloat16, **kw))
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="prompts per timed window")
    ap.add_argument("--t5-layers", type=int, default=24)
    ap.add_argument("--clip-layers", type=int, default=12)
    ap.add_argument("--vocab", type=int, default=4096)
    a = ap.parse_args()
    hip.require_gpu()
    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        t5 = T5EncoderModel(T5Config(vocab_size=a.vocab, num_layers=a.t5_layers))
        clip = CLIPTextModel(CLIPTextConfig(vocab_size=a.vocab, num_hidden_layers=a.clip_layers, eos_token_id=a.vocab - 1))
    t5, clip = fill(t5, dev), fill(clip, dev)
    t5_ids = tiny_ids(512, a.vocab, seed=5)[None].to(dev)
    clip_ids = tiny_ids(77, a.vocab, seed=6, eos=a.vocab - 1, eos_at=20)[None].to(dev)
    t5_hd, clip_hd = t5.handle(), clip.handle()
    st = torch.cuda.Stream(dev)

    legs = (("t5", "python", lambda: t5(t5_ids)), ("t5", "handle", lambda: t5_hd.encode(t5_ids)[0]),
            ("clip", "python", lambda: clip(clip_ids)[0]), ("clip", "handle", lambda: clip_hd.encode(clip_ids)[1]))
    ms = {(op, path): [] for op, path, _ in legs}
    out = {}
    board = BoardSampler(pci_bus_id_of(0), index=0, hz=10.0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(st):
        for r in range(a.rounds + 1):                 # round 0 warms every kernel, captures the plans and warms the clocks
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
    res = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, calls_per_window=a.calls, vocab=a.vocab,
               t5=dict(layers=a.t5_layers, ids=512, d_model=t5.cfg.d_model, workspace_bytes=t5_hd.workspace_bytes(512), captured_plans=t5_hd.plan_count()),
               clip=dict(layers=a.clip_layers, ids=77, d_model=clip.cfg.hidden_size, workspace_bytes=clip_hd.workspace_bytes(77),
                         captured_plans=clip_hd.plan_count()))
    for op in ("t5", "clip"):
        same = bool(torch.equal(out[(op, "python")], out[(op, "handle")]))
        assert same and torch.isfinite(out[(op, "handle")].float()).all(), op
        med = {p: statistics.median(ms[(op, p)]) for p in ("python", "handle")}
        res[op].update({p: dict(ms_median=round(med[p], 3), ms_min=round(min(ms[(op, p)]), 3), ms_max=round(max(ms[(op, p)]), 3))
                        for p in ("python", "handle")})
        res[op]["handle_over_python_pct"] = round(100 * (med["handle"] / med["python"] - 1), 2)
        res[op]["python_spread_pct"] = round(100 * (max(ms[(op, "python")]) / min(ms[(op, "python")]) - 1), 2)
        res[op]["bit_identical"] = same
    b = board.summary()
    res["board"] = {k: b.get(k) for k in ("power_w_avg", "power_cap_w", "sclk_mhz_avg", "source")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
