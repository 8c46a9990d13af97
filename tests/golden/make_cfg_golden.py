"""Generate tests/golden/cfg_golden.npz: the REFERENCE's own `Flux.forward_with_cfg` (models/model.py:126-145) and its
`Sampler.sample_ode("euler")` over it, on CPU, under the shims of make_golden.py (flash_attn, torchdiffeq.odeint, torch.cuda.device)
and with the procedural tiny model of tests/procedural.py.  Runs only where the reference tree is (VC_REFERENCE); only the vectors
travel.  The Euler rule of the odeint shim is unpinned against real torchdiffeq, as in make_golden.py.

The inputs are `cfg_inputs(B)`, which the tests import from this file: `tiny_inputs(B, seed=7)` arranged as a true-CFG batch - the
first half the conditional samples, the second half their unconditional twins (the same x and cond, another text of another
length, another y, another guidance).  B = 4 has a shorter, right-padded grid in its second pair (both samples of the pair: the
fused loop needs equal image masks within a pair).  Recorded for B in (2, 4) at cfg_scale = 3.5:
    fwd_b<B>_t                          the timesteps of the forward_with_cfg call
    fwd_b<B> / fwd_b<B>_bf16            forward_with_cfg in fp32 / with bf16 parameters under bf16 autocast (as make_fullwidth_reference.py)
    traj_b<B>_states                    4-point (3-step) Euler trajectory over forward_with_cfg in fp32
    traj_b<B>_bf16_states / _model_t    ... under bf16 autocast with a bf16 state, and the times the model saw
    traj_b2_f32state_states             ... under bf16 autocast with an f32 state
    floor_b<B>                          rel-L2 between the reference's own bf16 and fp32 final states

    python tests/golden/make_cfg_golden.py     # rewrites tests/golden/cfg_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
CFG_SCALE = 3.5
BATCHES = (2, 4)
POINTS = 4                     # 3 solver steps


def cfg_inputs(B: int) -> dict:
    """A true-CFG batch of the tiny geometry: samples [0, B/2) conditional, [B/2, B) unconditional."""
    from tests.procedural import tiny_inputs
    assert B % 2 == 0
    h = B // 2
    inp = tiny_inputs(B=B, seed=7)
    inp["x"][h:] = inp["x"][:h]                 # the halves start from one state and share the conditioning columns
    inp["cond"][h:] = inp["cond"][:h]
    inp["txt_mask"][h:, -5:] = 0                # the negative prompt is shorter
    inp["guidance"][h:] = 4.0
    if B >= 4:
        inp["img_mask"][1, -12:] = 0            # the second pair is a shorter grid, padded (sampling.py:68-70)
        inp["img_mask"][h + 1, -12:] = 0
    return inp


def cfg_timesteps(B: int) -> torch.Tensor:
    return torch.tensor([0.9, 0.25][: B // 2] * 2) if B >= 4 else torch.tensor([0.7, 0.7])


def main():
    sys.path.insert(0, HERE)
    import make_golden
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    from models.model import FluxLoraWrapper, FluxParams  # noqa: E402
    from transport import Sampler, create_transport  # noqa: E402

    from tests.procedural import TINY, TINY_RANK, procedural_param

    torch.manual_seed(0)
    out = {"cfg_scale": np.array(CFG_SCALE, dtype=np.float64)}
    model = FluxLoraWrapper(lora_rank=TINY_RANK, lora_scale=1.0, params=FluxParams(**TINY)).float().eval()
    key_shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: procedural_param(k, s) for k, s in key_shapes}, strict=True)
    mb = FluxLoraWrapper(lora_rank=TINY_RANK, lora_scale=1.0, params=FluxParams(**TINY)).eval()
    mb.load_state_dict({k: procedural_param(k, s) for k, s in key_shapes})
    mb = mb.to(torch.bfloat16)
    sampler = Sampler(create_transport("Linear", "velocity", do_shift=True))
    fn = sampler.sample_ode(sampling_method="euler", num_steps=POINTS, atol=1e-6, rtol=1e-3, reverse=False, do_shift=True,
                            time_shifting_factor=1)

    with torch.no_grad():
        for B in BATCHES:
            inp = cfg_inputs(B)
            t = cfg_timesteps(B)
            kw = dict(txt=inp["txt"], txt_ids=inp["txt_ids"], txt_mask=inp["txt_mask"], y=inp["y"], img_ids=inp["img_ids"],
                      img_mask=inp["img_mask"], guidance=inp["guidance"])
            kwb = dict(kw, txt=inp["txt"].bfloat16(), y=inp["y"].bfloat16(), guidance=inp["guidance"].bfloat16())
            img = torch.cat((inp["x"], inp["cond"]), -1)
            out[f"fwd_b{B}_t"] = t.numpy()
            out[f"fwd_b{B}"] = model.forward_with_cfg(img, timesteps=t, cfg_scale=CFG_SCALE, **kw).numpy()
            with torch.autocast("cpu", torch.bfloat16):
                yb = mb.forward_with_cfg(img.bfloat16(), timesteps=t, cfg_scale=CFG_SCALE, **kwb)
            assert yb.dtype == torch.bfloat16
            out[f"fwd_b{B}_bf16"] = yb.float().numpy()

            out[f"traj_b{B}_states"] = fn(inp["x"], model.forward_with_cfg, dict(kw, cond=inp["cond"], cfg_scale=CFG_SCALE)).numpy()
            seen = []

            def mb_fwd(x, timesteps, **k):
                seen.append(float(timesteps[0]))
                assert timesteps.dtype == torch.float32
                return mb.forward_with_cfg(x, timesteps=timesteps, **k)
            kwt = dict(kwb, cond=inp["cond"].bfloat16(), cfg_scale=CFG_SCALE)
            with torch.autocast("cpu", torch.bfloat16):
                trajb = fn(inp["x"].bfloat16(), mb_fwd, kwt)
            assert trajb.dtype == torch.bfloat16
            out[f"traj_b{B}_bf16_model_t"] = np.array(seen, dtype=np.float64)
            out[f"traj_b{B}_bf16_states"] = trajb.float().numpy()
            if B == 2:
                with torch.autocast("cpu", torch.bfloat16):
                    trajf = fn(inp["x"].float(), mb_fwd, kwt)
                assert trajf.dtype == torch.float32
                out["traj_b2_f32state_states"] = trajf.numpy()
            a, b = out[f"traj_b{B}_states"][-1], out[f"traj_b{B}_bf16_states"][-1]
            out[f"floor_b{B}"] = np.array(np.linalg.norm(a - b) / np.linalg.norm(a), dtype=np.float64)

    path = os.path.join(HERE, "cfg_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for B in BATCHES:
        print(f"floor_b{B} (reference bf16 vs fp32, final state, rel-L2) = {float(out[f'floor_b{B}']):.3e}")


if __name__ == "__main__":
    main()
