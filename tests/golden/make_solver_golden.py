"""Generate tests/golden/solver_golden.npz: the REFERENCE's own `Sampler.sample_ode(sampling_method="midpoint" | "rk4")`
on CPU, under the three shims of make_golden.py (flash_attn, torchdiffeq.odeint, torch.cuda.device) and with the procedural
tiny model of tests/procedural.py.  Runs only where the reference tree is (VC_REFERENCE); only the vectors travel.

The `odeint` shim is extended with the two fixed-grid step functions.  They are torchdiffeq 0.2.x's as recalled - the package
was not available to check against, so like the Euler rule of make_golden.py they are UNPINNED against real torchdiffeq:

    midpoint:  half_dt = 0.5 * dt;  f0 = f(t0, y0);  y_mid = y0 + f0 * half_dt;  y1 = y0 + dt * f(t0 + half_dt, y_mid)
    rk4:       k1 = f(t0, y0);  k2 = f(t0 + dt * (1/3), y0 + dt * k1 * (1/3));  k3 = f(t0 + dt * (2/3), y0 + dt * (k2 - k1 * (1/3)))
               k4 = f(t1, y0 + dt * (k1 - k2 + k3));  y1 = y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125

with every f call receiving t.to(y.dtype) (torchdiffeq's _PerturbFunc).  Recorded per method m:
    grid_cfg2_<m>_model_t_<f32|bf16>, grid_sdedit_<m>_model_t_<f32|bf16>   the times the model is called with (3456 tokens x 30
                                                  points, shifted; 4096 tokens x 10 points, strength 0.4, no shift)
    traj_<m>_states                               5-point trajectory of the tiny model in fp32
    traj_<m>_bf16_states / _bf16_model_t          ... under bf16 autocast with a bf16 state
    traj_<m>_f32state_states / _f32state_model_t  ... under bf16 autocast with an f32 state
    closed_<m>_<f32|bf16>_states / _model_t       trajectory of `closed_form_model` (multiplies and adds only: bit-reproducible)
    floor_<m>                                     rel-L2 between the reference's own bf16 and fp32 final states

    python tests/golden/make_solver_golden.py     # rewrites tests/golden/solver_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
METHODS = ("midpoint", "rk4")
CLOSED_SHAPE, CLOSED_POINTS = (2, 24, 8), 5


def closed_form_model(xin, timesteps, **kw):
    """A cheap velocity field of x || cond and t built from multiplies and adds alone, so that every machine computes the same
    bits: v = x * t - 0.25 * x^2 + 0.5 * (cond, cond) + t."""
    x, c = xin[..., :CLOSED_SHAPE[2]], xin[..., CLOSED_SHAPE[2]:]
    t = timesteps.to(xin.dtype)[:, None, None]
    return x * t - x * x * 0.25 + c.repeat(1, 1, 2) * 0.5 + t


def closed_form_inputs(dtype):
    from tests.procedural import ptensor
    B, N, C = CLOSED_SHAPE
    return ptensor((B, N, C), 91, q=6).to(dtype), ptensor((B, N, C // 2), 92, q=6).to(dtype)


def odeint(func, y0, t, method="euler", **kw):
    """fixed-grid solvers on the given time points; `calls` sees every time the drift is evaluated at"""
    def f(ti, y):
        odeint.calls.append(float(ti))
        return func(ti.to(y0.dtype), y)          # _PerturbFunc.forward

    def euler(t0, t1, dt, y0):
        return y0 + dt * f(t0, y0)

    def midpoint(t0, t1, dt, y0):
        half_dt = 0.5 * dt
        f0 = f(t0, y0)
        y_mid = y0 + f0 * half_dt
        return y0 + dt * f(t0 + half_dt, y_mid)

    def rk4(t0, t1, dt, y0):
        k1 = f(t0, y0)
        k2 = f(t0 + dt * (1 / 3), y0 + dt * k1 * (1 / 3))
        k3 = f(t0 + dt * (2 / 3), y0 + dt * (k2 - k1 * (1 / 3)))
        k4 = f(t1, y0 + dt * (k1 - k2 + k3))
        return y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125

    step = {"euler": euler, "midpoint": midpoint, "rk4": rk4}[method]
    ys = [y0]
    for i in range(len(t) - 1):
        ys.append(step(t[i], t[i + 1], t[i + 1] - t[i], ys[-1]))
    return torch.stack(ys)


odeint.calls = []


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    make_golden.install_shims()
    sys.modules["torchdiffeq"].odeint = odeint
    sys.path.insert(0, make_golden.REF)
    from models.model import FluxLoraWrapper, FluxParams  # noqa: E402
    from transport import Sampler, create_transport  # noqa: E402

    from tests.procedural import TINY, TINY_RANK, procedural_param, tiny_inputs

    torch.manual_seed(0)
    out = {}
    model = FluxLoraWrapper(lora_rank=TINY_RANK, lora_scale=1.0, params=FluxParams(**TINY)).float().eval()
    key_shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: procedural_param(k, s) for k, s in key_shapes}, strict=True)
    mb = FluxLoraWrapper(lora_rank=TINY_RANK, lora_scale=1.0, params=FluxParams(**TINY)).eval()
    mb.load_state_dict({k: procedural_param(k, s) for k, s in key_shapes})
    mb = mb.to(torch.bfloat16)
    inp = tiny_inputs(B=1)
    sampler = Sampler(create_transport("Linear", "velocity", do_shift=True))
    common = dict(atol=1e-6, rtol=1e-3, reverse=False)

    def record_times(fn, x):
        seen = []
        fn(x, lambda xin, timesteps, **kw: (seen.append(float(timesteps[0])), xin * 0)[1], {})
        return np.array(seen, dtype=np.float64)

    with torch.no_grad():
        for m in METHODS:
            cfg2 = sampler.sample_ode(sampling_method=m, num_steps=30, do_shift=True, time_shifting_factor=1, **common)
            sded = sampler.sample_ode(sampling_method=m, num_steps=10, do_shift=False, time_shifting_factor=1.0, strength=0.4, **common)
            for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                out[f"grid_cfg2_{m}_model_t_{name}"] = record_times(cfg2, torch.zeros(1, 3456, 2, dtype=dt))
                out[f"grid_sdedit_{m}_model_t_{name}"] = record_times(sded, torch.zeros(1, 4096, 2, dtype=dt))

            fn = sampler.sample_ode(sampling_method=m, num_steps=5, do_shift=True, time_shifting_factor=1, **common)
            kw = dict(txt=inp["txt"], txt_ids=inp["txt_ids"], txt_mask=inp["txt_mask"], y=inp["y"], img_ids=inp["img_ids"],
                      img_mask=inp["img_mask"], cond=inp["cond"], guidance=inp["guidance"])
            out[f"traj_{m}_states"] = fn(inp["x"], model.forward, kw).numpy()
            kwb = dict(txt=inp["txt"].bfloat16(), txt_ids=inp["txt_ids"], txt_mask=inp["txt_mask"], y=inp["y"].bfloat16(),
                       img_ids=inp["img_ids"], img_mask=inp["img_mask"], cond=inp["cond"].bfloat16(),
                       guidance=inp["guidance"].bfloat16())
            seen = []

            def mb_fwd(x, timesteps, **k):
                seen.append(float(timesteps[0]))
                assert timesteps.dtype == torch.float32
                return mb.forward(x, timesteps=timesteps, **k)
            with torch.autocast("cpu", torch.bfloat16):
                trajb = fn(inp["x"].bfloat16(), mb_fwd, kwb)
            assert trajb.dtype == torch.bfloat16
            out[f"traj_{m}_bf16_model_t"] = np.array(seen, dtype=np.float64)
            out[f"traj_{m}_bf16_states"] = trajb.float().numpy()
            seen.clear()
            with torch.autocast("cpu", torch.bfloat16):
                trajf = fn(inp["x"].float(), mb_fwd, kwb)
            assert trajf.dtype == torch.float32
            out[f"traj_{m}_f32state_model_t"] = np.array(seen, dtype=np.float64)
            out[f"traj_{m}_f32state_states"] = trajf.numpy()
            a, b = out[f"traj_{m}_states"][-1], out[f"traj_{m}_bf16_states"][-1]
            out[f"floor_{m}"] = np.array(np.linalg.norm(a - b) / np.linalg.norm(a), dtype=np.float64)

            fn = sampler.sample_ode(sampling_method=m, num_steps=CLOSED_POINTS, do_shift=True, time_shifting_factor=1, **common)
            for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                x, cond = closed_form_inputs(dt)
                seen = []
                traj = fn(x, lambda xin, timesteps, **k: (seen.append(float(timesteps[0])), closed_form_model(xin, timesteps, **k))[1],
                          dict(cond=cond))
                assert traj.dtype == dt
                out[f"closed_{m}_{name}_model_t"] = np.array(seen, dtype=np.float64)
                out[f"closed_{m}_{name}_states"] = traj.float().numpy()

    path = os.path.join(HERE, "solver_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for m in METHODS:
        print(f"floor_{m} (reference bf16 vs fp32, final state, rel-L2) = {float(out[f'floor_{m}']):.3e}")


if __name__ == "__main__":
    main()
