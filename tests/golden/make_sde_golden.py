"""Generate tests/golden/sde_golden.npz: the REFERENCE's own `Sampler.sample_sde` (transport/transport.py:300-359, the class `sde` of
transport/integrators.py, ICPlan of transport/path.py) on CPU in float64, under the torchdiffeq shim of make_golden.py.  Runs only
where the reference tree is (VC_REFERENCE); only the vectors travel.  float64 means torch's DEFAULT dtype is float64 while the
reference runs: its time grid, its `th.ones(...) * t1` of the last step and its draws are then doubles like the state (with the
f32 default its last step rounds w(t1) and sigma^2 / alpha to f32, a 1e-8 artefact of its own).

The reference adapted only sample_ode to Flux's reversed time; its sample_sde feeds the model t and takes the output unsigned.  It is
therefore driven with the adapter  A(x, t) = -F(x, 1 - t)  around the toy model F(x, tau) below (tau = the model time, as
Flux.forward takes it): the reference then runs its own mathematics on the velocity v(x, t) = -F(x, 1 - t), which is what
`visualcloze_amd.transport.sde_integrate` restates for F.

`th.randn` of the reference's integrators module is wrapped to record every draw, so a test can replay them.

Settings: B = 2, N = 5, C = 8; diffusion_norm 0.7; last_step_size 0.25; forms sigma / linear / decreasing / inccreasing-decreasing
x Euler / Heun x Mean / Euler / Tweedie with num_steps = 13 - the grid linspace(0, 0.75, 13) is exactly dyadic (k / 16), so the
reference's single dt = t[1] - t[0] equals every per-step difference - plus last_step None for Euler with num_steps = 17: the
reference then ends its grid at 1, and 17 points keep linspace(0, 1, 17) dyadic too (13 would not: k / 12).
"SBDM" (infinite at t0 = 0), "constant" (a TypeError in the reference) and Heun without a last step (a division by zero at t = 1)
do not run in the reference with this transport and are not recorded.

Recorded per case <c> = <form>_<method>_<last>:  <c>_draws  f64 [steps, B, N, C];  <c>_states  f64 [num_steps, B, N, C] (the
reference's list);  and once:  x0  f64 [B, N, C].

    python tests/golden/make_sde_golden.py     # rewrites tests/golden/sde_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SHAPE = (2, 5, 8)
NORM, LAST_STEP_SIZE = 0.7, 0.25
FORMS = ("sigma", "linear", "decreasing", "inccreasing-decreasing")
METHODS = ("Euler", "Heun")
LAST_STEPS = ("Mean", "Euler", "Tweedie")


def cases():
    """(name, form, method, last_step, num_steps)"""
    out = [(f"{f}_{m}_{l}", f, m, l, 13) for f in FORMS for m in METHODS for l in LAST_STEPS]
    return out + [(f"{f}_Euler_None", f, "Euler", None, 17) for f in FORMS]


def toy_model(x, tau):
    """F(x, tau): a smooth, nonlinear model output for the state x at the model time tau (a float or a [B] tensor)"""
    tau = torch.as_tensor(tau, dtype=x.dtype)
    if tau.dim() == 1:
        tau = tau.view(-1, *([1] * (x.dim() - 1)))
    return torch.sin(x) * (0.5 + tau) + 0.3 * x * tau - 0.2 * torch.cos(2.0 * x + tau)


def start_state():
    g = torch.Generator().manual_seed(1234)
    return torch.randn(SHAPE, generator=g, dtype=torch.float64)


class _RecordingTorch:
    """the torch module as the reference's integrators see it, with `randn` recorded"""

    def __init__(self, th, log):
        self._th, self._log = th, log

    def __getattr__(self, name):
        return getattr(self._th, name)

    def randn(self, *a, **k):
        z = self._th.randn(*a, **k)
        self._log.append(z.clone())
        return z


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    import transport.integrators as integrators  # noqa: E402
    from transport import Sampler, create_transport  # noqa: E402

    torch.set_default_dtype(torch.float64)
    draws = []
    integrators.th = _RecordingTorch(torch, draws)

    def adapter(x, t=None, timesteps=None, **kw):          # the reference calls model(x, timesteps=t) and model(x, t)
        t = timesteps if t is None else t
        return -toy_model(x, 1.0 - t)

    sampler = Sampler(create_transport("Linear", "velocity", do_shift=True))
    x0 = start_state()
    out = {"x0": x0.numpy()}
    for i, (name, form, method, last, num_steps) in enumerate(cases()):
        torch.manual_seed(100 + i)
        draws.clear()
        fn = sampler.sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=NORM, last_step=last,
                                last_step_size=LAST_STEP_SIZE, num_steps=num_steps)
        xs = fn(x0.clone(), adapter)
        assert len(xs) == num_steps and len(draws) == num_steps - 1 and all(d.dtype == torch.float64 for d in draws)
        states = torch.stack(xs)
        assert states.dtype == torch.float64 and bool(torch.isfinite(states).all()), name
        out[f"{name}_draws"] = torch.stack(draws).numpy()
        out[f"{name}_states"] = states.numpy()
    path = os.path.join(HERE, "sde_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
