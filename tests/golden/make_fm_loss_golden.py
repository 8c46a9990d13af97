"""Generate tests/golden/fm_loss_golden.npz: the REFERENCE's own `create_transport(...).training_losses` (transport/transport.py:132-176
on Transport.sample, :98-130, and ICPlan.plan of transport/path.py) on the CPU with torch's DEFAULT dtype float64, under the
torchdiffeq shim of make_golden.py.  Runs only where the reference tree is (VC_REFERENCE); only the vectors travel.

The model is the toy callable F(x || cond, tau) below (tau = the model time 1 - t, as Flux.forward takes it).  `th.rand`, `th.normal`
and `th.randn_like` of the reference's transport module are wrapped to record t's base draw and x0, so a test can replay them.

Cases: snr_type in {uniform, uniform_0.2_0.8, lognorm} x do_shift in {on, off} x {with img_mask, without} x {with cond, without}
at B = 3, N = 5, C = 8 (cond: 4 channels); the mask is ragged, valid rows 5 / 3 / 1 of 5 (a prefix, as the reference's right-padded
masks); plus one case at B = 1.  Recorded per case <c>:  <c>_base f64 [B] (the uniform or normal draw);  <c>_t f64 [B];  <c>_x0 f64
[B, N, C];  <c>_loss f64 [B] (the reference's "task_loss");  and once:  x1 / cond f64 [3, 5, 8] / [3, 5, 4];  mask f64 [3, 5].

    python tests/golden/make_fm_loss_golden.py     # rewrites tests/golden/fm_loss_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
B, N, C, CC = 3, 5, 8, 4
VALID = (5, 3, 1)
SNR_TYPES = ("uniform", "uniform_0.2_0.8", "lognorm")


def cases():
    """(name, snr_type, do_shift, masked, with_cond, batch)"""
    out = [(f"{s}_{'shift' if sh else 'noshift'}_{'mask' if m else 'nomask'}_{'cond' if c else 'nocond'}", s, sh, m, c, B)
           for s in SNR_TYPES for sh in (True, False) for m in (True, False) for c in (True, False)]
    return out + [("uniform_shift_mask_cond_b1", "uniform", True, True, True, 1)]


def toy_model(xin, timesteps, **kw):
    """F(x || cond, tau): a smooth, nonlinear model output of x's shape for the model input xin = x || cond at the model times tau [B]"""
    x, cond = xin[..., :C], xin[..., C:]
    tau = torch.as_tensor(timesteps, dtype=xin.dtype).view(-1, 1, 1)
    out = torch.sin(x) * (0.5 + tau) + 0.3 * x * tau - 0.2 * torch.cos(2.0 * x + tau)
    if cond.shape[-1]:
        out = out + 0.1 * torch.cat((cond, cond), dim=-1) * (1.0 - tau)
    return out


def data():
    g = torch.Generator().manual_seed(4321)
    x1 = torch.randn(B, N, C, generator=g, dtype=torch.float64)
    cond = torch.randn(B, N, CC, generator=g, dtype=torch.float64)
    mask = torch.zeros(B, N, dtype=torch.float64)
    for b, v in enumerate(VALID):
        mask[b, :v] = 1.0
    return x1, cond, mask


class _RecordingTorch:
    """the torch module as the reference's transport module sees it, with its three draws recorded"""

    def __init__(self, th, log):
        self._th, self._log = th, log

    def __getattr__(self, name):
        return getattr(self._th, name)

    def _rec(self, name, *a, **k):
        z = getattr(self._th, name)(*a, **k)
        self._log.append((name, z.clone()))
        return z

    def rand(self, *a, **k):
        return self._rec("rand", *a, **k)

    def normal(self, *a, **k):
        return self._rec("normal", *a, **k)

    def randn_like(self, *a, **k):
        return self._rec("randn_like", *a, **k)


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    import transport.transport as ref_transport  # noqa: E402
    from transport import create_transport  # noqa: E402

    torch.set_default_dtype(torch.float64)
    draws = []
    ref_transport.th = _RecordingTorch(torch, draws)
    x1, cond, mask = data()
    out = {"x1": x1.numpy(), "cond": cond.numpy(), "mask": mask.numpy()}
    for i, (name, snr, shift, masked, with_cond, bs) in enumerate(cases()):
        torch.manual_seed(500 + i)
        draws.clear()
        tr = create_transport("Linear", "velocity", snr_type=snr, do_shift=shift)
        kw = {"img_mask": mask[:bs]} if masked else {}

        def model(xin, timesteps, img_mask=None):
            return toy_model(xin, timesteps)

        terms = tr.training_losses(model, x1[:bs].clone(), kw, {"cond": cond[:bs] if with_cond else None})
        kinds = [k for k, _ in draws]
        assert kinds == ["randn_like", "normal" if snr == "lognorm" else "rand"], kinds
        assert all(z.dtype == torch.float64 for _, z in draws) and terms["task_loss"].dtype == torch.float64
        assert terms["task_loss"].shape == (bs,) and bool(torch.isfinite(terms["task_loss"]).all()), name
        out[f"{name}_x0"] = draws[0][1].numpy()
        out[f"{name}_base"] = draws[1][1].numpy()
        out[f"{name}_t"] = terms["t"].numpy()
        out[f"{name}_loss"] = terms["task_loss"].numpy()
    path = os.path.join(HERE, "fm_loss_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
