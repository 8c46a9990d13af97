"""Host-side mirror of the reference's sampler interface (transport/__init__.py:4-62,
transport/transport.py:236-410, transport/integrators.py:79-120, transport/utils.py:33-44):

    sampler = Sampler(create_transport("Linear", "velocity", do_shift=True))
    sample_fn = sampler.sample_ode(sampling_method="euler", num_steps=30, ...)
    latents = sample_fn(x, model.forward, model_kwargs)[-1]

Only the configuration the inference pipeline uses is implemented (Linear path, velocity prediction) with the
fixed-grid solvers "euler", "midpoint" and "rk4"; anything else raises NotImplementedError.  When `model` is the
bound `forward` of a `visualcloze_amd.Flux`, the whole loop runs as hipGraph replays of one captured evaluation +
the solver's update (Euler step / midpoint or rk4 stage combination) with zero host synchronisation inside the
loop; a foreign callable is stepped eagerly with the same grid.  The bound `forward_with_cfg` of a `visualcloze_amd.Flux`
(true classifier-free guidance, model.py:126-145: `model_kwargs["cfg_scale"]`, conditional samples first, unconditional ones
behind them) runs the same fused loop with the cross-sample combine as one more node of the captured step.

`Sampler.sample_ode_adaptive` is the error-controlled solve the reference's `sample_ode` defaults to ("dopri5"), under a name of its
own - `sample_ode(sampling_method="dopri5")` keeps raising: adaptive Dormand-Prince 5(4), fused through vc_flux_sample_dopri5 for a
`visualcloze_amd.Flux` with the C handle, `dopri5_integrate` (the same rule in plain torch) for any other callable.
`method="bosh3"` / `"adaptive_heun"` run the cheaper embedded pairs (3 / 2 evaluations per attempt against 6) through the same loop:
vc_flux_sample_rk fused, `rk_integrate` in plain torch.

`Sampler.sample_sde` is the reference's stochastic sampler (transport.py:300-359: Euler-Maruyama / stochastic Heun, the six diffusion
forms, the four last steps) on the velocity v(x, t) = -model(x || cond, timesteps = 1 - t) - the adaptation the reference made for
sample_ode only.  `sde_plan` turns a setting into one coefficient row per evaluation (bit for bit vc_sde_plan's table), `sde_integrate`
is the literal torch restatement of the loop, and the fused path is vc_flux_sample_sde: the captured evaluation with vc_sde_stage
behind it, the noise drawn inside that kernel from the library's counter-based stream.

`Transport.sample` / `Transport.training_losses` are the reference's training objective (transport.py:98-176: the masked flow-matching
loss of ONE model evaluation at a drawn time and noise) as an EVALUATION: forward only, under torch.no_grad(), nothing here can be
back-propagated.  `fm_times` is the rule that maps base draws to training times (bit for bit vc_fm_times for f32 draws), `fm_loss_terms`
the loss in literal torch for any callable, and the fused path is vc_flux_eval_loss: vc_fm_plan in front of the handle's single
evaluation and vc_fm_loss behind it, one call per chunk of samples.

The step rules (`STEP_RULES`) are torchdiffeq 0.2.x's fixed-grid solvers as recalled - unpinned against real
torchdiffeq, which was not available to check against (as the Euler rule, tests/golden/make_golden.py).  They
are written ONCE, as the literal torch expressions: a correction is a one-line change here and in
csrc/elementwise.hip (ode_update).
"""
from __future__ import annotations

import math
import re
from contextlib import contextmanager
from functools import partial
from typing import Callable, Optional

import torch

from . import hip
from .reduction import ordered_sum


def time_shift(mu: float, sigma: float, t: torch.Tensor) -> torch.Tensor:
    """transport/utils.py:33-39 (endpoints 0 -> 0 and 1 -> 1 through inf arithmetic, as the reference)."""
    t = 1 - t
    t = math.exp(mu) / (math.exp(mu) + (1 / t - 1) ** sigma)
    return 1 - t


def get_lin_function(x1: float = 256, y1: float = 0.5, x2: float = 4096, y2: float = 1.15) -> Callable:
    m = (y2 - y1) / (x2 - x1)
    b = y1 - m * x1
    return lambda x: m * x + b


def solver_time_grid(num_steps: int, n_tokens: int, t0: float, t1: float, do_shift: bool,
                     time_shifting_factor: Optional[float]) -> torch.Tensor:
    """ode.__init__ + ode.sample (integrators.py:99-101,113-116): the solver's time POINTS (f32, CPU)."""
    assert t0 < t1, "ODE sampler has to be in forward time"
    t = torch.linspace(t0, t1, num_steps)
    if time_shifting_factor:
        t = t / (t + time_shifting_factor - time_shifting_factor * t)
    if do_shift:
        mu = get_lin_function(y1=0.5, y2=1.15)(n_tokens)
        t = time_shift(mu, 1.0, t)
    return t


_SNR_UNIFORM = re.compile(r"^uniform_([0-9eE+\-.]+)_([0-9eE+\-.]+)$")


def parse_snr_type(snr_type: str):
    """-> ("uniform" | "lognorm", t0, t1) of Transport.sample's `snr_type` (transport.py:112-121): "uniform", "uniform_<t0>_<t1>" (two
    finite plain decimal numbers) or "lognorm"; (t0, t1) = (0, 1) - check_interval for Linear + velocity - unless the string gives
    them.  Anything else raises: NotImplementedError for an unknown type, as the reference, ValueError for a malformed interval
    (where the reference's unpacking or float() fails).  vc_fm_times refuses the same strings."""
    if not isinstance(snr_type, str):
        raise NotImplementedError("Not implemented snr_type %s" % (snr_type,))
    if snr_type == "lognorm":
        return "lognorm", 0.0, 1.0
    if snr_type == "uniform":
        return "uniform", 0.0, 1.0
    if snr_type.startswith("uniform_"):
        m = _SNR_UNIFORM.match(snr_type)
        try:
            t0, t1 = (float(m.group(1)), float(m.group(2))) if m else (math.nan, math.nan)
        except ValueError:
            t0 = t1 = math.nan
        if not (math.isfinite(t0) and math.isfinite(t1)):
            raise ValueError(f"snr_type {snr_type!r} is not 'uniform_<t0>_<t1>' with two finite numbers")
        return "uniform", t0, t1
    raise NotImplementedError("Not implemented snr_type %s" % snr_type)


def _exp_f32(x: torch.Tensor) -> torch.Tensor:
    """exp of an f32 tensor, each value taken in double (libm, as vc_fm_times) and rounded once to f32: the correctly rounded f32
    exponential, which torch's vectorised CPU exp is not (it is within an ulp of it)"""
    def one(v: float) -> float:
        try:
            return math.exp(v)
        except OverflowError:
            return math.inf
    return torch.tensor([one(float(v)) for v in x.reshape(-1).tolist()], dtype=torch.float64).to(torch.float32).reshape(x.shape)


def fm_times(base: torch.Tensor, snr_type: str, n_tokens: int, do_shift: bool) -> torch.Tensor:
    """Transport.sample's training times (transport.py:112-127) from its base draws - torch.rand for "uniform" / "uniform_<t0>_<t1>",
    torch.normal(0, 1) for "lognorm" - as the reference's own torch expressions, in the draws' dtype:
        uniform   t = base * (t1 - t0) + t0          lognorm   t = 1 / (1 + exp(-base)) * (t1 - t0) + t0
    then time_shift(mu(n_tokens), 1.0, t) with do_shift.  f64 draws give the reference's f64 bits; f32 draws give vc_fm_times' bits
    (hip.fm_times), which are the reference's f32 operations except that the exponential of "lognorm" is the correctly rounded one
    (`_exp_f32`).  Any other dtype is computed in f32."""
    kind, t0, t1 = parse_snr_type(snr_type)
    if base.dtype not in (torch.float32, torch.float64):
        base = base.to(torch.float32)
    if kind == "uniform":
        t = base * (t1 - t0) + t0
    else:
        e = torch.exp(-base) if base.dtype == torch.float64 else _exp_f32(-base.cpu()).to(base.device)
        t = 1 / (1 + e) * (t1 - t0) + t0
    if do_shift:
        t = time_shift(get_lin_function(y1=0.5, y2=1.15)(n_tokens), 1.0, t)
    return t


def fm_path(t: torch.Tensor, x0: torch.Tensor, x1: torch.Tensor):
    """ICPlan.plan of the reference for the Linear path (alpha = t, sigma = 1 - t): -> (x_t, u_t) = (t x1 + (1 - t) x0, x1 - x0) with t
    [B] broadcast over the samples.  f64 tensors: the reference's f64 expressions, bit for bit.  f32 / bf16 tensors: vc_fm_plan's
    arithmetic - every operand converted to f32, t * x1 and (1 - t) * x0 rounded on their own, x_t rounded ONCE to bf16 and handed
    back in x1's dtype, u_t in f32."""
    tb = t.view(t.size(0), *([1] * (x1.dim() - 1)))
    if x1.dtype == torch.float64:
        return tb * x1 + (1 - tb) * x0, 1 * x1 + -1 * x0
    tf, a, z = tb.to(torch.float32), x1.to(torch.float32), x0.to(torch.float32)
    return (tf * a + (1 - tf) * z).to(torch.bfloat16).to(x1.dtype), a - z


def _fm_ordered_sum(sq: torch.Tensor, rows_total: int) -> torch.Tensor:
    """sum of the f32 squares `sq` [valid rows, cols] of ONE sample in vc_fm_loss's order (include/vcloze_hip.h): units of 8 elements
    along a row, the grid sized by all `rows_total` rows, summed by `reduction.ordered_sum`"""
    sq = sq.detach().to("cpu", torch.float32)
    R, cols = sq.shape
    upr = (cols + 7) // 8
    units = torch.zeros(R, upr * 8, dtype=torch.float32)       # (x + 0 = x for the squares: zero padding does not show)
    units[:, :cols] = sq
    return ordered_sum(units.view(R * upr, 8), rows_total * upr, hip.FM_LOSS_MAX_BLOCKS)


def fm_loss_reduce(out: torch.Tensor, ut: torch.Tensor, img_mask: Optional[torch.Tensor] = None, ordered: bool = False) -> torch.Tensor:
    """The reduction of Transport.training_losses (transport.py:149-171) for a tensor x1: model_output = -out; with an image mask
    sum(((model_output - ut) * mask)^2) / (mask.sum * D) per sample, else the mean over all non-batch dimensions.  f64 `ut`: the
    reference's expressions in f64.  Otherwise f32, d = (-out) - ut, in torch's own summation order - or with `ordered` in the fixed
    order of vc_fm_loss over each sample's valid rows (taken in row order: the handle's valid-first order), divided by
    f32(valid rows * D): the kernel's bits.  -> [B]"""
    B = ut.shape[0]
    if ut.dtype == torch.float64:
        model_output = -out.to(torch.float64)
        if img_mask is not None:
            D = model_output.shape[-1]
            mask_loss = (model_output - ut) * img_mask.unsqueeze(-1)
            return (mask_loss ** 2).sum(dim=list(range(1, ut.dim()))) / (img_mask.sum(dim=1) * D)
        return torch.mean((model_output - ut) ** 2, dim=list(range(1, ut.dim())))
    d = (0 - out.to(torch.float32)) - ut.to(torch.float32)
    sq = d * d
    if not ordered:
        if img_mask is not None:
            m = img_mask.to(sq.device, torch.float32)
            return (sq * m.unsqueeze(-1)).sum(dim=list(range(1, ut.dim()))) / (m.sum(dim=1) * sq.shape[-1])
        return torch.mean(sq, dim=list(range(1, ut.dim())))
    sq = sq.reshape(B, -1, sq.shape[-1]).cpu()
    rows, cols = sq.shape[1:]
    res = []
    for b in range(B):
        keep = torch.ones(rows, dtype=torch.bool) if img_mask is None else img_mask[b].reshape(-1).cpu() != 0
        n = int(keep.sum())
        total = _fm_ordered_sum(sq[b][keep], rows)
        res.append(total / torch.tensor(float(n * cols), dtype=torch.float64).to(torch.float32))
    return torch.stack(res).to(ut.device)


@torch.no_grad()
def fm_loss_terms(model: Callable, x1: torch.Tensor, t: torch.Tensor, x0: torch.Tensor, model_kwargs: Optional[dict] = None,
                  cond: Optional[torch.Tensor] = None, ordered: bool = False) -> dict:
    """Transport.training_losses (transport.py:132-176) for given t [B] and x0, in literal torch, for any callable and any float dtype:
    -> {"loss", "task_loss" [B], "t"}.  EVALUATION only: it runs under torch.no_grad() and nothing here can be back-propagated.
    x_t, u_t = `fm_path`; out = model(x_t || cond, timesteps = 1 - t, **model_kwargs); the reduction = `fm_loss_reduce` with
    model_kwargs["img_mask"] where it is given.  f64 in: the reference's f64 computation.  f32 / bf16 in: the arithmetic of
    vc_fm_plan / vc_fm_loss (t in x1's dtype, x_t rounded once to bf16, u_t and the loss in f32); with `ordered` the sum follows the
    kernel's stated order, so a test can ask for its bits."""
    model_kwargs = {} if model_kwargs is None else model_kwargs
    t = t.to(x1[0])
    x0 = x0.to(x1)
    xt, ut = fm_path(t, x0, x1)
    xin = torch.cat((xt, cond.to(xt)), dim=-1) if cond is not None else xt
    out = model(xin, timesteps=1 - t, **model_kwargs)
    assert out.shape == ut.shape, f"the model returned {tuple(out.shape)} for a target of {tuple(ut.shape)}"
    loss = fm_loss_reduce(out.detach(), ut, model_kwargs.get("img_mask"), ordered).detach()
    return {"loss": loss, "task_loss": loss.clone(), "t": t}


class Transport:
    def __init__(self, path_type: str, prediction: str, do_shift: bool, snr_type: str = "uniform"):
        self.path_type, self.prediction, self.do_shift, self.snr_type = path_type, prediction, do_shift, snr_type
        self.train_eps = self.sample_eps = 0  # velocity & Linear is stable everywhere (transport/__init__.py:46-48)

    def sample(self, x1, snr_type=None):
        """transport.py:98-130: draw x0 and t for the data x1 [B, N, C] -> (t, x0, x1), with torch.randn_like, then torch.rand
        ("uniform...") or torch.normal ("lognorm") exactly as the reference draws them, so the same torch.manual_seed gives the
        reference's t and x0 on the CPU.  t = `fm_times` of the base draw with n_tokens = x1.shape[1], converted to x1's dtype and device."""
        if isinstance(x1, (list, tuple)):
            raise NotImplementedError("Transport.sample: a list of tensors (the reference's variable-size branch) is not implemented; pass "
                                      "one [B, N, C] tensor")
        kind, _, _ = parse_snr_type(self.snr_type if snr_type is None else snr_type)
        x0 = torch.randn_like(x1)
        if kind == "uniform":
            base = torch.rand((len(x1),))
        else:
            base = torch.normal(mean=0.0, std=1.0, size=(len(x1),))
        t = fm_times(base, self.snr_type if snr_type is None else snr_type, x1.shape[1], self.do_shift)
        return t.to(x1[0]), x0, x1

    @torch.no_grad()
    def training_losses(self, model, x1, model_kwargs=None, extra_kwargs=None, *, t=None, x0=None, rng=None):
        """transport.py:132-176 as an EVALUATION: the flow-matching loss of one model evaluation at a drawn (or given) time t [B] and
        noise x0 -> {"loss", "task_loss": [B], "t": [B]} - masked by model_kwargs["img_mask"] where given, the mean over all
        non-batch elements otherwise; extra_kwargs["cond"] is concatenated behind x_t.  It runs under torch.no_grad(): `loss` carries
        no graph and NOTHING HERE CAN BE BACK-PROPAGATED - it is the validation loss, not a training step.
        t / x0 None: drawn as `sample` draws them (torch.manual_seed reproduces).  rng: a `pipeline.NoiseStream` - x0 comes from the
        library's stream at rng.offset, which advances by x1.numel(); a `TorchNoiseStream` draws x0 = rng.randn(x1.shape) first.
        Fused (vc_flux_eval_loss, one call per chunk of samples through `ChunkPlan`) for the bound `forward` of a visualcloze_amd.Flux that
        has the C handle and a bf16 / f32 x1; a NoiseStream's x0 is then drawn inside the kernel, element i of a chunk - the flat index
        in its [bs, N, C] rows IN THE HANDLE'S ROW ORDER (image rows valid-first per sample) - at offset + i, chunk after chunk.  Eager
        (`fm_loss_terms`) for everything else.  A list of tensors raises NotImplementedError."""
        if isinstance(x1, (list, tuple)):
            raise NotImplementedError("training_losses: a list of tensors (the reference's variable-size branch) is not implemented; pass "
                                      "one [B, N, C] tensor")
        model_kwargs = {} if model_kwargs is None else model_kwargs
        cond = (extra_kwargs or {}).get("cond")
        if rng is not None and x0 is not None:
            raise ValueError("training_losses: pass x0 or rng, not both")
        owner, kind, kw, _ = _classify(model, model_kwargs)
        fused = kind == "forward" and owner.handle() is not None and x1.dtype in (torch.bfloat16, torch.float32) and x1.dim() == 3
        if t is None and x0 is None and rng is None:
            t, x0, _ = self.sample(x1)
        elif t is None:
            kind_, _, _ = parse_snr_type(self.snr_type)
            base = torch.rand((len(x1),)) if kind_ == "uniform" else torch.normal(mean=0.0, std=1.0, size=(len(x1),))
            t = fm_times(base, self.snr_type, x1.shape[1], self.do_shift)
        t = torch.as_tensor(t).reshape(-1).to(x1[0])
        if t.numel() != len(x1):
            raise ValueError(f"training_losses: {t.numel()} times for a batch of {len(x1)}")
        in_kernel = None
        if rng is not None:
            if hasattr(rng, "threads_per_sm") or not fused:      # a TorchNoiseStream, or the eager path: the tensor first
                x0 = rng.randn(tuple(x1.shape), dtype=x1.dtype, device=x1.device if x1.is_cuda else None)
            else:
                if rng.offset + x1.numel() > 1 << 64:
                    raise ValueError(f"training_losses: {x1.numel()} elements at offset {rng.offset} leave the 64-bit stream")
                in_kernel = (int(rng.seed), int(rng.offset))
        elif x0 is None:
            x0 = torch.randn_like(x1)
        if fused:
            loss = _losses_fused(owner, x1, kw, cond, t, x0, in_kernel)
            if in_kernel is not None:
                rng.offset = in_kernel[1] + x1.numel()
            return {"loss": loss, "task_loss": loss.clone(), "t": t}
        return fm_loss_terms(model, x1, t, x0, model_kwargs, cond)

    def check_interval(self, reverse: bool = False, *, sde: bool = False, diffusion_form: str = "SBDM", last_step_size: float = 0.0,
                       sample_eps=None):
        t0, t1 = 0, 1  # transport.py:70-96 for Linear + velocity
        if sde:        # ... eval=True: t0 = eps for SBDM, t1 = 1 - last_step_size with a last step, else 1 - eps
            eps = self.sample_eps if sample_eps is None else sample_eps
            t0 = eps if diffusion_form == "SBDM" else 0
            t1 = 1 - eps if last_step_size == 0 else 1 - last_step_size
        if reverse:
            t0, t1 = 1 - t0, 1 - t1
        return t0, t1


def create_transport(path_type="Linear", prediction="velocity", loss_weight=None, train_eps=None, sample_eps=None,
                     snr_type="uniform", loss_type="mse", do_shift=True) -> Transport:
    if path_type != "Linear" or prediction != "velocity":
        raise NotImplementedError("the MI355X denoising path implements Linear path + velocity prediction only")
    return Transport(path_type, prediction, do_shift, snr_type)


@torch.no_grad()
def _losses_fused(flux, x1, kw, cond, t, x0, in_kernel):
    """vc_flux_eval_loss per chunk of samples -> loss f32 [B] on the model's device.  in_kernel: (seed, offset) of the in-kernel draw
    (x0 None), a chunk's draw behind the last chunk's in the stream"""
    h = flux.handle()
    B, N, C = x1.shape
    kw = dict(kw)
    if kw.get("img_mask") is not None and kw.get("txt_mask") is None:      # the loss's mask alone: every text row is valid
        kw["txt_mask"] = torch.ones(kw["txt"].shape[:2], dtype=torch.bool)
    plan = flux.chunk_plan(B, N, kw, channels=(C, 0 if cond is None else cond.shape[-1]))
    loss = torch.empty(B, dtype=torch.float32, device=plan.dev)
    pos = None if in_kernel is None else in_kernel[1]
    tf = t.detach().to("cpu", torch.float32)
    with flux.monitored(h) as monitored:
        try:
            h.set_cfg(None)
            h.set_eval_loss(True)
            for sl in plan.chunks:
                h.prepare(*plan.prepare_args(sl, 1))
                xs = plan.img_rows(x1, sl, x1.dtype)
                with monitored(1):
                    out = h.eval_loss(xs, None if cond is None else plan.img_rows(cond, sl, torch.bfloat16), tf[sl],
                                      x0=None if x0 is None else plan.img_rows(x0, sl, x1.dtype),
                                      seed=0 if in_kernel is None else in_kernel[0], offset=pos or 0)
                if pos is not None:
                    pos += xs.numel()
                loss[sl] = out
        finally:
            h.set_eval_loss(False)             # a later forward or trajectory sizes its workspace as it always did
    return loss


def _step_euler(f, t0, t1, dt, y0):
    return y0 + dt * f(t0, y0)


def _step_midpoint(f, t0, t1, dt, y0):
    half_dt = 0.5 * dt
    f0 = f(t0, y0)
    y_mid = y0 + f0 * half_dt
    return y0 + dt * f(t0 + half_dt, y_mid)


def _step_rk4(f, t0, t1, dt, y0):          # the 3/8 rule
    k1 = f(t0, y0)
    k2 = f(t0 + dt * (1 / 3), y0 + dt * k1 * (1 / 3))
    k3 = f(t0 + dt * (2 / 3), y0 + dt * (k2 - k1 * (1 / 3)))
    k4 = f(t1, y0 + dt * (k1 - k2 + k3))
    return y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


# y1 = rule(f, t0, t1, dt, y0) with 0-dim f32 tensors t0, t1, dt = t1 - t0 on the state's device and f(t, y) the drift
STEP_RULES = {"euler": _step_euler, "midpoint": _step_midpoint, "rk4": _step_rk4}


# ---- the adaptive solve of an embedded Runge-Kutta pair (vc_flux_sample_dopri5 / vc_flux_sample_rk, csrc/rk_embedded.hip): the same
# rules in plain torch, for any callable - ONE step, error ratio, controller, initial-step search and loop (the _rk_* functions), each
# taking the pair's record; the public dopri5_* and rk_* names below are those at a record.  A method of S stages evaluates k1..kS
# per step; kS = f(t1, y1) is the next step's k1 (first same as last), so an attempt costs S - 1 evaluations.  The Dormand-Prince
# tableau is SciPy's RK45.C / .A / .B / .E plus torchdiffeq's DPS_C_MID, bosh3 SciPy's RK23.C / .A / .B / .E and adaptive_heun the
# closed form (tests/test_dopri5_cpu.py and tests/test_rk_embedded_cpu.py pin them, and single steps); the controller is
# torchdiffeq's as recalled - unpinned against real torchdiffeq, which was not available to check against.
DOPRI5_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)
DOPRI5_A = ((1 / 5,),
            (3 / 40, 9 / 40),
            (44 / 45, -56 / 15, 32 / 9),
            (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
            (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))
DOPRI5_B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)
DOPRI5_E = (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)
DOPRI5_C_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
                187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


class Dopri5Error(RuntimeError):
    """the adaptive solve gave up: a NaN error ratio, a step size that underflowed, or more than max_attempts attempts"""


def _dopri5_combine(row, ks):
    """sum of row[j] * ks[j] over the non-zero coefficients, left to right (csrc/rk_embedded.hip: rk_combine - the same bits in f32)"""
    acc = None
    for c, k in zip(row, ks):
        if c == 0.0:
            continue
        term = c * k
        acc = term if acc is None else acc + term
    return acc


def _f32(v: float) -> float:
    """a Python float rounded to f32: the scalar an f32 kernel argument holds"""
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def _scalar(v: float, y: torch.Tensor) -> float:
    return _f32(v) if y.dtype == torch.float32 else float(v)


def _rms(a) -> float:
    return float((a * a).mean().sqrt())


def _rk_norm(num: torch.Tensor, den: torch.Tensor) -> float:
    """sqrt(mean(q^2)) of q = num / den over all n elements, summed in q's dtype in the fixed order of csrc/rk_embedded.hip: single
    elements through `reduction.ordered_sum`.  For an f32 q this gives the kernel's bits; the callers form num and den on the CPU too."""
    q = num.reshape(-1) / den.reshape(-1)
    n = q.numel()
    mean = float(ordered_sum((q * q).reshape(n, 1)) / torch.tensor(float(n), dtype=torch.float64).to(q.dtype))
    # the square root in double, rounded once more for an f32 q: the correctly rounded f32 root (53 >= 2 * 24 + 2 bits), which
    # torch's vectorised CPU sqrt is not
    return math.sqrt(mean) if q.dtype == torch.float64 else _f32(math.sqrt(mean))


def dopri5_interp(y0, y1, ks, dt: float, theta: float):
    """The dense output at theta in [0, 1]: the quartic through (y0, f0, y_mid, y1, f1) as torchdiffeq fits and evaluates it; theta = 0
    and theta = 1 return y0 and y1 themselves.  For an f32 state the scalars are f32, as in csrc/rk_embedded.hip."""
    x = _scalar(theta, y0)
    if x == 0.0:
        return y0.clone()
    if x == 1.0:
        return y1.clone()
    f32 = y0.dtype == torch.float32
    h = _scalar(dt, y0)
    f0, f1 = ks[0], ks[6]
    y_mid = y0 + h * _dopri5_combine(DOPRI5_C_MID, ks)
    a = (2 * h * (f1 - f0) - 8 * (y1 + y0)) + 16 * y_mid
    b = ((h * (5 * f0 - 3 * f1) + 18 * y0) + 14 * y1) - 32 * y_mid
    c = ((h * (f1 - 4 * f0) - 11 * y0) - 5 * y1) + 16 * y_mid
    d = h * f0
    xp = x
    out = y0 + xp * d
    for coeff in (c, b, a):
        xp = _f32(xp * x) if f32 else xp * x          # (the product of two f32 values in double, rounded once: the f32 product)
        out = out + xp * coeff
    return out


def rk_hermite(y0, y1, ks, dt: float, theta: float):
    """The dense output of bosh3 / adaptive_heun at theta in [0, 1]: the cubic through (y0, f0 = k1, y1, f1 = kS),
    y = (1-x) y0 + x y1 + x (x-1) ((1-2x)(y1-y0) + (x-1) dt f0 + x dt f1), as the ONE sequence of operations csrc/rk_embedded.hip
    states; theta = 0 and theta = 1 return y0 and y1 themselves.  For an f32 state every scalar is formed in f32."""
    x = _scalar(theta, y0)
    if x == 0.0:
        return y0.clone()
    if x == 1.0:
        return y1.clone()
    f0, f1 = ks[0], ks[-1]
    if y0.dtype == torch.float32:
        xt, h, one = (torch.tensor(v, dtype=torch.float64).to(torch.float32) for v in (x, dt, 1.0))
        c1 = xt - one
        c0, c1, c2, w, h0, h1 = (float(v) for v in (one - xt, c1, one - 2 * xt, xt * c1, c1 * h, xt * h))
    else:
        c0, c1, c2 = 1.0 - x, x - 1.0, 1.0 - 2.0 * x
        w, h0, h1 = x * c1, c1 * dt, x * dt
    d = y1 - y0
    inner = (c2 * d + h0 * f0) + h1 * f1
    return (c0 * y0 + x * y1) + w * inner


# A pair's record.  c: the S stage times; a: the rows a2 .. a(S-1); b: forms y1 (= row aS); e: the S weights of the error estimate;
# interp: its dense output.  `name` (the prefix of its messages), `local` and `norm` say how the RMS norms are taken, and there are
# two ways, which differ in the last bits: _KERNEL_NORM, on CPU copies in the summation order of the kernel (vc_rk_error_ratio) - what
# every rk_* function does, Dormand-Prince included; and _TORCH_NORM, torch's mean() on the tensor's own device - what the dopri5_*
# functions do (_DOPRI5).  The fused Dormand-Prince solve is held to the latter on forced attempts (tests/test_dopri5_gpu.py).
_KERNEL_NORM = dict(name="rk", local=lambda v: v.detach().cpu(), norm=_rk_norm)
_TORCH_NORM = dict(name="dopri5", local=lambda v: v, norm=lambda num, den: _rms(num / den))
RK_TABLEAUS = {
    "dopri5": dict(code=0, order=5, c=DOPRI5_C + (1.0,), a=DOPRI5_A, b=DOPRI5_B, e=DOPRI5_E, interp=dopri5_interp, **_KERNEL_NORM),
    "bosh3": dict(code=1, order=3, c=(0.0, 1 / 2, 3 / 4, 1.0), a=((1 / 2,), (0.0, 3 / 4)), b=(2 / 9, 1 / 3, 4 / 9),
                  e=(5 / 72, -1 / 12, -1 / 9, 1 / 8), interp=rk_hermite, **_KERNEL_NORM),
    "adaptive_heun": dict(code=2, order=2, c=(0.0, 1.0, 1.0), a=((1.0,),), b=(1 / 2, 1 / 2), e=(1 / 2, -1 / 2, 0.0), interp=rk_hermite,
                          **_KERNEL_NORM),
}
_DOPRI5 = dict(RK_TABLEAUS["dopri5"], **_TORCH_NORM)
ADAPTIVE_METHODS = ("dopri5", "bosh3", "adaptive_heun")       # Sampler.sample_ode_adaptive(method=)


def _rk_tableau(method: str, solve: bool = False) -> dict:
    """the record behind the rk_* functions; solve: of rk_integrate, which leaves Dormand-Prince to dopri5_integrate"""
    if method not in RK_TABLEAUS or (solve and method == "dopri5"):
        raise ValueError(f"method {method!r}: one of {[m for m in RK_TABLEAUS if not (solve and m == 'dopri5')]} expected"
                         + (" (Dormand-Prince has one route: dopri5_integrate)" if method == "dopri5" else ""))
    return RK_TABLEAUS[method]


def _rk_step(tab, f, t: float, dt: float, y0: torch.Tensor, k1: torch.Tensor):
    h = _scalar(dt, y0)
    ks = [k1.to(y0.dtype)]
    for i, row in enumerate(tab["a"]):
        ks.append(f(t + tab["c"][i + 1] * dt, y0 + h * _dopri5_combine(row, ks)).to(y0.dtype))
    y1 = y0 + h * _dopri5_combine(tab["b"], ks)
    ks.append(f(t + dt, y1).to(y0.dtype))
    return y1, ks


def _rk_error_ratio(tab, y0, y1, ks, dt: float, rtol: float, atol: float) -> float:
    local = tab["local"]
    y0, y1, ks = local(y0), local(y1), [local(k) for k in ks]
    err = _scalar(dt, y0) * _dopri5_combine(tab["e"], ks)
    tol = _scalar(atol, y0) + _scalar(rtol, y0) * torch.maximum(y0.abs(), y1.abs())
    return tab["norm"](err, tol)


def _rk_controller(tab, dt: float, ratio: float):
    if ratio != ratio:
        raise Dopri5Error(f"{tab['name']}: the error ratio of a step of dt = {dt:.3g} is NaN")
    if ratio == 0.0:
        return True, dt * 10.0
    return ratio <= 1.0, dt * min(10.0, max(0.9 / math.pow(ratio, 1.0 / tab["order"]), 1.0 if ratio < 1.0 else 0.2))


def _rk_initial_step(tab, f, t0: float, y0, f0, rtol: float, atol: float) -> float:
    """Hairer's starting step size with the exponent 1 / order (one more evaluation)"""
    name, local, norm = tab["name"], tab["local"], tab["norm"]
    f0 = f0.to(y0.dtype)
    c0, cf0 = local(y0), local(f0)
    scale = _scalar(atol, y0) + _scalar(rtol, y0) * c0.abs()
    d0, d1 = norm(c0, scale), norm(cf0, scale)
    if d0 != d0 or d1 != d1:
        raise Dopri5Error(f"{name}: the state or the drift at the first time is not finite")
    h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    f1 = f(t0 + h0, y0 + _scalar(h0, y0) * f0).to(y0.dtype)
    d2 = norm(local(f1) - cf0, scale) / h0
    if d2 != d2:
        raise Dopri5Error(f"{name}: the drift at the first time + h0 is not finite")
    h1 = max(1e-6, h0 * 1e-3) if max(d1, d2) <= 1e-15 else math.pow(0.01 / max(d1, d2), 1.0 / tab["order"])
    return min(100.0 * h0, h1)


def _rk_integrate(tab, f, y0, t, rtol, atol, max_attempts, forced_dts, log, on_attempt) -> torch.Tensor:
    """the loop of dopri5_integrate and rk_integrate"""
    name = tab["name"]
    who = name + "_integrate"
    ts = [float(v) for v in (t.tolist() if torch.is_tensor(t) else t)]
    if len(ts) < 2 or any(b <= a for a, b in zip(ts, ts[1:])):
        raise ValueError(f"{who}: t must hold at least two strictly increasing times")
    if y0.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: an f32 or f64 state expected, got {y0.dtype}")
    log = log if log is not None else []
    tc = ts[0]
    k1 = f(tc, y0).to(y0.dtype)
    forced = None if forced_dts is None else list(forced_dts)
    dt = None if forced is not None else _rk_initial_step(tab, f, tc, y0, k1, rtol, atol)
    outs, nxt, attempts = [y0], 1, 0
    while nxt < len(ts):
        if forced is not None:
            if attempts >= len(forced):
                raise Dopri5Error(f"{name}: the {len(forced)} forced attempts end at t = {tc!r}, before t[{nxt}] = {ts[nxt]!r}")
            item = forced[attempts]
            dt, accept_as = (float(item[0]), bool(item[1])) if isinstance(item, (tuple, list)) else (float(item), None)
        if attempts >= max_attempts:
            raise Dopri5Error(f"{name}: more than max_attempts = {max_attempts} attempts (t = {tc!r}, dt = {dt:.3g})")
        if tc + dt == tc:
            raise Dopri5Error(f"{name}: the step size underflowed (t = {tc!r}, dt = {dt:.3g})")
        attempts += 1
        y1, ks = _rk_step(tab, f, tc, dt, y0, k1)
        ratio = _rk_error_ratio(tab, y0, y1, ks, dt, rtol, atol)
        if on_attempt is not None:
            on_attempt(tc, dt, y0, y1, ks)
        if forced is not None and accept_as is not None:
            accepted, dt_next = accept_as, None
            log.append((tc, dt, ratio, accepted))
        else:
            log.append((tc, dt, ratio, ratio <= 1.0))
            accepted, dt_next = _rk_controller(tab, dt, ratio)
        if accepted:
            t1 = tc + dt
            while nxt < len(ts) and ts[nxt] <= t1:
                outs.append(tab["interp"](y0, y1, ks, dt, min(1.0, max(0.0, (ts[nxt] - tc) / dt))))
                nxt += 1
            y0, k1, tc = y1, ks[-1], t1
        dt = dt_next
    return torch.stack(outs)


def dopri5_step(f, t: float, dt: float, y0: torch.Tensor, k1: torch.Tensor):
    """One Dormand-Prince step from (t, y0) with k1 = f(t, y0): -> (y1, [k1..k7]); k7 = f(t + dt, y1) is the next step's k1.
    Every k is converted to the state's dtype, every sum is taken left to right."""
    return _rk_step(_DOPRI5, f, t, dt, y0, k1)


def dopri5_error_ratio(y0, y1, ks, dt: float, rtol: float, atol: float) -> float:
    """sqrt(mean(((dt * sum e_i k_i) / (atol + rtol * max(|y0|, |y1|)))^2)) over ALL elements"""
    return _rk_error_ratio(_DOPRI5, y0, y1, ks, dt, rtol, atol)


def dopri5_controller(dt: float, ratio: float):
    """-> (accepted, dt_next): accept iff ratio <= 1; dt_next = 10 dt for ratio 0, else dt * min(10, max(0.9 / ratio^(1/5), 1 if
    ratio < 1 else 0.2)).  A NaN ratio raises Dopri5Error."""
    return _rk_controller(_DOPRI5, dt, ratio)


def dopri5_initial_step(f, t0: float, y0, f0, rtol: float, atol: float) -> float:
    """Hairer's starting step size for order 4 (one more evaluation)"""
    return _rk_initial_step(_DOPRI5, f, t0, y0, f0, rtol, atol)


def dopri5_integrate(f, y0: torch.Tensor, t, rtol: float = 1e-3, atol: float = 1e-6, max_attempts: int = 1000, forced_dts=None,
                     log: Optional[list] = None, on_attempt: Optional[Callable] = None) -> torch.Tensor:
    """The adaptive Dormand-Prince 5(4) solve of y' = f(t, y) from y(t[0]) = y0: -> [len(t), ...] = y at every t (t[0]: y0 itself;
    the others by dense output inside the accepted step that covers them - steps are not clamped to the output times, so f may be
    evaluated past t[-1]).  t: increasing Python floats (or a 1-d tensor); f takes a Python float and the state and returns the drift.
    The state keeps its dtype (f32 or f64); one step size serves the whole tensor.  `forced_dts`: replay a given attempt sequence -
    a list of dt, or of (dt, accepted) pairs, one per attempt: no initial-step search, no controller.  `log` (a list) receives
    (t, dt, ratio, accepted) per attempt; `on_attempt(t, dt, y0, y1, ks)` sees every attempt's tensors.  Raises Dopri5Error on a NaN ratio, an underflowed step or more than max_attempts attempts."""
    return _rk_integrate(_DOPRI5, f, y0, t, rtol, atol, max_attempts, forced_dts, log, on_attempt)


def rk_step(f, t: float, dt: float, y0: torch.Tensor, k1: torch.Tensor, method: str):
    """One step of the pair from (t, y0) with k1 = f(t, y0): -> (y1, [k1..kS]); kS = f(t + dt, y1) is the next step's k1.  Every k is
    converted to the state's dtype, every sum is taken left to right over the non-zero coefficients."""
    return _rk_step(_rk_tableau(method), f, t, dt, y0, k1)


def rk_error_ratio(y0, y1, ks, dt: float, rtol: float, atol: float, method: str) -> float:
    """sqrt(mean(((dt * sum e_i k_i) / (atol + rtol * max(|y0|, |y1|)))^2)) over ALL elements, in the kernel's summation order"""
    return _rk_error_ratio(_rk_tableau(method), y0, y1, ks, dt, rtol, atol)


def rk_controller(dt: float, ratio: float, order: int):
    """-> (accepted, dt_next): dopri5_controller with the exponent 1 / order (at order 5 the same bits).  A NaN ratio raises."""
    return _rk_controller(dict(_KERNEL_NORM, order=order), dt, ratio)


def rk_initial_step(f, t0: float, y0, f0, rtol: float, atol: float, order: int) -> float:
    """dopri5_initial_step with the exponent 1 / order and the norms in the kernel's summation order (one more evaluation)"""
    return _rk_initial_step(dict(_KERNEL_NORM, order=order), f, t0, y0, f0, rtol, atol)


def rk_integrate(f, y0: torch.Tensor, t, method: str, rtol: float = 1e-3, atol: float = 1e-6, max_attempts: int = 1000, forced_dts=None,
                 log: Optional[list] = None, on_attempt: Optional[Callable] = None) -> torch.Tensor:
    """dopri5_integrate for the pair `method` ("bosh3" | "adaptive_heun"): the same loop, arguments, log and errors (Dopri5Error), the
    outputs read off the Hermite cubic of the accepted step that covers them.  For an f32 state every bit - states, ratios, step
    sizes - is the fused loop's (vc_flux_sample_rk)."""
    return _rk_integrate(_rk_tableau(method, solve=True), f, y0, t, rtol, atol, max_attempts, forced_dts, log, on_attempt)


# ---- the stochastic (SDE) sampler (vc_sde_plan / vc_sde_stage / vc_flux_sample_sde).  Time runs as in sample_ode: t = 0 noise, t = 1
# data; Linear path alpha = t, sigma = 1 - t.  With v the velocity and w(t) the diffusion coefficient:
#   score s = (t v - x) / (1 - t);   sde drift D(x, t) = v + w s = A v - Bc x,  A = 1 + w t / (1 - t),  Bc = w / (1 - t)
# so every update is one row of y + h (A v - Bc y) + g z.  The coefficients are computed in double, operation by operation as in
# csrc/sde_plan.hip, and rounded once to f32.
SDE_FORMS = ("constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")     # (the reference's spelling of the last)
SDE_METHODS = ("Euler", "Heun")
SDE_LAST_STEPS = ("Mean", "Euler", "Tweedie")


def _div(a: float, b: float) -> float:
    """a / b as IEEE double division gives it (inf / NaN for b == 0, where Python raises)"""
    if b != 0.0:
        return a / b
    return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a: float) -> float:
    return math.sqrt(a) if a >= 0.0 else math.nan


def sde_diffusion(form: str, norm: float, t: float) -> float:
    """w(t) of transport/path.py's ICPlan.compute_diffusion for the Linear path, in double"""
    if form == "constant":
        return norm
    if form == "SBDM":
        return _div(norm * (1.0 - t), t)
    if form in ("sigma", "linear"):
        return norm * (1.0 - t)
    if form == "decreasing":
        u = norm * math.cos(math.pi * t) + 1.0
        return 0.25 * (u * u)
    s = math.sin(math.pi * t)
    return norm * (s * s)


def sde_plan(method: str, form: str, norm: float, last_step, last_step_size: float, t) -> dict:
    """The host rule of the stochastic sampler, bit for bit vc_sde_plan (hip.sde_plan): the f32 time grid `t` (n points) ->
    {"rows": f32 [n_rows, 5] = (mode, h, A, Bc, g) per evaluation - for "Heun" one more row behind them, the injection of draw 0 -,
    "rows64": the same coefficients before their rounding to f32 (what an f64 state is stepped with), "times": f32 [evals] = the model
    times 1 - t, "evals": Euler (n - 1) + (last step ? 1 : 0), Heun 2 (n - 1) + (last step ? 1 : 0), "draws": n - 1}.
    NotImplementedError for an unknown method / form / last step; ValueError for a grid that does not increase strictly and for ANY
    non-finite coefficient (SBDM at t = 0 - it needs a sample_eps; any row at t = 1, hence Heun without a last step)."""
    import numpy as np
    if method not in SDE_METHODS:
        raise NotImplementedError(f"sde_plan: unknown method {method!r} {SDE_METHODS}")
    if form == "increasing-decreasing":
        form = "inccreasing-decreasing"
    if form not in SDE_FORMS:
        raise NotImplementedError(f"sde_plan: unknown diffusion form {form!r} {SDE_FORMS}")
    if last_step is not None and last_step != "" and last_step not in SDE_LAST_STEPS:
        raise NotImplementedError(f"sde_plan: unknown last step {last_step!r} ({SDE_LAST_STEPS}, or None)")
    last_step = last_step or None
    t32 = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32).reshape(-1)
    n = int(t32.size)
    if n < 2 or not bool(np.all(t32[1:] > t32[:-1])):
        raise ValueError("sde_plan: t must hold at least two strictly increasing times")
    norm, lss, S = float(norm), float(last_step_size), n - 1
    tt = [float(v) for v in t32]
    dts = [float(np.float32(t32[i + 1] - t32[i])) for i in range(S)]
    rows64, times = [], []

    def A(w, tv):
        return 1.0 + _div(w * tv, 1.0 - tv)

    def Bc(w, tv):
        return _div(w, 1.0 - tv)

    def noise(i):
        return _sqrt(2.0 * sde_diffusion(form, norm, tt[i]) * dts[i])

    with np.errstate(all="ignore"):
        def put(mode, h, a, b, g, tv, timed=True):
            row = (mode, h, a, b, g)
            for name, c in zip(("h", "A", "Bc", "g"), row[1:]):
                if not math.isfinite(float(np.float32(c))):
                    raise ValueError(f"sde_plan: the coefficient {name} = {c!r} at t = {tv!r} is not finite with diffusion form {form!r} "
                                     "(SBDM needs t > 0 - a sample_eps; every form needs t < 1 - a last step, or an end time below 1)")
            rows64.append(tuple(float(c) for c in row))
            if timed:
                times.append(np.float32(1.0) - np.float32(tv))

        for i in range(S):
            tv, dt = tt[i], dts[i]
            w = sde_diffusion(form, norm, tv)
            if method == "Euler":
                put(hip.SDE_EM, dt, A(w, tv), Bc(w, tv), noise(i), tv)
            else:
                put(hip.SDE_HEUN1, dt, A(w, tv), Bc(w, tv), 0.0, tv)
                t2 = tv + dt
                w2 = sde_diffusion(form, norm, t2)
                put(hip.SDE_HEUN2, 0.5 * dt, A(w2, t2), Bc(w2, t2), noise(i + 1) if i + 1 < S else 0.0, t2)
        if last_step is not None:
            t1 = tt[S]
            w = sde_diffusion(form, norm, t1)
            if last_step == "Mean":
                put(hip.SDE_LAST, lss, A(w, t1), Bc(w, t1), 0.0, t1)
            else:
                put(hip.SDE_LAST, lss if last_step == "Euler" else 1.0 - t1, 1.0, 0.0, 0.0, t1)
        evals = len(rows64)
        if method == "Heun":
            put(hip.SDE_INJECT, 0.0, 0.0, 0.0, noise(0), tt[0], timed=False)
        rows = np.array(rows64, dtype=np.float64).astype(np.float32)
    return {"rows": rows, "rows64": rows64, "times": np.array(times, dtype=np.float32), "evals": evals, "draws": S, "method": method}


def sde_integrate(f, x: torch.Tensor, plan: dict, noise: Callable) -> torch.Tensor:
    """The stochastic sampler as literal torch expressions - what vc_sde_stage computes, operation by operation (an f32 state gives
    the kernel's bits) - for any callable and any float dtype: -> [n_points, ...], x' after every loop step and the last step's result
    as the final row (without a last step it repeats the state).  f(tau, y) is the MODEL's output for the state y at the model time
    tau = 1 - t (a Python float); the velocity is -f.  noise(d, shape) supplies draw d (d = solver step index).  An f64 state is
    stepped with the double coefficients (plan["rows64"]), anything else with the f32 rows; g == 0 adds no noise term."""
    n_evals = plan["evals"]
    rows = plan["rows64"] if x.dtype == torch.float64 else [tuple(float(c) for c in r) for r in plan["rows"]]

    def z(d):
        return noise(d, x.shape).to(device=x.device, dtype=x.dtype)

    y, xhat, k1, outs = x, None, None, []
    y_in = y
    if len(rows) > n_evals:                        # Heun: draw 0 goes in ahead of the first evaluation
        g = rows[n_evals][4]
        xhat = y + g * z(0) if g != 0.0 else y
        y_in = xhat
    for e in range(n_evals):
        mode, h, A, Bc, g = rows[e]
        mode = int(mode)
        vel = (-f(float(plan["times"][e]), y_in)).to(x.dtype)
        if mode in (hip.SDE_EM, hip.SDE_LAST):
            y = y + h * (A * vel - Bc * y)
            if mode == hip.SDE_EM and g != 0.0:
                y = y + g * z(e)
            y_in = y
            outs.append(y)
        elif mode == hip.SDE_HEUN1:
            k1 = A * vel - Bc * xhat
            y = xhat + h * k1
            y_in = y
        else:                                      # SDE_HEUN2: the step's end, and the NEXT step's noise
            y = xhat + h * (k1 + (A * vel - Bc * y))
            xhat = y + g * z((e + 1) // 2) if g != 0.0 else y
            y_in = xhat
            outs.append(y)
    if len(outs) == plan["draws"]:                 # no last step
        outs.append(y)
    return torch.stack(outs)


MS_MAX_ORDER = 4


def ms_plan(order: int, t, rounded: bool = True) -> dict:
    """The host rule of the Adams-Bashforth multistep solve, bit for bit vc_ms_plan (hip.ms_plan): the f32 time grid `t` (n points) and
    the order (1..4) -> {"rows": [n - 1, 4] = c_{i,0..3} per step, "times": f32 [n - 1] = the model times 1 - t_i, "evals": n - 1}.
    Step i uses k = min(order, i + 1) nodes tau_j = t_{i-j}; c_{i,j} = the integral over [t_i, t_{i+1}] of the Lagrange polynomial of
    node j, computed in double from the widened f32 grid values - in u = (tau - t_i) / h the numerator is multiplied out factor by
    factor, integrated term by term, divided by the running product of the node differences and scaled by h - and rounded ONCE to f32;
    unused entries are exactly 0.  rounded=False: "rows" holds the double coefficients (what an f64 state is stepped with).
    ValueError for an order outside 1..4, fewer than two points, a grid that does not increase strictly and any non-finite
    coefficient."""
    import numpy as np
    if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= MS_MAX_ORDER:
        raise ValueError(f"ms_plan: order = {order!r} outside 1..{MS_MAX_ORDER}")
    t32 = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32).reshape(-1)
    n = int(t32.size)
    if n < 2:
        raise ValueError(f"ms_plan: n_points = {n}, at least 2 expected")
    if not bool(np.all(t32[1:] > t32[:-1])):
        raise ValueError("ms_plan: t must increase strictly")
    tt = [float(v) for v in t32]
    rows64 = []
    for i in range(n - 1):
        k = min(order, i + 1)
        ti = tt[i]
        h = tt[i + 1] - ti
        b = [(tt[i - m] - ti) / h for m in range(k)]
        row = [0.0] * MS_MAX_ORDER
        for j in range(k):
            p, den = [1.0], 1.0
            for m in range(k):
                if m == j:
                    continue
                deg = len(p) - 1
                q = [-(b[m] * p[0])] + [p[d - 1] - b[m] * p[d] for d in range(1, deg + 1)] + [p[deg]]
                p = q
                den = den * (b[j] - b[m])
            integral = 0.0
            for d, pd in enumerate(p):
                integral = integral + pd / float(d + 1)
            c = h * _div(integral, den)
            with np.errstate(all="ignore"):
                finite = math.isfinite(float(np.float32(c)))
            if not finite:
                raise ValueError(f"ms_plan: the coefficient c[{i}][{j}] = {c!r} of the step from t = {ti!r} to {tt[i + 1]!r} is not finite "
                                 f"(order {order})")
            row[j] = c
        rows64.append(row)
    rows = np.array(rows64, dtype=np.float64).reshape(n - 1, MS_MAX_ORDER)
    return {"rows": rows.astype(np.float32) if rounded else rows, "times": np.float32(1.0) - t32[:-1], "evals": n - 1, "order": order}


def multistep_integrate(f, y0: torch.Tensor, t, order: int) -> torch.Tensor:
    """The Adams-Bashforth multistep solve as literal torch expressions - what vc_ms_stage computes, operation by operation (an f32
    state gives the kernel's bits) - for any callable and an f32 or f64 state: -> [n_points, ...], y0 and the state after every step.
    f(t_i, y) is the DRIFT for the state y at the grid time t_i (a Python float, the widened f32 value); ONE call per step, its result
    is kept as returned (a bf16 velocity stays bf16) and widened where a later step uses it.  Step i:
        y <- y + (((c0 f_i) + c1 f_{i-1}) + c2 f_{i-2}) + c3 f_{i-3}
    left to right; a coefficient c_j, j >= 1, that is exactly zero adds no term.  An f64 state is stepped with the double coefficients
    (ms_plan(rounded=False)), an f32 state with the f32 rows."""
    if y0.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"multistep_integrate: an f32 or f64 state expected, got {y0.dtype}")
    plan = ms_plan(order, t, rounded=y0.dtype != torch.float64)
    t32 = t.detach().cpu().to(torch.float32).reshape(-1) if torch.is_tensor(t) else torch.tensor(t, dtype=torch.float32).reshape(-1)
    y, past, outs = y0, [], [y0]
    for i in range(plan["evals"]):
        c0, c1, c2, c3 = (float(c) for c in plan["rows"][i])
        past.insert(0, f(float(t32[i]), y))
        del past[MS_MAX_ORDER:]
        fs = [past[j].to(y0.dtype) if j < len(past) else None for j in range(MS_MAX_ORDER)]
        z = c0 * fs[0]
        if c1 != 0.0:
            z = z + c1 * fs[1]
        if c2 != 0.0:
            z = z + c2 * fs[2]
        y = y + z
        if c3 != 0.0:
            y = y + c3 * fs[3]
        outs.append(y)
    return torch.stack(outs)


class StepCache:
    """Opt-in first-block step cache of the fused Euler loop (vc_flux_set_step_cache).  IT CHANGES RESULTS: an
    evaluation whose first-block residual moved by less than `threshold` (relative L1 against the last computed evaluation's) is
    replaced by that evaluation's remaining-blocks residual; at most `max_consecutive` evaluations in a row (-1: no limit).  Its
    effect on image quality is unmeasured and no default threshold is recommended, hence none is offered."""
    __slots__ = ("threshold", "max_consecutive")

    def __init__(self, threshold: float, max_consecutive: int = 1):
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
            raise TypeError(f"StepCache: threshold must be a number, got {type(threshold).__name__}")
        if isinstance(max_consecutive, bool) or not isinstance(max_consecutive, int):
            raise TypeError(f"StepCache: max_consecutive must be an int, got {type(max_consecutive).__name__}")
        if math.isnan(threshold) or threshold <= 0:
            raise ValueError(f"StepCache: threshold must be positive (inf allowed), got {threshold}; pass step_cache=None for off")
        if max_consecutive == 0 or max_consecutive < -1:
            raise ValueError(f"StepCache: max_consecutive must be >= 1, or -1 for no limit, got {max_consecutive}")
        object.__setattr__(self, "threshold", float(threshold))
        object.__setattr__(self, "max_consecutive", int(max_consecutive))

    def __setattr__(self, k, v):
        raise AttributeError("StepCache is immutable")

    def __repr__(self):
        return f"StepCache(threshold={self.threshold!r}, max_consecutive={self.max_consecutive})"

    def __eq__(self, o):
        return isinstance(o, StepCache) and (self.threshold, self.max_consecutive) == (o.threshold, o.max_consecutive)

    def __hash__(self):
        return hash((self.threshold, self.max_consecutive))


def _classify(model: Callable, model_kwargs: dict):
    """-> (owner, kind, kw, cfg_scale): kind "forward" / "forward_with_cfg" = that bound method of a visualcloze_amd.Flux (owner), else
    "foreign"; kw a copy of model_kwargs, for forward_with_cfg without its "cfg_scale" (which is None otherwise)"""
    from .model import Flux
    owner, name, kw = getattr(model, "__self__", None), getattr(model, "__name__", ""), dict(model_kwargs)
    if not isinstance(owner, Flux) or name not in ("forward", "forward_with_cfg"):
        return owner, "foreign", kw, None
    return owner, name, kw, float(kw.pop("cfg_scale", 1.0)) if name == "forward_with_cfg" else None


def _route(model: Callable, model_kwargs: dict, x: torch.Tensor, method: str, step_cache: Optional[StepCache] = None):
    """What a sampler method branches on, once: -> (owner, kw, cfg_scale, fused, eager).  owner, kw (without "cfg_scale") and cfg_scale
    as `_classify`; fused: the fused loop of `owner` runs (`_fusable` / `_cfg_fusable`); eager: the callable stepped on the host
    otherwise - the foreign callable itself, and for a visualcloze_amd.Flux its forward (true CFG: forward_with_cfg at cfg_scale) with
    the velocity rounded to bf16, as the reference's is under autocast (visualcloze.py:363) whatever dtype Flux.forward hands back to
    its caller.  method: a STEP_RULES name of the fixed grid - "euler" alone may run on the Python-ordered plan - or the family
    "adaptive" / "sde" / "multistep", which needs the C handle.  step_cache (sample_ode's): never silently ignored - only the C
    handle's Euler loop over Flux.forward implements it, every other route raises."""
    owner, kind, kw, cfg_scale = _classify(model, model_kwargs)
    if kind == "foreign":
        if step_cache is not None:
            raise ValueError("step_cache: only the fused loop of a visualcloze_amd.Flux implements it, not a foreign callable")
        return owner, kw, None, False, model
    if kind == "forward_with_cfg":
        if step_cache is not None:
            raise ValueError("step_cache works with Flux.forward only, not with forward_with_cfg (true CFG)")
        # eager: unequal image masks within a pair, no C handle, an f16 / f64 state
        return (owner, kw, cfg_scale, _cfg_fusable(owner, x, method, kw),
                lambda xin, **k: owner.forward_with_cfg(xin, cfg_scale=cfg_scale, **k).to(torch.bfloat16))
    fused = _fusable(owner, x, method)
    if step_cache is not None:
        if owner.handle() is None:
            raise ValueError("step_cache needs the C handle: not available with lora_mode='ref' (unless ref_plan='handle') "
                             "or the Python-ordered plan (use_handle False)")
        if not fused:
            raise ValueError(f"step_cache: a {x.dtype} state is stepped eagerly, where no cache exists")
    return owner, kw, None, fused, lambda xin, **k: model(xin, **k).to(torch.bfloat16)


def _ode_interval(transport: Transport, reverse: bool, strength: Optional[float]):
    """-> (t0, t1) of the three ODE methods: check_interval, the start moved by `strength`, forward time"""
    t0, t1 = transport.check_interval(reverse=reverse)
    if strength is not None:
        t0 = (t1 - t0) * strength + t0
    assert t0 < t1, "ODE sampler has to be in forward time"
    return t0, t1


class Sampler:
    def __init__(self, transport: Transport):
        self.transport = transport
        self.last_step_cache_stats = None      # of the last cached trajectory this sampler ran: one dict per chunk of samples
        self.last_adaptive_log = None          # of the last sample_ode_adaptive run: one dict per chunk of samples

    def sample_ode(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, reverse=False,
                   do_shift=True, time_shifting_factor=None, strength=None, return_trajectory: bool = False,
                   step_cache: Optional[StepCache] = None):
        if sampling_method not in STEP_RULES:
            raise NotImplementedError(f"solver {sampling_method!r}: only the fixed-grid solvers {sorted(STEP_RULES)} are implemented "
                                      "(no adaptive or multistep methods)")
        if step_cache is not None:
            if not isinstance(step_cache, StepCache):
                raise TypeError(f"step_cache must be a StepCache or None, got {type(step_cache).__name__}")
            if sampling_method != "euler":
                raise ValueError(f"step_cache works with sampling_method='euler' only, not {sampling_method!r}")
        t0, t1 = _ode_interval(self.transport, reverse, strength)

        def _sample(x: torch.Tensor, model: Callable, model_kwargs: dict) -> torch.Tensor:
            t = solver_time_grid(num_steps, x.shape[1], t0, t1, do_shift, time_shifting_factor)
            owner, kw, cfg_scale, fused, eager = _route(model, model_kwargs, x, sampling_method, step_cache)
            if fused:
                return _sample_fused(owner, x, kw, t, return_trajectory, sampling_method, step_cache, self, cfg_scale=cfg_scale)
            return _sample_foreign(eager, x, kw, t, return_trajectory, sampling_method)      # (dt * f stays a bf16 product for a Flux)

        return _sample

    def sample_ode_adaptive(self, *, num_steps=50, atol=1e-6, rtol=1e-3, reverse=False, do_shift=True, time_shifting_factor=None,
                            strength=None, return_trajectory: bool = False, max_attempts: int = 1000, method: str = "dopri5"):
        """The error-controlled solve the reference's sample_ode defaults to (sampling_method="dopri5", atol, rtol), under a name of
        its own: sample_ode("dopri5") keeps raising.  Adaptive Dormand-Prince 5(4) (`dopri5_integrate`); `num_steps` only places the
        OUTPUT times - the solver chooses its own steps and reads the outputs off its dense output.  Fused (vc_flux_sample_dopri5:
        replays of one captured evaluation, one 4-byte host read per attempt) for the bound forward / forward_with_cfg of a
        visualcloze_amd.Flux that has the C handle and a bf16 or f32 state, eager otherwise.  The state is stepped in f32 (f64 for an
        f64 caller) and rounded once per output.  `sampler.last_adaptive_log` holds, per chunk of samples,
        {"attempts": [(t, dt, ratio, accepted)], "evaluations", "rejected"} of the last run.
        `method`: "dopri5" (the default: the path above, untouched), or one of the cheaper embedded pairs "bosh3" (Bogacki-Shampine
        3(2)) / "adaptive_heun" (2(1)) - `rk_integrate`, fused through vc_flux_sample_rk under the same conditions, eager otherwise;
        evaluations per attempt: 6 / 3 / 2.  Their controller is torchdiffeq's as recalled, unpinned against real torchdiffeq."""
        if method not in ADAPTIVE_METHODS:
            raise ValueError(f"sample_ode_adaptive: method {method!r}: one of {list(ADAPTIVE_METHODS)} expected")
        t0, t1 = _ode_interval(self.transport, reverse, strength)

        def _sample(x: torch.Tensor, model: Callable, model_kwargs: dict) -> torch.Tensor:
            t = solver_time_grid(num_steps, x.shape[1], t0, t1, do_shift, time_shifting_factor)
            owner, kw, cfg_scale, fused, eager = _route(model, model_kwargs, x, "adaptive")
            if fused:
                out, logs = _sample_adaptive_fused(owner, x, kw, t, return_trajectory, rtol, atol, max_attempts, cfg_scale, method=method)
            else:
                out, log = _sample_adaptive_foreign(eager, x, kw, t, return_trajectory, rtol, atol, max_attempts, method=method)
                logs = [log]
            self.last_adaptive_log = logs
            return out

        return _sample

    def sample_ode_multistep(self, *, order: int = 2, num_steps=50, reverse=False, do_shift=True, time_shifting_factor=None, strength=None,
                             return_trajectory: bool = False):
        """A fixed-grid, variable-step Adams-Bashforth solve of `order` 1..4 on sample_ode's own (time-shifted) grid, under a name of
        its own: sample_ode("adams") keeps raising.  ONE model evaluation per step - the velocities of the last steps are reused; the
        first steps run at the orders 1, 2, ... (no extra evaluations).  Returns `_sample(x, model, model_kwargs)` -> [1, B, N, C], or
        [num_steps, B, N, C] with return_trajectory (the start state, then the state after every step), in the caller's dtype.
        Fused (vc_flux_sample_multistep: replays of one captured evaluation, whatever the order) for the bound forward /
        forward_with_cfg of a visualcloze_amd.Flux that has the C handle and a bf16 or f32 state, eager (`multistep_integrate`)
        otherwise.  The state is stepped in f32 (f64 for an f64 caller) and rounded once per output.
        Order 1 is Euler's rule with f32 roundings (not bit-equal to sample_ode("euler"), whose step multiplies by bf16(dt)); orders
        3 and 4 have small stability regions and no order is recommended; image quality at any order is unmeasured."""
        if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= MS_MAX_ORDER:
            raise ValueError(f"sample_ode_multistep: order = {order!r} outside 1..{MS_MAX_ORDER}")
        t0, t1 = _ode_interval(self.transport, reverse, strength)

        def _sample(x: torch.Tensor, model: Callable, model_kwargs: dict) -> torch.Tensor:
            t = solver_time_grid(num_steps, x.shape[1], t0, t1, do_shift, time_shifting_factor)
            owner, kw, cfg_scale, fused, eager = _route(model, model_kwargs, x, "multistep")
            if fused:
                return _sample_multistep_fused(owner, x, kw, t, order, return_trajectory, cfg_scale)
            return _sample_multistep_foreign(eager, x, kw, t, order, return_trajectory)

        return _sample

    def sample_sde(self, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04,
                   num_steps=250, sample_eps=None, rng=None, return_trajectory: bool = False):
        """The reference's stochastic sampler (transport.py:300-359; names, defaults and call shape are its own): returns
        `_sample(init, model, **model_kwargs)` -> [1, B, N, C], or [num_steps, B, N, C] with return_trajectory (x' after every loop
        step, then the last step's result), in the caller's dtype; `[-1]` is the sample, as with the reference's list.
        sampling_method "Euler" (Euler-Maruyama) | "Heun"; diffusion_form: one of SDE_FORMS; last_step "Mean" | "Euler" | "Tweedie" |
        None.  The mathematics is applied to the velocity -model(x || cond, timesteps = 1 - t), the adaptation the reference made for
        sample_ode only.  Interval as `Transport.check_interval(sde=True)`: t0 = eps for SBDM else 0, t1 = 1 - last_step_size with a
        last step else 1 - eps, eps = `sample_eps` if given else the transport's 0; the grid is linspace(t0, t1, num_steps).  The
        reference's default (SBDM, eps 0) is infinite at t = 0: here it raises a ValueError naming sample_eps, as does every setting
        with a non-finite coefficient (Heun without a last step) - never a NaN latent.
        Fused (vc_flux_sample_sde) for the bound forward / forward_with_cfg of a visualcloze_amd.Flux that has the C handle and a bf16 /
        f32 state, per chunk of samples; eager (`sde_integrate`) otherwise.  The state is stepped in f32 (f64 for an f64 caller) and
        rounded once per output.
        rng: a `pipeline.NoiseStream` - draw d of a chunk takes the stream positions offset + d * n + i, n the chunk's elements and i
        the flat index in the chunk's [B, N, C] state IN THE HANDLE'S ROW ORDER (image rows valid-first per sample: for all-ones image
        masks the caller's order); its offset advances by draws * elements, chunk after chunk.  rng=None: a seed is drawn from
        torch's default generator, so torch.manual_seed reproduces.  The eager path of a CUDA state draws the same stream for the
        whole batch in the caller's order; a foreign callable on the CPU draws with torch.randn.
        Image quality under any diffusion_form is unmeasured (only random-init weights exist here)."""
        if last_step is None:
            last_step_size = 0.0
        t0, t1 = self.transport.check_interval(sde=True, diffusion_form=diffusion_form, last_step_size=last_step_size, sample_eps=sample_eps)
        assert t0 < t1, "SDE sampler has to be in forward time"
        t = torch.linspace(t0, t1, num_steps)
        plan = sde_plan(sampling_method, diffusion_form, diffusion_norm, last_step, last_step_size, t)     # every refusal, up front
        setting = (sampling_method, diffusion_form, float(diffusion_norm), last_step, float(last_step_size))

        def _sample(init: torch.Tensor, model: Callable, **model_kwargs) -> torch.Tensor:
            x = init
            owner, kw, cfg_scale, fused, eager = _route(model, model_kwargs, x, "sde")
            total = plan["draws"] * x.numel()
            if rng is not None:
                if hasattr(rng, "threads_per_sm"):            # a pipeline.TorchNoiseStream: its offset counts Philox outputs, not elements
                    raise ValueError("sample_sde: the stochastic sampler draws inside the step from the library's own stream (vc_sde_stage), "
                                     "which a TorchNoiseStream does not restate: pass rng=NoiseStream(seed)")
                if not x.is_cuda:
                    raise ValueError("sample_sde: a NoiseStream draws on the device; a CPU state draws with torch.randn (rng=None)")
                seed, offset = int(rng.seed), int(rng.offset)
                if offset + total > 1 << 64:
                    raise ValueError(f"sample_sde: {total} elements at offset {offset} leave the 64-bit stream")
            else:
                seed, offset = int(torch.randint(0, (1 << 63) - 1, (1,)).item()), 0
            if fused:
                out = _sample_sde_fused(owner, x, kw, t, plan, setting, seed, offset, return_trajectory, cfg_scale)
            else:
                out = _sample_sde_foreign(eager, x, kw, plan, seed, offset, return_trajectory)
            if rng is not None:
                rng.offset = offset + total
            return out

        return _sample


def _times_as_state(ti, y):
    """the fixed grid's `timesteps` (transport.py:193-198,384): ones(B) * t with t a 0-dim tensor rounded to the state's dtype, then 1 - t"""
    tt = torch.ones(y.size(0), device=y.device) * _solver_t_as_state(ti, y)
    return torch.ones_like(tt) * (1 - tt)


def _times_f32(t, y):
    """`timesteps` = 1 - f32(t) for a Python-float t, the f32 subtraction (vcloze_hip.h: the adaptive and the multistep solve)"""
    tm = torch.tensor(1.0) - torch.tensor(t, dtype=torch.float64).to(torch.float32)
    return torch.ones(y.size(0), device=y.device) * tm.to(y.device)


def _times_tau(tau, y):
    """`timesteps` = the model time tau the stochastic sampler's plan holds (a Python float)"""
    return torch.ones(y.size(0), device=y.device) * tau


def _drift(model, dtype, kw, times, sign=-1, bf16_out=False, solver="ODE"):
    """f(t, y) = sign * model(y in `dtype` || cond, timesteps = times(t, y), **kw) - THE drift of every eager solve; what differs
    between them is the dtype the model sees the state in (the caller's; None: the solver's own, as it comes), the sign (the
    stochastic sampler takes the model's output itself), how the solver's time becomes `timesteps` (`_times_*`) and whether the
    output is rounded to bf16 (bf16_out: a Flux velocity that `_route` has not rounded)"""
    cond = kw.pop("cond", None)

    def f(t, y):
        ym = y if dtype is None else y.to(dtype)
        xin = torch.cat((ym, cond), dim=-1) if cond is not None else ym
        v = model(xin, timesteps=times(t, y), **kw)
        assert v.shape == y.shape, f"Output shape from {solver} solver must match input shape"
        v = v.to(torch.bfloat16) if bf16_out else v
        return -v if sign < 0 else v
    return f


def _sample_eager(x, return_trajectory, integrate):
    """What the eager adaptive, stochastic and multistep solves share: integrate(y0) -> [rows, ...] on the whole batch with the state
    in f32 (f64 for an f64 caller), rounded once per output; the whole trajectory or its last row"""
    out = integrate(x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float32)).to(x.dtype)
    return out if return_trajectory else out[-1:]


def _sample_multistep_foreign(model, x, kw, t, order, return_trajectory, bf16_out=False):
    """Any callable: transport.multistep_integrate through `_sample_eager`"""
    drift = _drift(model, x.dtype, kw, _times_f32, bf16_out=bf16_out)
    return _sample_eager(x, return_trajectory, torch.no_grad()(lambda y0: multistep_integrate(drift, y0, t.to(torch.float32), order)))


def _sample_sde_foreign(model, x, kw, plan, seed, offset, return_trajectory, bf16_out=False):
    """Any callable: transport.sde_integrate through `_sample_eager`"""
    f = _drift(model, x.dtype, kw, _times_tau, sign=1, bf16_out=bf16_out, solver="SDE")

    def noise(d, shape):
        if not x.is_cuda:
            return torch.randn(shape, dtype=torch.float32)
        return hip.randn(tuple(shape), seed, offset + d * x.numel(), dtype=torch.float32, device=x.device)

    return _sample_eager(x, return_trajectory, torch.no_grad()(lambda y0: sde_integrate(f, y0, plan, noise)))


def _log_dict(attempts, evaluations):
    return {"attempts": list(attempts), "evaluations": evaluations, "rejected": sum(1 for a in attempts if not a[3])}


def _sample_adaptive_foreign(model, x, kw, t, return_trajectory, rtol, atol, max_attempts, bf16_out=False, forced_dts=None,
                             on_attempt=None, method="dopri5"):
    """Any callable: transport.dopri5_integrate (method "dopri5") or rk_integrate through `_sample_eager` (not under no_grad, as ever)"""
    calls = []
    drift = _drift(model, x.dtype, kw, _times_f32, bf16_out=bf16_out)
    f = lambda tt, y: (calls.append(tt), drift(tt, y))[1]  # noqa: E731
    log = []
    tab = _DOPRI5 if method == "dopri5" else _rk_tableau(method, solve=True)
    out = _sample_eager(x, return_trajectory,
                        lambda y0: _rk_integrate(tab, f, y0, t.to(torch.float32), rtol, atol, max_attempts, forced_dts, log, on_attempt))
    return out, _log_dict(log, len(calls))


@contextmanager
def _on_capture_stream(st):
    """run on the plan's capture stream `st`: behind torch's current stream, which waits for it afterwards - on failure too"""
    st.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(st):
            yield st.cuda_stream
    finally:
        torch.cuda.current_stream().wait_stream(st)


def _solve_begin(flux, x, kw, S, return_trajectory, pairs=False):
    """-> (ChunkPlan, cond, out [B, N, C], traj [S, B, N, C] or None) of a fused solve of the state x"""
    B, N, C = x.shape
    cond = kw.get("cond")
    if cond is None:
        raise hip.VclozeHipError("fused sampler expects model_kwargs['cond'] (x || cond feeds img_in)")
    plan = flux.chunk_plan(B, N, kw, pairs, channels=(C, cond.shape[-1]))
    out = torch.empty(B, N, C, dtype=x.dtype, device=plan.dev)
    return plan, cond, out, torch.empty(S, B, N, C, dtype=x.dtype, device=plan.dev) if return_trajectory else None


def _solve_on_handle(flux, h, x, kw, S, return_trajectory, max_evals, run, step_cache=None, cfg_scale=None, buffers=None,
                     prepend_start=True):
    """What the fused solves through the C handle share.  Per trajectory: the options, taken back on failure too.  Per chunk of samples
    (true CFG: whole pairs (j, j + B/2), conditional samples first): vc_flux_prepare for `max_evals` evaluations, a copy of the state's
    rows in kernel order for run(xs, cond rows, trajectory buffer [S, bs, N, C] or None, stream) to advance in place, and the way back.
    buffers: the workspace option the solve needs (a name of `FluxHandle.WS_OPTIONS`, None for the fixed grid).  The trajectory
    buffer has S rows; prepend_start: the start state goes in front of them (the fixed grid's and the adaptive solve's rows are the
    states after it) - False: the rows stand as the entry point wrote them (the stochastic sampler's S rows end with the sample, the
    multistep solve's begin with the start state)."""
    plan, cond, out, traj = _solve_begin(flux, x, kw, S, return_trajectory, pairs=cfg_scale is not None)
    with _on_capture_stream(flux.plan().stream) as s:
        try:
            h.set_step_cache(step_cache)           # None: off, whatever an earlier trajectory on this handle ran with
            h.set_cfg(cfg_scale)
            if buffers is not None:
                h.set_ws_option(buffers, True)
            for sl in plan.chunks:
                h.prepare(*plan.prepare_args(sl, max_evals), stream=s)
                xs = plan.img_rows(x, sl, x.dtype, copy=True)       # stepped in ITS dtype, in place: never the caller's
                tj = torch.empty(S, plan.size(sl), *x.shape[1:], dtype=x.dtype, device=plan.dev) if return_trajectory else None
                run(xs, plan.img_rows(cond, sl, torch.bfloat16), tj, s)
                if return_trajectory:
                    traj[:, sl] = torch.stack([plan.img_back(tj[i], sl) for i in range(S)])
                out[sl] = plan.img_back(xs, sl)
        finally:
            if buffers is not None:
                h.set_ws_option(buffers, False)    # a later fixed-grid trajectory sizes its workspace as it always did
            if cfg_scale is not None:
                h.set_cfg(None)                    # a later trajectory driven on this handle directly is a plain one again
    if traj is None:
        return out[None]
    return torch.cat((x.to(out.device)[None], traj), dim=0) if prepend_start else traj


def _unmonitored_handle(flux, why: str):
    """the C handle of a solve the monitor cannot log: never silently ignored (the entry points refuse it too)"""
    h = flux.handle()
    if flux.monitor_level(h):
        raise ValueError(f"monitor: {why}; set Flux.monitor = 0 or use a fixed-grid solver")
    return h


@torch.no_grad()
def _sample_multistep_fused(flux, x, kw, t, order, return_trajectory, cfg_scale=None):
    """vc_flux_sample_multistep per chunk of samples"""
    h = _unmonitored_handle(flux, "the multistep solve is not logged")
    t32 = t.to(torch.float32)

    def run(xs, cond, tj, s):
        h.sample_multistep(order, xs, cond, t32, x.dtype == torch.bfloat16, s, trajectory=tj)

    return _solve_on_handle(flux, h, x, kw, len(t), return_trajectory, len(t) - 1, run, cfg_scale=cfg_scale, buffers="multistep",
                            prepend_start=False)


@torch.no_grad()
def _sample_sde_fused(flux, x, kw, t, plan, setting, seed, offset, return_trajectory, cfg_scale=None):
    """vc_flux_sample_sde per chunk of samples; a chunk's draws follow the last chunk's in the stream"""
    h = _unmonitored_handle(flux, "the stochastic sampler is not logged")
    method, form, norm, last_step, lss = setting
    t32 = t.to(torch.float32)
    pos = [offset]

    def run(xs, cond, tj, s):
        h.sample_sde(method, xs, cond, t32, x.dtype == torch.bfloat16, s, form=form, norm=norm, last_step=last_step, last_step_size=lss,
                     seed=seed, offset=pos[0], trajectory=tj)
        pos[0] += plan["draws"] * xs.numel()

    return _solve_on_handle(flux, h, x, kw, len(t), return_trajectory, plan["evals"], run, cfg_scale=cfg_scale, buffers="sde",
                            prepend_start=False)


@torch.no_grad()
def _sample_adaptive_fused(flux, x, kw, t, return_trajectory, rtol, atol, max_attempts, cfg_scale=None, method="dopri5"):
    """vc_flux_sample_dopri5 (method "dopri5") or vc_flux_sample_rk per chunk of samples: ONE step size per chunk, so a sample's result
    depends on its chunk's other samples"""
    h = _unmonitored_handle(flux, "the adaptive solve has no evaluation index to log under")     # (its counter is a stage of an attempt)
    t32 = t.to(torch.float32)
    logs = []

    def run(xs, cond, tj, s):
        try:                                       # (the C ABI keeps one route to Dormand-Prince: its own entry point)
            solve = h.sample_dopri5 if method == "dopri5" else partial(h.sample_rk, method)
            solve(xs, cond, t32, x.dtype == torch.bfloat16, s, rtol, atol, max_attempts, trajectory=tj)
        finally:
            logs.append(h.dopri5_log())            # one log serves both entry points: the last adaptive solve's

    stages = len(RK_TABLEAUS[method]["c"])         # the modulation rows of one attempt
    return _solve_on_handle(flux, h, x, kw, len(t) - 1, return_trajectory, stages, run, cfg_scale=cfg_scale, buffers="adaptive"), logs


def _fusable(flux, x: torch.Tensor, method: str = "euler") -> bool:
    """The fused loop steps a bf16 state (the pipeline's, visualcloze.py:399) or - through the C handle - an f32 one IN f32
    (integrators.py:119 keeps the caller's state dtype).  Anything else (f16 / f64 states, an f32 state in the un-merged LoRA
    parity mode where its plan is ordered from Python, ref_plan="python") is stepped eagerly through Flux.forward with torch's own promotion rules:
    never a silent per-step rounding of the caller's state.  The Python-ordered plan (engine.py: use_handle False, or the
    un-merged LoRA parity mode lora_mode="ref" unless ref_plan="handle") knows the Euler update only: "midpoint" / "rk4" without the C handle are
    stepped eagerly too, one Flux.forward per stage through `_sample_foreign` - and so are the solves that are no fixed grid (method:
    `_route`'s family name "adaptive" / "sde" / "multistep"), through their own eager runners."""
    if method != "euler" and flux.handle() is None:
        return False
    if x.dtype == torch.bfloat16:
        return True
    return x.dtype == torch.float32 and flux.handle() is not None


def _cfg_fusable(flux, x: torch.Tensor, method: str, kw: dict) -> bool:
    """True CFG runs fused through the C handle alone, on pairs (j, j + B/2) that advance in one chunk: `MaskLayout` permutes image
    rows valid-first per sample, so the two samples of a pair must share their image mask for row i of one to be row i of the other
    (text masks may differ: a negative prompt of another length).  Anything else is stepped eagerly through forward_with_cfg."""
    if flux.handle() is None or not _fusable(flux, x, method):
        return False
    B = x.shape[0]
    if B % 2:
        return False              # forward_with_cfg raises for it
    tm, im = kw.get("txt_mask"), kw.get("img_mask")
    if tm is None or im is None:
        return True
    im = im.reshape(B, -1) != 0
    return bool(torch.equal(im[:B // 2], im[B // 2:]))


def cfg_chunks(B: int, max_batch: int) -> list:
    """The chunks of a true-CFG batch (samples [0, B/2) conditional, [B/2, B) unconditional) as lists of sample indices: whole pairs
    (j, j + B/2), as many as fit into `max_batch` samples, stacked conditional-first - cfg_chunks(6, 4) = [[0, 1, 3, 4], [2, 5]]."""
    if B % 2 or max_batch < 2:
        raise ValueError(f"true CFG needs an even batch and chunks of at least one pair, got B = {B}, max_batch = {max_batch}")
    half, ppc = B // 2, max_batch // 2
    return [list(range(p0, min(p0 + ppc, half))) + [j + half for j in range(p0, min(p0 + ppc, half))] for p0 in range(0, half, ppc)]


def _solver_t_as_state(t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """torchdiffeq hands the drift `t.to(y.dtype)` (`_PerturbFunc.forward`): with the bf16 state of
    visualcloze.py:399 the time a model sees is bf16(t_i), while dt = t_{i+1} - t_i comes from the f32 grid."""
    return t.to(x.dtype).to(torch.float32) if x.dtype.is_floating_point else t.to(torch.float32)


def model_times(t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The `timesteps` of the S = len(t) - 1 Flux evaluations (f32): 1 - t_i with t_i rounded to the state dtype
    (integrators.py:108-109 builds `ones(B) * t` in f32 from it; transport.py:384 forms 1 - t)."""
    t32 = t.to(torch.float32)
    return torch.ones(len(t) - 1) * (1 - _solver_t_as_state(t32[:-1], x))


def _sample_foreign(model, x, kw, t, return_trajectory, method="euler"):
    """Any other callable: the same grid and step rule (STEP_RULES), one host-driven call per evaluation.  Not through
    `_sample_eager`, on purpose: this is the reference's own stepping, the state in the CALLER's dtype under torch's promotion rules
    with 0-dim tensor times, where the other eager solves keep an f32 / f64 state and round once per output."""
    rule = STEP_RULES[method]
    f = _drift(model, None, kw, _times_as_state)      # the drift the reference builds (transport.py:193-198,384), ti a 0-dim f32 tensor
    t = t.to(x.device)       # as integrators.py:113: t0, t1 and dt are 0-dim tensors on the state's device
    states = [x]
    for i in range(len(t) - 1):
        x = rule(f, t[i], t[i + 1], t[i + 1] - t[i], x)
        if return_trajectory:
            states.append(x)
    return torch.stack(states) if return_trajectory else x[None]


@torch.no_grad()
def _sample_fused(flux, x, kw, t, return_trajectory, method="euler", step_cache=None, sampler=None, cfg_scale=None):
    """The whole trajectory of a chunk in ONE call on the C handle (vc_flux_sample_ode); without the handle the Python-ordered plan
    (`_sample_twin`).  cfg_scale: None = the drift is Flux.forward; a number = Flux.forward_with_cfg with it (C handle only)."""
    h = flux.handle()
    if h is None:
        if cfg_scale is not None:
            raise hip.VclozeHipError("true CFG in the fused loop needs the C handle")
        flux.monitor_level(h)                      # ValueError with the Python-ordered plan: never silently ignored
        return _sample_twin(flux, x, kw, t, return_trajectory)
    S = len(t) - 1
    n = S * hip.solver_evals(method)               # model evaluations: the workspace's tables hold all of them
    t32 = t.to(torch.float32)
    stats = []
    with flux.monitored(h) as monitored:
        def run(xs, cond, tj, s):
            with monitored(n, s):
                h.sample_ode(method, xs, cond, t32, x.dtype == torch.bfloat16, s, trajectory=tj)
            if step_cache is not None:
                stats.append(h.step_cache_stats(S))

        out = _solve_on_handle(flux, h, x, kw, S, return_trajectory, n, run, step_cache, cfg_scale)
    if step_cache is not None:
        flux.last_step_cache_stats = stats         # one dict per chunk of <= MAX_BATCH samples, in order
        if sampler is not None:
            sampler.last_step_cache_stats = stats
    return out


def _sample_twin(flux, x, kw, t, return_trajectory):
    """`_sample_fused` with the Python-ordered plan (engine.FluxEngine; bf16 states, Euler only: `_fusable`): a graph replay per step"""
    eng = flux.engine()
    S = len(t) - 1
    t32 = t.to(torch.float32)
    eval_t = model_times(t32, x)                   # Flux sees 1 - t (transport.py:384), t in the state's dtype
    dts = (t32[1:] - t32[:-1]).contiguous()        # torchdiffeq fixed grid: dt = t1 - t0
    plan, cond, out, traj = _solve_begin(flux, x, kw, S, return_trajectory)
    N, C = x.shape[1:]
    with _on_capture_stream(eng.stream) as s:
        for sl in plan.chunks:                     # a chunk of samples advances together
            bs = plan.size(sl)
            ws = eng.workspace(plan.T, N, S, bs)
            args, kwargs = plan.twin_prepare_args(sl, eval_t)
            eng.prepare_sample(ws, *args, s=s, **kwargs)
            ws.DTS.copy_(dts, non_blocking=True)
            ws.STEP.zero_()
            ws.XS.copy_(plan.img_rows(x, sl, torch.bfloat16).reshape(bs * N, C))     # the state stays in kernel row order for all steps
            ws.COND.copy_(plan.img_rows(cond, sl, torch.bfloat16).reshape(bs * N, -1))
            graph = eng.step_graph(ws, s)
            states = []
            for _ in range(S):
                graph.launch(s)                    # one Flux evaluation + Euler update + step counter increment
                if return_trajectory:
                    states.append(plan.img_back(ws.XS.reshape(bs, N, C), sl).clone())
            if return_trajectory:
                traj[:, sl] = torch.stack(states)  # [S, bs, N, C]
            out[sl].copy_(plan.img_back(ws.XS.reshape(bs, N, C), sl))
    return out[None] if traj is None else torch.cat((x.to(out.device)[None], traj), dim=0)
