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

The step rules (`STEP_RULES`) are torchdiffeq 0.2.x's fixed-grid solvers as recalled - unpinned against real
torchdiffeq, which was not available to check against (as the Euler rule, tests/golden/make_golden.py).  They
are written ONCE, as the literal torch expressions: a correction is a one-line change here and in
csrc/elementwise.hip (ode_update).
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch

from . import hip


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


class Transport:
    def __init__(self, path_type: str, prediction: str, do_shift: bool):
        self.path_type, self.prediction, self.do_shift = path_type, prediction, do_shift
        self.train_eps = self.sample_eps = 0  # velocity & Linear is stable everywhere (transport/__init__.py:46-48)

    def check_interval(self, reverse: bool = False):
        t0, t1 = 0, 1  # transport.py:70-96 for Linear + velocity, sde=False
        if reverse:
            t0, t1 = 1 - t0, 1 - t1
        return t0, t1


def create_transport(path_type="Linear", prediction="velocity", loss_weight=None, train_eps=None, sample_eps=None,
                     snr_type="uniform", loss_type="mse", do_shift=True) -> Transport:
    if path_type != "Linear" or prediction != "velocity":
        raise NotImplementedError("the MI355X denoising path implements Linear path + velocity prediction only")
    return Transport(path_type, prediction, do_shift)


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


class Sampler:
    def __init__(self, transport: Transport):
        self.transport = transport
        self.last_step_cache_stats = None      # of the last cached trajectory this sampler ran: one dict per chunk of samples

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
        t0, t1 = self.transport.check_interval(reverse=reverse)
        if strength is not None:
            t0 = (t1 - t0) * strength + t0
        assert t0 < t1, "ODE sampler has to be in forward time"

        def _sample(x: torch.Tensor, model: Callable, model_kwargs: dict) -> torch.Tensor:
            t = solver_time_grid(num_steps, x.shape[1], t0, t1, do_shift, time_shifting_factor)
            from .model import Flux
            owner = getattr(model, "__self__", None)
            if isinstance(owner, Flux) and getattr(model, "__name__", "") == "forward_with_cfg":
                if step_cache is not None:
                    raise ValueError("step_cache works with Flux.forward only, not with forward_with_cfg (true CFG)")
                kw = dict(model_kwargs)
                cfg_scale = float(kw.pop("cfg_scale", 1.0))
                if _cfg_fusable(owner, x, sampling_method, kw):
                    return _sample_fused(owner, x, kw, t, return_trajectory, sampling_method, None, self, cfg_scale=cfg_scale)
                # stepped eagerly (unequal image masks within a pair, no C handle, an f16 / f64 state): the same bf16 velocity
                fwd = lambda xin, **k: owner.forward_with_cfg(xin, cfg_scale=cfg_scale, **k).to(torch.bfloat16)  # noqa: E731
                return _sample_foreign(fwd, x, kw, t, return_trajectory, sampling_method)
            if isinstance(owner, Flux) and getattr(model, "__name__", "") == "forward":
                if step_cache is not None:      # never silently ignored: only the C handle's loop implements it
                    if owner.handle() is None:
                        raise ValueError("step_cache needs the C handle: not available with lora_mode='ref' (unless ref_plan='handle') "
                                         "or the Python-ordered plan (use_handle False)")
                    if not _fusable(owner, x, sampling_method):
                        raise ValueError(f"step_cache: a {x.dtype} state is stepped eagerly, where no cache exists")
                if _fusable(owner, x, sampling_method):
                    return _sample_fused(owner, x, dict(model_kwargs), t, return_trajectory, sampling_method, step_cache, self)
                # stepped eagerly; the velocity of this model is a bf16 tensor as the reference's is under autocast
                # (visualcloze.py:363) whatever dtype Flux.forward hands back to its caller: dt * f stays a bf16 product
                fwd = model
                model = lambda xin, **k: fwd(xin, **k).to(torch.bfloat16)  # noqa: E731
            elif step_cache is not None:
                raise ValueError("step_cache: only the fused loop of a visualcloze_amd.Flux implements it, not a foreign callable")
            return _sample_foreign(model, x, dict(model_kwargs), t, return_trajectory, sampling_method)

        return _sample


def _fusable(flux, x: torch.Tensor, method: str = "euler") -> bool:
    """The fused loop steps a bf16 state (the pipeline's, visualcloze.py:399) or - through the C handle - an f32 one IN f32
    (integrators.py:119 keeps the caller's state dtype).  Anything else (f16 / f64 states, an f32 state in the un-merged LoRA
    parity mode where its plan is ordered from Python, ref_plan="python") is stepped eagerly through Flux.forward with torch's own promotion rules:
    never a silent per-step rounding of the caller's state.  The Python-ordered plan (engine.py: use_handle False, or the
    un-merged LoRA parity mode lora_mode="ref" unless ref_plan="handle") knows the Euler update only: "midpoint" / "rk4" without the C handle are
    stepped eagerly too, one Flux.forward per stage through `_sample_foreign`."""
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
    """Any other callable: the same grid and step rule (STEP_RULES), one host-driven call per evaluation."""
    cond = kw.pop("cond", None)
    rule = STEP_RULES[method]

    def f(ti, y):            # the drift the reference builds (transport.py:193-198,384), ti a 0-dim f32 tensor
        tt = torch.ones(y.size(0), device=y.device) * _solver_t_as_state(ti, y)
        xin = torch.cat((y, cond), dim=-1) if cond is not None else y
        v = model(xin, timesteps=torch.ones_like(tt) * (1 - tt), **kw)
        assert v.shape == y.shape, "Output shape from ODE solver must match input shape"
        return -v

    t = t.to(x.device)       # as integrators.py:113: t0, t1 and dt are 0-dim tensors on the state's device
    states = [x]
    for i in range(len(t) - 1):
        x = rule(f, t[i], t[i + 1], t[i + 1] - t[i], x)
        if return_trajectory:
            states.append(x)
    return torch.stack(states) if return_trajectory else x[None]


@torch.no_grad()
def _sample_fused(flux, x, kw, t, return_trajectory, method="euler", step_cache=None, sampler=None, cfg_scale=None):
    """cfg_scale: None = the drift is Flux.forward; a number = Flux.forward_with_cfg with it (C handle only).  Samples then advance
    in chunks of whole pairs (j, j + B/2), conditional samples first, and go back in the caller's order."""
    eng = flux.engine()
    dev = eng.dev
    B, N, C = x.shape
    cond = kw.get("cond")
    if cond is None:
        raise hip.VclozeHipError("fused sampler expects model_kwargs['cond'] (x || cond feeds img_in)")
    if C + cond.shape[-1] != flux.in_channels:
        raise hip.VclozeHipError(f"x ({C}) || cond ({cond.shape[-1]}) does not match in_channels {flux.in_channels}")
    txt, y, guidance = kw["txt"], kw["y"], kw.get("guidance")
    if flux.params.guidance_embed and guidance is None:
        raise ValueError("Didn't get guidance strength for guidance distilled model.")
    T = txt.shape[1]
    S = len(t) - 1
    E = hip.solver_evals(method)                   # model evaluations per step: the workspace's tables hold S * E of them
    t32 = t.to(torch.float32)
    eval_t = model_times(t32, x)                   # Flux sees 1 - t (transport.py:384), t in the state's dtype
    dts = (t32[1:] - t32[:-1]).contiguous()        # torchdiffeq fixed grid: dt = t1 - t0
    bf = lambda a: a.to(dev, torch.bfloat16).contiguous()  # noqa: E731
    sdt = x.dtype                                  # bf16, or f32 (handle path only): the state is stepped in ITS dtype
    out = torch.empty(B, N, C, dtype=sdt, device=dev)
    traj = torch.empty(S, B, N, C, dtype=sdt, device=dev) if return_trajectory else None
    gbf16 = guidance is not None and guidance.dtype == torch.bfloat16
    from .model import MaskLayout, per_sample
    guidance = per_sample(guidance, B)
    lay = MaskLayout(kw.get("txt_mask"), kw.get("img_mask"), B, T, N)
    st = eng.stream
    st.wait_stream(torch.cuda.current_stream())
    # the C handle runs the whole trajectory of a chunk in ONE call (vc_flux_sample_ode); the un-merged LoRA mode uses the
    # Python-ordered plan (bf16 states, Euler only: _fusable) unless ref_plan is "handle"
    h = flux.handle()
    if h is not None:
        h.set_step_cache(step_cache)               # None: off, whatever an earlier trajectory on this handle ran with
        h.set_cfg(cfg_scale)
    elif cfg_scale is not None:
        raise hip.VclozeHipError("true CFG in the fused loop needs the C handle")
    mb = flux.max_batch()
    if cfg_scale is None:
        chunks = [slice(b0, min(b0 + mb, B)) for b0 in range(0, B, mb)]
    else:
        chunks = cfg_chunks(B, mb)
    stats = []
    with torch.cuda.stream(st):
        s = st.cuda_stream
        for sl in chunks:                            # a chunk of samples advances together, one graph replay per step
            bs = len(range(B)[sl]) if isinstance(sl, slice) else len(sl)
            if h is not None:
                h.prepare(bf(lay.txt_rows(txt, sl)), bf(y[sl]), None if guidance is None else guidance[sl], gbf16,
                          lay.img_rows(kw["img_ids"], sl), lay.txt_rows(kw["txt_ids"], sl), S * E, lay.kv_len(sl), lay.kv_gap(sl), stream=s)
                xs = lay.img_rows(x, sl).to(dev, sdt, copy=True).contiguous()   # updated in place: never the caller's
                tj = torch.empty(S, bs, N, C, dtype=sdt, device=dev) if return_trajectory else None
                h.sample_ode(method, xs, bf(lay.img_rows(cond, sl)), t32, x.dtype == torch.bfloat16, s, trajectory=tj)
                if step_cache is not None:
                    stats.append(h.step_cache_stats(S))
                if return_trajectory:
                    traj[:, sl] = torch.stack([lay.img_rows_back(tj[i], sl) for i in range(S)])
                out[sl] = lay.img_rows_back(xs, sl)
                continue
            ws = eng.workspace(T, N, S, bs)
            eng.prepare_sample(ws, bf(lay.txt_rows(txt, sl)), bf(y[sl]), None if guidance is None else guidance[sl], gbf16,
                               lay.img_rows(kw["img_ids"], sl), lay.txt_rows(kw["txt_ids"], sl), eval_t, lay.kv_len(sl), s=s,
                               kv_gap=lay.kv_gap(sl))
            ws.DTS.copy_(dts, non_blocking=True)
            ws.STEP.zero_()
            ws.XS.copy_(bf(lay.img_rows(x, sl)).reshape(bs * N, C))     # the state stays in kernel row order for all steps
            ws.COND.copy_(bf(lay.img_rows(cond, sl)).reshape(bs * N, -1))
            graph = eng.step_graph(ws, s)
            states = []
            for _ in range(S):
                graph.launch(s)          # one Flux evaluation + Euler update + step counter increment
                if return_trajectory:
                    states.append(lay.img_rows_back(ws.XS.reshape(bs, N, C), sl).clone())
            if return_trajectory:
                traj[:, sl] = torch.stack(states)                 # [S, bs, N, C]
            out[sl].copy_(lay.img_rows_back(ws.XS.reshape(bs, N, C), sl))
        if cfg_scale is not None:
            h.set_cfg(None)                        # a later trajectory driven on this handle directly is a plain one again
    torch.cuda.current_stream().wait_stream(st)
    if step_cache is not None:
        flux.last_step_cache_stats = stats         # one dict per chunk of <= MAX_BATCH samples, in order
        if sampler is not None:
            sampler.last_step_cache_stats = stats
    if return_trajectory:
        return torch.cat((x.to(dev)[None], traj), dim=0)
    return out[None]
