"""`VisualClozeModel.process_images` / `.upsampling` (visualcloze.py:147-245, 363-434) on the MI355X path.

    rows = denoise_grid(model, noise_rows, cond_latent_rows, mask_rows, txt, vec, cfg=30, steps=30)       # latent space
    up   = sdedit_upsample(model, noise, latent, blank_latent, txt, vec, cfg=30, steps=10, strength=0.4)  # latent space
    imgs = generate_grid(model, ae, t5, clip, row_images, row_masks, t5_ids, clip_ids, seed, ...)         # pixels in/out
    outs = generate_and_upsample(model, ae, t5, clip, ..., grid_w, mask_position, upsampling_size, ...)   # both stages chained

`generate_grid` chains the whole tensor path of `process_images` (visualcloze.py:363-434): VAE-encode the grid rows,
pack latents + fill masks into `cond`, draw the per-row noise, encode the prompt with T5 / CLIP, run the fused sampler,
unpack, VAE-decode and map to [0, 1].  Image decoding, prefix stripping and tokenisation are host work and stay with the caller:
inputs are row tensors in [-1, 1] and token ids.  `preprocess_grid` makes the row tensors from photographs - with PIL as the
reference does, or with `device_resize=True` on the device (the library's resampler gives Pillow's bytes) - and the
`device_resize` switch of the upsampling functions does the same for the resize between the stages.
"""
from __future__ import annotations

import weakref
from typing import List, Optional, Sequence, Union

import torch

from . import hip, packing
from .transport import Sampler, create_transport


class NoiseStream:
    """The counterpart of `torch.Generator` over the library's own noise source (`hip.randn`, vc_randn of include/vcloze_hip.h:
    Philox4x32-10 + Box-Muller, every element a function of (seed, stream position) only).  `randn` draws at the current
    `offset` and advances it by the number of elements drawn, so a sequence of draws is one contiguous stretch of the stream: a
    caller without torch reproduces every tensor from (seed, offset) with vc_randn / vc_randn_tokens.  Its values differ from
    torch's: the images of a seed here are not the images `torch.Generator.manual_seed` gives for the same seed -
    `TorchNoiseStream` below is the stream that gives those.  Pass one as `rng` to `generate_grid`, `upsample_image(s)` or
    `generate_and_upsample`; the default noise stays torch's."""

    def __init__(self, seed: int, offset: int = 0, device=None):
        self.seed = int(seed)
        self.device = device
        self.offset = offset

    @property
    def offset(self) -> int:
        """the stream position of the next draw (readable and settable)"""
        return self._offset

    @offset.setter
    def offset(self, value: int) -> None:
        value = int(value)
        if not 0 <= value < 1 << 64:
            raise ValueError(f"NoiseStream.offset = {value}: an unsigned 64-bit stream position expected")
        self._offset = value

    def randn(self, shape, dtype=torch.bfloat16, device=None) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        if n < 1 or self._offset + n > 1 << 64:
            raise ValueError(f"NoiseStream.randn: {n} elements at offset {self._offset} leave the 64-bit stream")
        out = hip.randn(tuple(shape), self.seed, self._offset, dtype=dtype, device=device if device is not None else self.device)
        self._offset += n
        return out


class TorchNoiseStream(NoiseStream):
    """`NoiseStream`'s interface over torch's device generator stream, restated by the library (`hip.randn_torch`, vc_randn_torch of
    include/vcloze_hip.h, THE TORCH STREAM): the k-th `randn(shape, dtype)` is bit for bit the k-th
    `torch.randn(shape, device=dev, generator=G).to(dtype)` of `G = torch.Generator(dev).manual_seed(seed)`, and `offset` is
    `G.get_offset()` after every draw (the Philox offset, a multiple of 4 - not an element count).  Accepted wherever `rng` takes a
    `NoiseStream` - `use_grid_handle=True` included - except by the stochastic sampler, whose in-kernel draws are the library's own
    stream.  With it a seed gives the images the default path (`seed=`) and the reference give, now also from the C entry points.
    `sm_count` / `threads_per_sm`: another device's properties (draws above 256 * sm_count * (threads_per_sm / 256) elements depend
    on them); 0 = the current device's.  Parity is with the torch build this package is tested against."""

    def __init__(self, seed: int, device=None, sm_count: int = 0, threads_per_sm: int = 0, offset: int = 0):
        self.sm_count, self.threads_per_sm = int(sm_count), int(threads_per_sm)
        super().__init__(seed, offset, device)

    @property
    def offset(self) -> int:
        """the generator's Philox offset before the next draw (readable and settable; a multiple of 4)"""
        return self._offset

    @offset.setter
    def offset(self, value: int) -> None:
        value = int(value)
        if not 0 <= value < 1 << 64 or value % 4:
            raise ValueError(f"TorchNoiseStream.offset = {value}: an unsigned 64-bit multiple of 4 expected (torch.Generator.get_offset())")
        self._offset = value

    def randn(self, shape, dtype=torch.bfloat16, device=None) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        if n < 1:
            raise ValueError(f"TorchNoiseStream.randn: {n} elements")
        advance = hip.torch_randn_policy(n, self.sm_count, self.threads_per_sm)[1]
        if self._offset + advance >= 1 << 64:
            raise ValueError(f"TorchNoiseStream.randn: {n} elements at offset {self._offset} leave the 64-bit Philox offset")
        out = hip.randn_torch(tuple(shape), self.seed, self._offset, dtype=dtype, device=device if device is not None else self.device,
                              sm_count=self.sm_count, threads_per_sm=self.threads_per_sm)
        self._offset += advance
        return out


def _no_torch_stream(rng, what: str) -> None:
    if isinstance(rng, TorchNoiseStream):
        raise ValueError(f"{what}: the stochastic sampler draws its noise inside the step from the library's own stream (vc_sde_stage), "
                         "which a TorchNoiseStream does not restate: pass rng=NoiseStream(seed)")


def _draw(rng, shape, dev) -> torch.Tensor:
    """one bf16 noise tensor from `rng`: a NoiseStream, or a torch.Generator as the reference draws (f32, then .to(bf16))"""
    if isinstance(rng, NoiseStream):
        return rng.randn(shape, torch.bfloat16, device=dev)
    return torch.randn(shape, device=dev, generator=rng).to(torch.bfloat16)


def _encode(ae, px, noise, rng) -> torch.Tensor:
    """ae.encode of [1, 3, H, W]; with a NoiseStream and no `noise` given, the DiagonalGaussian draw (autoencoder.py:272) comes
    from the stream too, where the reference's `.sample()` makes it"""
    if noise is None and isinstance(rng, NoiseStream):
        f = 2 ** (ae.encoder.num_resolutions - 1)
        noise = rng.randn([1, ae.encoder.z_channels, px.shape[-2] // f, px.shape[-1] // f], torch.bfloat16, device=px.device)
    return ae.encode(px, noise=noise)


_GRID_HANDLES = weakref.WeakKeyDictionary()        # model -> (the four sub-handles' identities, GridHandle)


def _grid_handle(model, ae, t5, clip, rng, what: str, **unsupported):
    """the `handle.GridHandle` over the four modules' C handles for `use_grid_handle=True`, kept per model while those handles
    live.  The switch is never silently ignored: it needs the library's noise stream and all three `use_handle` switches on."""
    if not isinstance(rng, NoiseStream):
        raise ValueError(f"{what}(use_grid_handle=True) draws from the library's stream: pass rng=NoiseStream(seed)")
    for name, v in unsupported.items():
        if v is not None:
            raise ValueError(f"{what}(use_grid_handle=True) draws every noise tensor itself: {name} must be None")
    if getattr(model, "monitor", 0):
        raise ValueError(f"{what}(use_grid_handle=True) drives its own trajectory, which the numerics monitor does not log: set "
                         "model.monitor = 0 or use_grid_handle=False")
    if not (getattr(model, "use_handle", False) and model.handle() is not None and getattr(ae, "use_handle", False)
            and t5._handle_serves() and clip._handle_serves()):
        raise ValueError(f"{what}(use_grid_handle=True) needs the C handles of all four modules: model.use_handle, ae.use_handle, "
                         "t5.use_handle and clip.use_handle True (bf16 text encoders; with lora_mode 'ref': ref_plan 'handle')")
    from .handle import GridHandle
    key = tuple(id(h) for h in (model.handle(), ae.handle(), t5.handle(), clip.handle()))
    c = _GRID_HANDLES.get(model)
    if c is None or c[0] != key:
        c = (key, GridHandle(model, ae, t5, clip))
        _GRID_HANDLES[model] = c
    if isinstance(rng, TorchNoiseStream):
        c[1].set_noise("torch", rng.sm_count, rng.threads_per_sm)
    else:
        c[1].set_noise("own")
    return c[1]


def _kwargs(inp_ids, inp_mask, txt, vec, cond, cfg, dev):
    B, T = txt.shape[0], txt.shape[1]
    return dict(txt=txt, txt_ids=torch.zeros(B, T, 3, device=dev), txt_mask=torch.ones(B, T, dtype=torch.int32, device=dev),
                y=vec, img_ids=inp_ids, img_mask=inp_mask, cond=cond,
                guidance=torch.full((B,), cfg, device=dev, dtype=torch.bfloat16))   # visualcloze.py:413


@torch.no_grad()
def denoise_grid(model, noise_rows: List[torch.Tensor], cond_latent_rows: List[torch.Tensor],
                 mask_rows: List[torch.Tensor], txt: torch.Tensor, vec: torch.Tensor, cfg: float = 30.0,
                 steps: int = 30, solver: str = "euler", time_shifting_factor=1, step_cache=None,
                 adaptive: Optional[dict] = None, sde: Optional[dict] = None, rng=None,
                 multistep: Optional[dict] = None) -> List[torch.Tensor]:
    """One grid: per-row noise [1,16,h,w], VAE latents of the grid rows (already shifted/scaled), per-row PIXEL
    fill masks [1,1,8h,8w]; txt [1,T,4096], vec [1,768].  Returns the denoised row latents [1,16,h,w].
    `adaptive`: None, or dict(rtol=, atol=[, max_attempts=][, method=]) - the error-controlled solve (`Sampler.sample_ode_adaptive`:
    Dormand-Prince 5(4), or with method="bosh3" / "adaptive_heun" a cheaper embedded pair) instead of `solver`; `steps` then only places the end time's grid.
    `sde`: None, or dict(sampling_method=, diffusion_form=, diffusion_norm=, last_step=, last_step_size=, sample_eps=) - any subset -
    the stochastic sampler (`Sampler.sample_sde`, num_steps = `steps`) instead of `solver`; its noise comes from `rng`, which must be a
    `NoiseStream` (its offset advances by the draws).  Image quality under any diffusion form is unmeasured.
    `multistep`: None, or dict(order=) - the Adams-Bashforth multistep solve (`Sampler.sample_ode_multistep`, num_steps = `steps`, one
    evaluation per step) instead of `solver`.  Image quality at any order is unmeasured."""
    dev = noise_rows[0].device
    img, img_ids, img_mask = packing.prepare_grid([noise_rows])                       # visualcloze.py:403
    cond = packing.pack_cond(cond_latent_rows, mask_rows)                              # :381-389
    sampler = Sampler(create_transport("Linear", "velocity", do_shift=True))
    if multistep is not None:
        if adaptive is not None or sde is not None or step_cache is not None:
            raise ValueError("multistep: the multistep solve works neither with adaptive=, nor with sde=, nor with the step cache")
        fn = sampler.sample_ode_multistep(num_steps=steps, do_shift=True, time_shifting_factor=time_shifting_factor, **multistep)
        samples = fn(img, model.forward, _kwargs(img_ids, img_mask, txt, vec, cond, cfg, dev))[-1][:1]
        return packing.unpack_rows(samples, [tuple(r.shape[-2:]) for r in noise_rows])
    if sde is not None:
        if adaptive is not None or step_cache is not None:
            raise ValueError("sde: the stochastic sampler works neither with adaptive= nor with the step cache")
        if not isinstance(rng, NoiseStream):
            raise ValueError("sde: the stochastic sampler draws from the library's stream: pass rng=NoiseStream(seed)")
        _no_torch_stream(rng, "sde")
        fn = sampler.sample_sde(num_steps=steps, rng=rng, **sde)
        samples = fn(img, model.forward, **_kwargs(img_ids, img_mask, txt, vec, cond, cfg, dev))[-1][:1]
        return packing.unpack_rows(samples, [tuple(r.shape[-2:]) for r in noise_rows])
    if adaptive is not None:
        if step_cache is not None:
            raise ValueError("adaptive: the step cache works with the fixed-grid Euler loop only")
        fn = sampler.sample_ode_adaptive(num_steps=steps, do_shift=True, time_shifting_factor=time_shifting_factor, **adaptive)
        model.last_adaptive_log = None
        samples = fn(img, model.forward, _kwargs(img_ids, img_mask, txt, vec, cond, cfg, dev))[-1][:1]
        model.last_adaptive_log = sampler.last_adaptive_log
        return packing.unpack_rows(samples, [tuple(r.shape[-2:]) for r in noise_rows])
    fn = sampler.sample_ode(
        sampling_method=solver, num_steps=steps, atol=1e-6, rtol=1e-3, reverse=False, do_shift=True,
        time_shifting_factor=time_shifting_factor, step_cache=step_cache)              # :284-292
    samples = fn(img, model.forward, _kwargs(img_ids, img_mask, txt, vec, cond, cfg, dev))[-1][:1]   # :415-420
    return packing.unpack_rows(samples, [tuple(r.shape[-2:]) for r in noise_rows])     # :425-429


@torch.no_grad()
def sdedit_upsample(model, noise: torch.Tensor, latent: torch.Tensor, blank_latent: torch.Tensor, txt: torch.Tensor,
                    vec: torch.Tensor, cfg: float = 30.0, steps: int = 10, strength: float = 0.4,
                    solver: str = "euler", step_cache=None) -> torch.Tensor:
    """SDEdit refinement of one image (visualcloze.py:184-237): start from noise*(1-s) + latent*s, everything masked,
    un-shifted grid from t0 = strength.  noise/latent/blank_latent: [1,16,h,w]; returns [1,16,h,w]."""
    dev = latent.device
    h, w = latent.shape[-2:]
    img, img_ids, img_mask = packing.prepare_grid([[noise]])
    lat_tok, _, _ = packing.prepare_grid([[latent]])
    x0 = hip.sdedit_mix(img, lat_tok, strength)                                        # :221
    ones = torch.ones(1, 1, 8 * h, 8 * w, dtype=torch.bfloat16, device=dev)            # mask = 1 everywhere, :198
    cond = packing.pack_cond([blank_latent], [ones])                                   # :214
    fn = Sampler(create_transport("Linear", "velocity", do_shift=True)).sample_ode(
        sampling_method=solver, num_steps=steps, atol=1e-6, rtol=1e-3, reverse=False, do_shift=False,
        time_shifting_factor=1.0, strength=strength, step_cache=step_cache)            # :184-193
    sample = fn(x0, model.forward, _kwargs(img_ids, img_mask, txt, vec, cond, cfg, dev))[-1][:1]
    return packing.unpack_rows(sample, [(h, w)])[0]


@torch.no_grad()
def sdedit_upsample_batch(model, noises: Sequence[torch.Tensor], latents: Sequence[torch.Tensor],
                          blank_latents: Sequence[torch.Tensor], txt: torch.Tensor, vec: torch.Tensor, cfg: float = 30.0,
                          steps: int = 10, strength: float = 0.4, solver: str = "euler", step_cache=None) -> List[torch.Tensor]:
    """`sdedit_upsample` for K targets of ONE size and prompt advanced TOGETHER: the reference refines the masked cells of a
    grid one after the other (visualcloze.py:450-465), each an independent ODE solve over the same (T, N), so they stack into
    a per-GPU batch - one graph replay per solver step moves all of them (chunks of <= 4) and the GEMMs see M = K * L rows:
    at L = 4608 that is +14 % (K = 2) / +17 % (K = 4) evaluations per second over one target at a time
    (profiles/r04a_per_gpu_batch_probe.json).  Per target the result equals the one-at-a-time call up to the bf16 noise of
    another GEMM tile plan (tests/test_model_gpu.py).  txt [1,T,4096] / vec [1,768]: the shared content prompt."""
    K = len(noises)
    if K == 0:
        return []
    dev = latents[0].device
    h, w = latents[0].shape[-2:]
    if any(t.shape[-2:] != (h, w) for t in list(noises) + list(latents) + list(blank_latents)):
        raise ValueError("sdedit_upsample_batch: all targets must share one latent size")
    img, img_ids, img_mask = packing.prepare_grid([[n] for n in noises])
    lat_tok, _, _ = packing.prepare_grid([[l] for l in latents])
    x0 = hip.sdedit_mix(img, lat_tok, strength)                                        # :221, all targets at once
    ones = torch.ones(1, 1, 8 * h, 8 * w, dtype=torch.bfloat16, device=dev)
    cond = torch.cat([packing.pack_cond([b], [ones]) for b in blank_latents], dim=0)
    fn = Sampler(create_transport("Linear", "velocity", do_shift=True)).sample_ode(
        sampling_method=solver, num_steps=steps, atol=1e-6, rtol=1e-3, reverse=False, do_shift=False,
        time_shifting_factor=1.0, strength=strength, step_cache=step_cache)
    kw = _kwargs(img_ids, img_mask, txt.expand(K, -1, -1), vec.expand(K, -1), cond, cfg, dev)
    sample = fn(x0, model.forward, kw)[-1]
    return [packing.unpack_rows(sample[k:k + 1], [(h, w)])[0] for k in range(K)]


@torch.no_grad()
def generate_grid(model, ae, t5, clip, row_images: List[torch.Tensor], row_masks: List[torch.Tensor],
                  t5_ids: torch.Tensor, clip_ids: torch.Tensor, seed: int, cfg: float = 30.0, steps: int = 30,
                  encode_noise: Optional[List[torch.Tensor]] = None, decode_rows: Optional[Sequence[int]] = None,
                  solver: str = "euler", time_shifting_factor=1, rng: Union[torch.Generator, NoiseStream, None] = None,
                  step_cache=None, use_grid_handle: bool = False, adaptive: Optional[dict] = None,
                  monitor: Optional[int] = None, sde: Optional[dict] = None, multistep: Optional[dict] = None) -> List[torch.Tensor]:
    """One grid, pixels in, pixels out (visualcloze.py:363-434).

    row_images[i]: [3, H, W_row] in [-1, 1] (the images of grid row i side by side); row_masks[i]: [1, 1, H, W_row]
    pixel fill mask (1 = generate); t5_ids [1, 512], clip_ids [1, 77]; `seed` drives the initial noise exactly like
    `torch.Generator(device).manual_seed(seed)` + one `torch.randn` per row (:394-399).  `encode_noise` are the VAE's
    DiagonalGaussian samples per row (None: drawn with torch.randn_like, as the reference's encode does).
    `rng`: the generator to draw from instead of a fresh one seeded with `seed` (the upsampling stage keeps drawing from
    the SAME generator, :450-458), or a `NoiseStream`: every draw then comes from the library's own stream in the reference's
    order of draws - the DiagonalGaussian draw of each row's encode (:377; unless `encode_noise` gives it), then one start-noise
    tensor per row (:395-399) - each a contiguous stretch of the stream.  A `TorchNoiseStream` is taken the same way and draws
    torch's own stream: with `encode_noise` given, `rng=TorchNoiseStream(seed)` is bit for bit what `seed` alone gives.  Returns the decoded rows `decode_rows` (default: all) as
    [3, H, W_row] tensors in [0, 1] (:430-432).  `step_cache`: a `transport.StepCache` or None (off, the default) - the opt-in first-block step cache of
    the Euler loop; it changes results; the stats of the last cached trajectory are `model.last_step_cache_stats`.
    `use_grid_handle`: opt-in, off by default - the whole function as ONE call of the library's grid handle (vc_grid_generate,
    `handle.GridHandle`: the same composition kept in csrc/grid_engine.hip, the same bits).  Valid only with a `NoiseStream` and the
    use_handle switches of all four modules on (ValueError otherwise); `rng.offset` advances as it does here.
    `adaptive`: None (the default), or dict(rtol=, atol=[, method="dopri5" | "bosh3" | "adaptive_heun"]) - denoise with the
    error-controlled solve (Dormand-Prince 5(4) unless `method` names a cheaper embedded pair) instead of
    `solver` (`denoise_grid`); `model.last_adaptive_log` tells what it did.  Refused together with use_grid_handle=True: the grid
    handle runs the fixed-grid solvers only.
    `monitor`: None (the default: `model.monitor` as it stands), or 0 | 1 | 2 - the numerics monitor of the Flux handle for this call
    (`Flux.monitor`): `model.last_monitor_log` / `model.last_monitor_report` tell what the solve's evaluations held, and with
    `model.monitor_strict` a NaN / inf raises FloatingPointError.  Refused together with use_grid_handle=True, `adaptive` and `sde`.
    `sde`: None (the default), or a dict of `Sampler.sample_sde` settings - denoise with the stochastic sampler instead of `solver`
    (`denoise_grid`); needs `rng` to be a `NoiseStream`, from which the sampler's draws follow the start noise.  Refused together with
    use_grid_handle=True: the grid handle runs the fixed-grid solvers only.
    `multistep`: None (the default), or dict(order=) - denoise with the Adams-Bashforth multistep solve of that order (1..4, one
    evaluation per step) instead of `solver` (`denoise_grid`, `Sampler.sample_ode_multistep`).  Refused together with
    use_grid_handle=True, `adaptive`, `sde`, `step_cache` and a `monitor` level above 0."""
    if multistep is not None:
        if use_grid_handle:
            raise ValueError("generate_grid(multistep=...) does not work with use_grid_handle=True: the grid handle runs the fixed-grid "
                             "solvers only")
        if adaptive is not None:
            raise ValueError("generate_grid(multistep=...) does not work with adaptive=: one solver per call")
        if sde is not None:
            raise ValueError("generate_grid(multistep=...) does not work with sde=: one solver per call")
        if step_cache is not None:
            raise ValueError("generate_grid(multistep=...) does not work with step_cache=: the step cache works with the fixed-grid Euler "
                             "loop only")
        if monitor:
            raise ValueError("generate_grid(multistep=...) does not work with monitor=: the multistep solve is not logged")
    if sde is not None:
        if use_grid_handle:
            raise ValueError("generate_grid(sde=...) does not work with use_grid_handle=True: the grid handle runs the fixed-grid solvers only")
        if not isinstance(rng, NoiseStream):
            raise ValueError("generate_grid(sde=...) draws from the library's stream: pass rng=NoiseStream(seed)")
        _no_torch_stream(rng, "generate_grid(sde=...)")
    if monitor is not None:
        if monitor and (use_grid_handle or adaptive is not None or sde is not None):
            raise ValueError("generate_grid(monitor=...) works with the fixed-grid solvers of the Flux handle, not with use_grid_handle=True "
                             "(the grid handle drives its own trajectory), adaptive= or sde=")
        before = model.monitor
        model.monitor = monitor
        try:
            return generate_grid(model, ae, t5, clip, row_images, row_masks, t5_ids, clip_ids, seed, cfg=cfg, steps=steps,
                                 encode_noise=encode_noise, decode_rows=decode_rows, solver=solver, time_shifting_factor=time_shifting_factor,
                                 rng=rng, step_cache=step_cache, use_grid_handle=use_grid_handle, adaptive=adaptive, sde=sde,
                                 multistep=multistep)
        finally:
            model.monitor = before
    if adaptive is not None and use_grid_handle:
        raise ValueError("generate_grid(adaptive=...) does not work with use_grid_handle=True: the grid handle runs the fixed-grid solvers only")
    if use_grid_handle:
        gh = _grid_handle(model, ae, t5, clip, rng, "generate_grid", encode_noise=encode_noise)
        if step_cache is not None and solver != "euler":
            raise ValueError(f"step_cache works with sampling_method='euler' only, not {solver!r}")
        gh.flux.set_step_cache(step_cache)             # what Sampler.sample_ode sets before a trajectory on this handle
        gh.flux.set_cfg(None)
        out, rng.offset = gh.generate(row_images, row_masks, t5_ids, clip_ids, rng.seed, rng.offset, cfg=cfg, steps=steps, solver=solver,
                                      time_shifting_factor=time_shifting_factor, decode_rows=decode_rows)
        return out
    dev = row_images[0].device
    lat = []
    for i, img in enumerate(row_images):                                               # :377-378
        n = None if encode_noise is None else encode_noise[i]
        lat.append(_encode(ae, img[None].to(torch.bfloat16), n, rng))
    if rng is None:
        rng = torch.Generator(device=dev).manual_seed(int(seed))                       # :394
    noise = [_draw(rng, [1, 16, img.shape[-2] // 8, img.shape[-1] // 8], dev) for img in row_images]     # :395-399
    txt = t5(t5_ids)                                                                   # prepare_modified -> HFEmbedder
    vec, _ = clip(clip_ids)
    rows = denoise_grid(model, noise, lat, row_masks, txt, vec, cfg=cfg, steps=steps, solver=solver,
                        time_shifting_factor=time_shifting_factor, step_cache=step_cache, adaptive=adaptive, sde=sde, rng=rng,
                        multistep=multistep)
    out = []
    for i in (range(len(rows)) if decode_rows is None else decode_rows):
        img = ae.decode(rows[i])[0]                                                    # :430
        out.append(((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0))                       # :431-432
    return out


def to_uint8_image(img01: torch.Tensor):
    """`to_pil_image(row_sample.float())` (visualcloze.py:437-439): [3,H,W] in [0,1] -> 8-bit RGB PIL image; torchvision's
    conversion is `pic.mul(255).byte()`, i.e. it TRUNCATES."""
    from PIL import Image
    a = img01.detach().float().mul(255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
    return Image.fromarray(a)


def compare_images(a, b):
    """How far two renderings lie apart: `hip.image_compare` (vc_image_compare: error sums, PSNR, mean SSIM, computed on the device,
    the same bits on every run) on what `generate_grid` / `upsample_images` return on either path - two f32 [3, H, W] tensors in
    [0, 1], or two uint8 [H, W, 3] tensors (the 8-bit form of vc_pixels_out) - or two lists of them of one length, image by image.
    Returns {"psnr_db", "ssim", "mse", "max_abs", "n_diff"} (a list of them for lists).  A distance between two renderings made with
    the SAME weights, seed and prompt: it ranks sampler settings against each other and says nothing about absolute image quality."""
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        if not (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))) or len(a) != len(b):
            raise ValueError("compare_images: two lists of one length (or two tensors) expected")
        return [compare_images(x, y) for x, y in zip(a, b)]
    m = hip.image_compare(a, b)
    return {k: m[k] for k in ("psnr_db", "ssim", "mse", "max_abs", "n_diff")}


def upsampling_size(target_size):
    """The size rule of `upsampling` (visualcloze.py:165-179): default 1024x1024, at most 1024^2 pixels at the requested
    aspect ratio, both sides rounded down to multiples of 16.  (w, h) in, (w, h) out."""
    if target_size is None:
        target_size = (1024, 1024)
    if target_size[0] * target_size[1] > 1024 * 1024:
        aspect = target_size[0] / target_size[1]
        new_h = int((1024 * 1024 / aspect) ** 0.5)
        target_size = (int(new_h * aspect), new_h)
    return (target_size[0] // 16) * 16, (target_size[1] // 16) * 16


def fit_size(w: int, h: int, resolution: int):
    """The size rule of `resize_with_aspect_ratio` (visualcloze.py:52-60): about resolution^2 pixels at the image's aspect ratio,
    both sides multiples of 16.  (w, h) in, (w, h) out."""
    aspect = w / h
    new_h = int((resolution * resolution / aspect) ** 0.5)
    new_w = int(new_h * aspect)
    return max(new_w // 16, 1) * 16, max(new_h // 16, 1) * 16


def _u8_tensor(image, dev=None) -> torch.Tensor:
    """a PIL image, a [3, H, W] tensor in [0, 1] or a uint8 [H, W, 3] tensor as uint8 [H, W, 3] (on `dev` if given)"""
    import numpy as np
    if torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3:
        t = image
    elif torch.is_tensor(image):
        t = image.detach().float().mul(255).to(torch.uint8).permute(1, 2, 0)           # to_pil_image's truncation, :437-439
    else:
        t = torch.from_numpy(np.asarray(image.convert("RGB"), dtype=np.uint8).copy())
    return t.contiguous() if dev is None else t.to(dev).contiguous()


def preprocess_grid(images, resolution: int = 384, device_resize: bool = False, device="cuda"):
    """The image half of `process_images` (visualcloze.py:298-374): images[i][j] the image of grid row i, column j - a PIL image or
    decoded bytes as a uint8 [H, W, 3] tensor - or None for a cell to generate (last row only).  Every image is fitted to `resolution` (LANCZOS), resized to cover its row's reference
    size (bicubic) and centre-cropped; an absent cell is black and masked; with more than one masked cell everything is resized
    once more (:350-360).  Returns (row_images, row_masks) as `generate_grid` takes them: bf16 [3, H, W_row] in [-1, 1] and bf16
    [1, 1, H, W_row] on `device`.  `device_resize=False`: PIL does the resizing, as the reference; True: only the decoded bytes go
    to the device, and vc_grid_layout, vc_resample_u8, vc_pixels_in and vc_mask_fill do the rest there - the same bits."""
    gh, gw = len(images), len(images[0])
    if any(len(r) != gw for r in images):
        raise ValueError("preprocess_grid: every row must hold the same number of cells")
    if device_resize:
        return _preprocess_grid_device([[None if im is None else _u8_tensor(im, device) for im in row] for row in images], resolution, device)
    import numpy as np
    from PIL import Image
    images = [[None if im is None else Image.fromarray(im.cpu().numpy()) if torch.is_tensor(im) else im.convert("RGB") for im in row]
              for row in images]
    cells, mask_position, target_w = [], [], None
    for i, row in enumerate(images):
        first = next((im for im in row if im is not None), None)
        ref = None if first is None else fit_size(first.width, first.height, resolution)
        if i == gh - 1 and ref is not None:
            target_w = ref[0]
        for im in row:
            if im is None:
                if i != gh - 1:
                    raise ValueError(f"preprocess_grid: row {i} lacks an image; only cells of the last row may be None")
                cells.append(Image.new("RGB", ref if ref else (resolution, resolution), (0, 0, 0)))
                mask_position.append(1)
                continue
            t = im.resize(fit_size(im.width, im.height, resolution), Image.LANCZOS)
            if t.width <= t.height:
                t = t.resize((ref[0], int(ref[0] / t.width * t.height)))
            else:
                t = t.resize((int(ref[1] / t.height * t.width), ref[1]))
            left, top = (t.width - ref[0]) // 2, (t.height - ref[1]) // 2
            cells.append(t.crop((left, top, left + ref[0], top + ref[1])))
            if i == gh - 1:
                mask_position.append(0)
    if len(mask_position) > 1 and sum(mask_position) > 1:
        width = 384 if target_w is None else target_w                                  # a running width, shared by all cells
        for k, c in enumerate(cells):
            height = int(c.height * (width / c.width))                                  # from the width BEFORE it is rounded
            width, height = int(width / 16) * 16, int(height / 16) * 16
            cells[k] = c.resize((width, height))
    rows, masks = [], []
    for i in range(gh):
        px = [torch.from_numpy(np.asarray(c, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0) for c in cells[i * gw:(i + 1) * gw]]
        px = [(p - 0.5) / 0.5 for p in px]                                             # ToTensor, Normalize(0.5, 0.5), :133-137
        ms = [torch.full((1, 1, px[0].shape[1], px[0].shape[2]), float(m if i == gh - 1 else 0)) for m in mask_position]
        rows.append(torch.cat(px, dim=2).to(device, torch.bfloat16))
        masks.append(torch.cat(ms, dim=3).to(device, torch.bfloat16))
    return rows, masks


def _preprocess_grid_device(images, resolution: int, device):
    """`images`: uint8 [H, W, 3] tensors on `device` or None"""
    plans = hip.grid_layout([[None if im is None else (im.shape[1], im.shape[0]) for im in row] for row in images], resolution)
    rows, masks = [], []
    for row, plan in zip(images, plans):
        H, W = plan[0].final_h, sum(p.final_w for p in plan)
        out = torch.empty(3, H, W, dtype=torch.bfloat16, device=device)
        mask = torch.empty(H, W, dtype=torch.bfloat16, device=device)
        x0 = 0
        for im, p in zip(row, plan):
            if im is None:
                hip.pixels_in(None, (p.final_w, H), out=out, x0=x0)
            else:
                t = hip.resample_u8(im, (p.fit_w, p.fit_h), "lanczos")
                t = hip.resample_u8(t, (p.cover_w, p.cover_h), "bicubic")
                if (p.final_w, p.final_h) == (p.cell_w, p.cell_h):
                    hip.pixels_in(t, (p.cell_w, p.cell_h), p.crop_left, p.crop_top, out=out, x0=x0)
                else:                                                                   # the crop as bytes (outside = 0), resized again
                    cell = torch.zeros(p.cell_h, p.cell_w, 3, dtype=torch.uint8, device=device)
                    sx, sy, dx, dy = max(p.crop_left, 0), max(p.crop_top, 0), max(-p.crop_left, 0), max(-p.crop_top, 0)
                    cw, ch = min(p.cover_w - sx, p.cell_w - dx), min(p.cover_h - sy, p.cell_h - dy)
                    cell[dy:dy + ch, dx:dx + cw] = t[sy:sy + ch, sx:sx + cw]
                    hip.pixels_in(hip.resample_u8(cell, (p.final_w, p.final_h), "bicubic"), (p.final_w, p.final_h), out=out, x0=x0)
            hip.mask_fill(mask, x0, p.final_w, p.mask)
            x0 += p.final_w
        rows.append(out)
        masks.append(mask[None, None])
    return rows, masks


@torch.no_grad()
def upsample_image(model, ae, t5, clip, image, target_size, t5_ids: torch.Tensor, clip_ids: torch.Tensor,
                   rng: Union[torch.Generator, NoiseStream], cfg: float = 30.0, steps: int = 10, strength: float = 0.4,
                   encode_noise: Optional[Sequence[torch.Tensor]] = None, solver: str = "euler", step_cache=None) -> torch.Tensor:
    """`VisualClozeModel.upsampling` (visualcloze.py:147-245) for one image: resize on the host (PIL, bicubic - the
    default of `Image.resize`), VAE-encode the image and a blank, SDEdit from `strength` with everything masked, decode.
    image: PIL image or [3,H,W] tensor in [0,1]; t5_ids / clip_ids: the tokenised CONTENT prompt (prefix stripping and
    tokenisation are host work, :149-163); `encode_noise`: the two DiagonalGaussian draws (image, blank) or None for
    torch.randn_like as the reference's `.sample()`; `rng`: a torch.Generator, or a `NoiseStream`, from which the draws then come
    in the reference's order - encode(image), encode(blank), start noise (:200-217).  Returns [3, h, w] in [0, 1]."""
    import numpy as np
    dev = next(ae.parameters()).device
    if torch.is_tensor(image):
        image = to_uint8_image(image)
    image = image.convert("RGB").resize(upsampling_size(target_size))                  # :179
    px = torch.from_numpy(np.asarray(image, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)   # ToTensor, :133-137
    if strength >= 1.0:
        return px.to(dev)                                                              # :180-181
    px = ((px - 0.5) / 0.5).to(dev, torch.bfloat16)                                    # Normalize(0.5, 0.5)
    n_img, n_blank = (None, None) if encode_noise is None else encode_noise
    latent = _encode(ae, px[None], None if n_img is None else n_img[None] if n_img.dim() == 3 else n_img, rng)     # :200,202
    blank = _encode(ae, torch.zeros_like(px)[None], None if n_blank is None else n_blank[None] if n_blank.dim() == 3 else n_blank, rng)
    noise = _draw(rng, [1, 16, latent.shape[-2], latent.shape[-1]], dev)               # :217
    txt = t5(t5_ids)
    vec, _ = clip(clip_ids)
    z = sdedit_upsample(model, noise, latent, blank, txt, vec, cfg=cfg, steps=steps, strength=strength, solver=solver,
                        step_cache=step_cache)
    img = ae.decode(z)[0]                                                              # :238
    return ((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0)                                # :239-240


@torch.no_grad()
def upsample_images(model, ae, t5, clip, images: Sequence, target_size, t5_ids: torch.Tensor, clip_ids: torch.Tensor,
                    rng: Union[torch.Generator, NoiseStream], cfg: float = 30.0, steps: int = 10, strength: float = 0.4,
                    encode_noise: Optional[Sequence] = None, solver: str = "euler", step_cache=None,
                    use_grid_handle: bool = False, device_resize: bool = False) -> List[torch.Tensor]:
    """`upsample_image` for several images of one grid in ONE batched SDEdit solve (`sdedit_upsample_batch`).  Host work
    (resize), the VAE encodes and every random draw happen per image in the reference's order - image k: encode(image),
    encode(blank), noise from `rng` (visualcloze.py:200-217) - so each target starts from exactly the state the
    one-at-a-time loop gives it; the prompt is encoded once (it is the same for every target, :458).  `use_grid_handle`: opt-in -
    everything behind the host resize as ONE call of the library's grid handle (vc_grid_sdedit), under the conditions of
    `generate_grid`'s switch; the same bits.  `device_resize`: opt-in, off by default - the bicubic resize runs on the device
    (vc_resample_u8: Pillow's bytes, so the same bits again); the images may then also be uint8 [H, W, 3] tensors, and those on the
    device never leave it with the grid handle on (vc_grid_sdedit_u8); without the handle only the PIL `resize` is replaced."""
    import numpy as np
    dev = next(ae.parameters()).device
    size = upsampling_size(target_size)
    gh = _grid_handle(model, ae, t5, clip, rng, "upsample_images", encode_noise=encode_noise) if use_grid_handle else None
    pxs, cells = [], []
    for image in images:
        if device_resize:
            cells.append(_u8_tensor(image, dev))
            if gh is not None and strength < 1.0:
                continue                                                               # resized inside vc_grid_sdedit_u8
            arr = hip.resample_u8(cells[-1], size).cpu().numpy()
        else:
            if torch.is_tensor(image):
                image = to_uint8_image(image)
            arr = np.asarray(image.convert("RGB").resize(size), dtype=np.uint8).copy()  # :179
        pxs.append(torch.from_numpy(arr).permute(2, 0, 1).float().div(255.0))
    if strength >= 1.0:
        return [px.to(dev) for px in pxs]                                              # :180-181
    if gh is not None:
        if step_cache is not None and solver != "euler":
            raise ValueError(f"step_cache works with sampling_method='euler' only, not {solver!r}")
        gh.flux.set_step_cache(step_cache)
        gh.flux.set_cfg(None)
        if device_resize:
            out, rng.offset = gh.sdedit_u8(cells, size, t5_ids, clip_ids, rng.seed, rng.offset, cfg=cfg, steps=steps, strength=strength,
                                           solver=solver)
            return out
        out, rng.offset = gh.sdedit([((px - 0.5) / 0.5).to(dev, torch.bfloat16) for px in pxs], t5_ids, clip_ids, rng.seed, rng.offset,
                                    cfg=cfg, steps=steps, strength=strength, solver=solver)
        return out
    lat, blank, noise = [], [], []
    for k, px in enumerate(pxs):
        px = ((px - 0.5) / 0.5).to(dev, torch.bfloat16)
        n_img, n_blank = (None, None) if encode_noise is None or encode_noise[k] is None else encode_noise[k]
        nz = lambda n: None if n is None else n[None] if n.dim() == 3 else n  # noqa: E731
        lat.append(_encode(ae, px[None], nz(n_img), rng))
        blank.append(_encode(ae, torch.zeros_like(px)[None], nz(n_blank), rng))
        noise.append(_draw(rng, [1, 16, lat[-1].shape[-2], lat[-1].shape[-1]], dev))
    txt = t5(t5_ids)
    vec, _ = clip(clip_ids)
    zs = sdedit_upsample_batch(model, noise, lat, blank, txt, vec, cfg=cfg, steps=steps, strength=strength, solver=solver,
                               step_cache=step_cache)
    return [((ae.decode(z)[0].float() + 1.0) / 2.0).clamp_(0.0, 1.0) for z in zs]     # :238-240


@torch.no_grad()
def generate_and_upsample(model, ae, t5, clip, row_images: List[torch.Tensor], row_masks: List[torch.Tensor],
                          t5_ids: torch.Tensor, clip_ids: torch.Tensor, seed: int, grid_w: int, mask_position: Sequence[bool],
                          target_size=None, content_t5_ids: Optional[torch.Tensor] = None,
                          content_clip_ids: Optional[torch.Tensor] = None, cfg: float = 30.0, steps: int = 30,
                          upsampling_steps: int = 10, upsampling_noise: float = 0.4, is_upsampling: bool = True,
                          encode_noise: Optional[List[torch.Tensor]] = None, upsample_encode_noise=None,
                          solver: str = "euler", time_shifting_factor=1, batch_targets: bool = True, step_cache=None,
                          rng: Union[torch.Generator, NoiseStream, None] = None, use_grid_handle: bool = False,
                          device_resize: bool = False):
    """Both stages of `process_images` chained (visualcloze.py:363-465): the grid is generated, its LAST row is decoded and
    quantised to 8 bits as `to_pil_image` does, every cell of that row whose `mask_position` is set is cropped
    (:452,461) and - with `is_upsampling` - refined by `upsample_image` at `target_size`, all noise coming from ONE
    generator seeded with `seed` (:394,456).  `batch_targets` (default): the masked cells are refined TOGETHER, one graph replay
    per solver step for all of them (`upsample_images`; same draws in the same order, per-target results equal up to bf16
    noise); False = one after the other as the reference loops.  `rng`: the generator both stages draw from instead of a fresh
    torch.Generator seeded with `seed` - a `NoiseStream` puts every draw of both stages on the library's own stream, in the
    reference's order.  `use_grid_handle`: opt-in - both stages through the library's grid handle (vc_grid_generate, then vc_grid_sdedit
    per batch of targets; the crop and the resize between them stay here), under the conditions of `generate_grid`'s switch; the same
    bits.  `device_resize`: opt-in, off by default - the quantised last row stays on the device, its cells are cropped there and
    resized by the library (`upsample_images(device_resize=True)`; with the grid handle: vc_grid_sdedit_u8), Pillow's bytes and so
    the same bits; every masked cell then goes through `upsample_images`, one at a time where `batch_targets` is off.
    Returns the output images as [3, h, w] tensors in [0, 1]."""
    if use_grid_handle:
        _grid_handle(model, ae, t5, clip, rng, "generate_and_upsample", encode_noise=encode_noise, upsample_encode_noise=upsample_encode_noise)
    dev = row_images[0].device
    if rng is None:
        rng = torch.Generator(device=dev).manual_seed(int(seed))
    last = len(row_images) - 1
    row = generate_grid(model, ae, t5, clip, row_images, row_masks, t5_ids, clip_ids, seed, cfg=cfg, steps=steps,
                        encode_noise=encode_noise, decode_rows=[last], solver=solver, time_shifting_factor=time_shifting_factor,
                        rng=rng, step_cache=step_cache, use_grid_handle=use_grid_handle)[0]
    if device_resize:
        return _upsample_cells_on_device(model, ae, t5, clip, _u8_tensor(row), grid_w, mask_position, target_size,
                                         content_t5_ids if content_t5_ids is not None else t5_ids,
                                         content_clip_ids if content_clip_ids is not None else clip_ids, rng, cfg, upsampling_steps,
                                         upsampling_noise, is_upsampling, upsample_encode_noise, solver, batch_targets, step_cache, use_grid_handle)
    pil = to_uint8_image(row)                                                          # :437-439
    ret_w, ret_h = pil.width, pil.height
    cells = [pil.crop((i * ret_w // grid_w, 0, (i + 1) * ret_w // grid_w, ret_h)) for i, m in enumerate(mask_position) if m]   # :452,461
    ct5 = content_t5_ids if content_t5_ids is not None else t5_ids
    cclip = content_clip_ids if content_clip_ids is not None else clip_ids
    if is_upsampling and batch_targets and len(cells) > 1:
        return upsample_images(model, ae, t5, clip, cells, target_size, ct5, cclip, rng, cfg=cfg, steps=upsampling_steps,
                               strength=upsampling_noise, encode_noise=upsample_encode_noise, solver=solver, step_cache=step_cache,
                               use_grid_handle=use_grid_handle)
    outs, k = [], 0
    for i, masked in enumerate(mask_position):
        if not masked:
            continue
        cell = pil.crop((i * ret_w // grid_w, 0, (i + 1) * ret_w // grid_w, ret_h))    # :452,461
        if is_upsampling and use_grid_handle:          # one target: a batch of one through vc_grid_sdedit
            outs += upsample_images(model, ae, t5, clip, [cell], target_size, ct5, cclip, rng, cfg=cfg, steps=upsampling_steps,
                                    strength=upsampling_noise, solver=solver, step_cache=step_cache, use_grid_handle=True)
        elif is_upsampling:
            en = None if upsample_encode_noise is None else upsample_encode_noise[k]
            outs.append(upsample_image(model, ae, t5, clip, cell, target_size, content_t5_ids if content_t5_ids is not None else t5_ids,
                                       content_clip_ids if content_clip_ids is not None else clip_ids, rng, cfg=cfg,
                                       steps=upsampling_steps, strength=upsampling_noise, encode_noise=en, solver=solver, step_cache=step_cache))
        else:
            import numpy as np
            outs.append(torch.from_numpy(np.asarray(cell, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0).to(dev))
        k += 1
    return outs


def _upsample_cells_on_device(model, ae, t5, clip, row_u8, grid_w, mask_position, target_size, ct5, cclip, rng, cfg, steps, strength,
                              is_upsampling, encode_noise, solver, batch_targets, step_cache, use_grid_handle):
    """the second stage of `generate_and_upsample(device_resize=True)`: row_u8 [H, W, 3] uint8 on the device, the quantised last row"""
    ret_w = row_u8.shape[1]
    cells = [row_u8[:, i * ret_w // grid_w:(i + 1) * ret_w // grid_w].contiguous() for i, m in enumerate(mask_position) if m]    # :452,461
    if not is_upsampling:
        return [c.permute(2, 0, 1).cpu().float().div(255.0).to(row_u8.device) for c in cells]
    kw = dict(cfg=cfg, steps=steps, strength=strength, solver=solver, step_cache=step_cache, use_grid_handle=use_grid_handle, device_resize=True)
    if batch_targets and len(cells) > 1:
        return upsample_images(model, ae, t5, clip, cells, target_size, ct5, cclip, rng, encode_noise=encode_noise, **kw)
    outs = []
    for k, cell in enumerate(cells):
        outs += upsample_images(model, ae, t5, clip, [cell], target_size, ct5, cclip, rng,
                                encode_noise=None if encode_noise is None else [encode_noise[k]], **kw)
    return outs
