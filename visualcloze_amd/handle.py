"""`FluxHandle`: the handle API of include/vcloze_hip.h (vc_flux_*) behind torch tensors — Flux.forward and the whole
fixed-grid solver loop (Euler, midpoint, rk4) as ONE C call each.  The launch plan lives in csrc/flux_engine.hip; this class
binds the prepared (bf16, LoRA-merged) weights by reference-module path, owns the workspace tensors and converts the
host-side inputs (ids, timesteps, masks) to the plain arrays the ABI takes.  Over un-merged weights (`PreparedWeights.ref`) it binds
the base weights and the LoRA pairs and runs the handle's un-merged mode (vc_flux_bind_lora, option lora_mode 1).
`engine.FluxEngine` is the same plan spelt in Python over the op-level ABI: the parity twin of both modes."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a.detach().to("cpu", torch.float32).numpy() if torch.is_tensor(a) else np.asarray(a, np.float32),
                                dtype=np.float32)


class _HostCopies:
    """Host copies of small DEVICE inputs (ids, guidance) that vc_flux_prepare takes as host arrays, remembered per argument
    while the caller keeps handing over the SAME MEMORY at the same version: a D2H copy synchronises the stream, i.e. drains
    every queued solver step - once per grid that is nothing, once per 3-evaluation sample (cfg 1) it left the GPU idle for
    2 - 6 % of the run.  The key is the memory, not the Python object: `Sampler.sample_ode` / `Flux.forward` slice their
    arguments per chunk (`MaskLayout._take`), which makes a NEW view object of the same storage on every call (advisor r04: keyed
    on identity the cache hit in bench.py only).  (storage address, offset, shape, strides, dtype, version counter - views share
    their base's); the entry holds the tensor, so the storage cannot be freed and its address recycled while the entry lives.
    These inputs are never written by the library's kernels (which would not bump the version)."""

    def __init__(self):
        self._c: Dict[str, tuple] = {}
        self.hits = self.misses = 0

    @staticmethod
    def _key(t) -> tuple:
        return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype, t._version)

    def f32(self, key: str, t) -> np.ndarray:
        if not torch.is_tensor(t) or not t.is_cuda:
            return _f32(t)
        k = self._key(t)
        e = self._c.get(key)
        if e is not None and e[0] == k:
            self.hits += 1
            return e[2]
        self.misses += 1
        a = _f32(t)
        self._c[key] = (k, t, a)
        return a


def _fp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


class _Handle:
    """What the three handles share: the `vc_*_destroy` / `vc_*_weight_name` calls named by the class attributes, the aligned base of
    a workspace tensor and the stream a captured plan runs on."""
    _destroy: str = ""
    _weight_name: str = ""      # (FluxHandle binds by reference-module path: the ABI has no vc_flux_weight_name)

    def __del__(self):
        try:
            if self.h:
                getattr(hip.lib(), self._destroy)(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def weight_names(self) -> list:
        out, buf = [], C.create_string_buffer(160)
        while getattr(hip.lib(), self._weight_name)(self.h, len(out), buf, 160) == 0:
            out.append(buf.value.decode())
        return out

    @staticmethod
    def _aligned(ws: torch.Tensor) -> Tuple[int, int]:
        """(the first 256-byte aligned address inside ws, the bytes of ws behind it)"""
        base = (ws.data_ptr() + 255) & ~255
        return base, ws.numel() - (base - ws.data_ptr())

    def _stream(self, stream):
        """(the hipStream_t value to pass, the torch stream the plan runs on when that is not torch's current stream, else None).
        stream 0 = torch's current stream; when that is the null stream - on which the library runs un-captured - the captured
        plan runs on a stream of the handle's own.  Any other value is taken as the caller's hipStream_t.  The copies into and out
        of the argument slots run on torch's current stream, so a plan on another stream is ordered behind and in front of it
        (`_join`).  None = the un-captured path, on the null stream."""
        cur = torch.cuda.current_stream(self.dev)
        if stream is None:
            cur.synchronize()
            return None, None
        if stream == 0 and cur.cuda_stream != 0:
            return cur.cuda_stream, None
        if stream != 0 and stream == cur.cuda_stream:
            return stream, None
        if stream == 0:
            if self._side is None:
                self._side = torch.cuda.Stream(self.dev)
            other = self._side
        else:
            other = torch.cuda.ExternalStream(stream, device=self.dev)
        other.wait_stream(cur)
        return other.cuda_stream, other

    def _join(self, stream, other) -> None:
        if stream is None:
            torch.cuda.synchronize(self.dev)
        elif other is not None:
            torch.cuda.current_stream(self.dev).wait_stream(other)


class FluxHandle(_Handle):
    _destroy = "vc_flux_destroy"
    MAX_BATCH = 4      # samples per launch sequence, as engine.FluxEngine

    def __init__(self, params, weights, dev: torch.device, _load=None):
        self.params, self.dev, self.W = params, dev, weights
        D = params.hidden_size
        cfg = hip.FluxConfig(params.in_channels, params.out_channels, params.vec_in_dim, params.context_in_dim, D, params.num_heads,
                             params.depth, params.depth_single_blocks, int(D * params.mlp_ratio), int(bool(params.guidance_embed)),
                             (C.c_int32 * 3)(*params.axes_dim), int(params.theta))
        self.h = C.c_void_p()
        with torch.cuda.device(dev):
            hip._check(hip.lib().vc_flux_create(C.byref(cfg), C.byref(self.h)), "vc_flux_create")
        L = hip.lib()
        self._opts: Dict[str, int] = {}
        if _load is not None:                               # from_state_dict: the library prepares and binds the set itself
            weights = self.W = self._load(*_load)
        else:
            self._bind_prepared(weights)
        hip._check(L.vc_flux_bind_weight(self.h, b"timestep_freqs", weights.temb_freqs.data_ptr(), None, 1, 128, 128),
                   "vc_flux_bind_weight(timestep_freqs)")      # torch's own f32 table: bit-equal to the Python-ordered plan
        # ONE split-K scratch for every geometry of this handle (its launches are ordered on one stream), instead of 100 MB carved
        # into each of the up to nine cached workspaces (advisor r04)
        self._sk_ws = hip.splitk_workspace(dev)
        nf = self._sk_ws.numel() // 4
        hip._check(L.vc_flux_bind_weight(self.h, b"splitk_ws", self._sk_ws.data_ptr(), None, 1, nf, nf), "vc_flux_bind_weight(splitk_ws)")
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._lora: Dict[str, tuple] = {}
        self._taps: Dict[str, torch.Tensor] = {}
        self.lora_mode = 0
        self.ws_options = dict.fromkeys(self.WS_OPTIONS, 0)     # name -> 0 / 1 as last set (`set_ws_option`)
        if getattr(weights, "ref", None) is not None:       # un-merged weights: every pair next to its base weight
            scales = []
            for name, R in weights.ref.items():
                if name.endswith(".linear1.qkv") or name.endswith(".linear1.mlp") or R.A is None:
                    continue                                # (row ranges of linear1, whose pair is bound whole)
                self.bind_lora(name, R.A, R.B, R.bB)
                scales.append(R.scale[:1])
            self.set_lora_mode(1)
            if scales:
                sc = set(torch.cat(scales).float().cpu().tolist())
                if len(sc) != 1:
                    raise hip.VclozeHipError(f"the handle's un-merged mode applies ONE lora scale to every Linear, the model holds {sorted(sc)}")
                self.set_lora_scale(sc.pop())
        self._step_cache = (0.0, 0)       # vc_flux_set_step_cache: off
        self._cfg = None                  # vc_flux_set_cfg: off
        self._monitor = None              # vc_flux_set_monitor: off
        self._monitor_bufs: Dict[tuple, tuple] = {}
        self.geom: Optional[Tuple[int, int, int, int]] = None
        self._host = _HostCopies()
        # the storage order of the bound qkv rows (head-permuted or natural) and the logit bound are PROPERTIES OF THE
        # WEIGHTS, not knobs: a handle built directly must un-permute exactly as model.handle()'s does
        if _load is None:
            self.set_options()
        else:           # vc_flux_load_finish has set what describes the weights; the rest are the defaults
            self.set_options(fuse_knorm=True, logit_bound=self.W.logit_bound)

    def _bind_prepared(self, weights) -> None:
        L = hip.lib()
        for name, off in weights.mod_off.items():          # the stacking order is part of the ABI
            if L.vc_flux_mod_offset(self.h, name.encode()) != off:
                raise hip.VclozeHipError(f"modulation row offset of {name} differs between model.prepare and libvcloze_hip.so")
        if L.vc_flux_mod_offset(self.h, None) != weights.n_mod:
            raise hip.VclozeHipError("stacked modulation size differs between model.prepare and libvcloze_hip.so")
        for name, w in weights.w.items():
            if name.endswith(".linear1.qkv") or name.endswith(".linear1.mlp"):
                continue                                    # row ranges of linear1, which is bound whole
            b = weights.b.get(name)
            rows, cols = (1, w.numel()) if w.dim() == 1 else tuple(w.shape)
            self._bind(name, w, b, rows, cols)
        self._bind("modulation", weights.mod_w, weights.mod_b, *weights.mod_w.shape)

    # ------------------------------------------------------------------ a checkpoint as stored (vc_flux_load_*)
    @classmethod
    def from_state_dict(cls, params, tensors, lora_scale: float = 1.0, dev=None) -> "FluxHandle":
        """A handle over a checkpoint AS STORED: `tensors` maps the state_dict() keys of FluxLoraWrapper (`load_keys()` lists them
        with their shapes) to tensors on the device - base weights, biases and QK-norm scales bf16 or f32, LoRA factors bf16; pairs
        may be missing.  The library merges (vc_lora_merge_qkv, one launch per Linear, `lora_scale` applied in f32), stacks the
        modulation Linears, permutes the qkv rows, casts the scales and binds the result (vc_flux_load_finish) into an arena this
        object allocates and keeps; `W` holds torch views of what is bound (vc_flux_bound).  No torch arithmetic touches a weight.
        `reload(lora_scale)` merges again into the same arena."""
        first = next(iter(tensors.values()))
        dev = torch.device(dev) if dev is not None else first.device
        return cls(params, None, dev, _load=(tensors, float(lora_scale)))

    def load_keys(self) -> list:
        """vc_flux_load_key: [(key, shape), ...] in state_dict order; the LoRA rank is reported as -1"""
        out, buf, shape, nd = [], C.create_string_buffer(160), (C.c_int64 * 2)(), C.c_int32(0)
        while hip.lib().vc_flux_load_key(self.h, len(out), buf, 160, shape, C.byref(nd)) == 0:
            out.append((buf.value.decode(), tuple(shape[:nd.value])))
        return out

    def bound(self, name: str):
        """vc_flux_bound: (w, bias) bound under a vc_flux_bind_weight name as (pointer, rows, cols, row stride) and the bias pointer"""
        w, b, rows, cols, ld = C.c_void_p(), C.c_void_p(), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        hip._check(hip.lib().vc_flux_bound(self.h, name.encode(), C.byref(w), C.byref(b), C.byref(rows), C.byref(cols), C.byref(ld)),
                   f"vc_flux_bound({name})")
        return w.value, b.value, rows.value, cols.value, ld.value

    def _view(self, ptr, rows, cols):
        """the [rows, cols] bf16 tensor at device address `ptr` of the arena"""
        off = ptr - self._arena.data_ptr()
        return self._arena[off:off + 2 * rows * cols].view(torch.bfloat16).view(rows, cols)

    def _load(self, tensors, lora_scale):
        from .engine import PreparedWeights
        L = hip.lib()
        self._loaded = {}
        for key, t in tensors.items():
            t = t.detach()
            if not t.is_cuda or t.device != self.dev or t.dtype not in (torch.bfloat16, torch.float32):
                raise hip.VclozeHipError(f"from_state_dict: {key} must be a bf16 / f32 tensor on {self.dev}, got {t.dtype} on {t.device}")
            t = t.contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            hip._check(L.vc_flux_load_tensor(self.h, key.encode(), t.data_ptr(), int(t.dtype == torch.float32), shape, t.dim()),
                       f"vc_flux_load_tensor({key})")
            self._loaded[key] = t
        n = L.vc_flux_load_bytes(self.h)
        self._arena = torch.empty(n + 256, dtype=torch.uint8, device=self.dev)
        self._finish(lora_scale)
        w, b = {}, {}
        D, H = self.params.hidden_size, self.params.num_heads
        mods = {}
        for key, shape in self.load_keys():
            if key.endswith(".scale"):
                w[key] = self._view(*self.bound(key)[:1], 1, 128).reshape(128)
            elif key.endswith(".weight") and ".lora_" not in key:
                name = key[:-len(".weight")]
                off = L.vc_flux_mod_offset(self.h, name.encode())
                if off >= 0:
                    mods[name] = off
                    continue
                wp, bp, rows, cols, _ = self.bound(name)
                w[name] = self._view(wp, rows, cols)
                b[name] = None if not bp else self._view(bp, 1, rows).reshape(rows)
                if name.endswith(".linear1"):
                    w[name + ".qkv"], w[name + ".mlp"] = w[name][:3 * D], w[name][3 * D:]
                    b[name + ".qkv"], b[name + ".mlp"] = (None, None) if b[name] is None else (b[name][:3 * D], b[name][3 * D:])
        wp, bp, rows, cols, _ = self.bound("modulation")
        half = 128
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).to(self.dev)
        # the per-block logit bounds as model.Flux.prepare holds them (read by engine-side tools; the C plan computes its own)
        amax = {k: float(t.float().abs().max()) for k, t in w.items() if k.endswith(("query_norm.scale", "key_norm.scale"))}
        c_log = 1.02 * 11.313708498984761 * 1.4426950408889634
        bounds = {}
        for pf in sorted({k.split(".img_attn.")[0].split(".txt_attn.")[0].split(".norm.")[0] for k in amax}):
            qm = max(v for k, v in amax.items() if k.startswith(pf + ".") and k.endswith("query_norm.scale"))
            km = max(v for k, v in amax.items() if k.startswith(pf + ".") and k.endswith("key_norm.scale"))
            bnd = c_log * qm * km
            bounds[pf] = float(torch.tensor(bnd, dtype=torch.float32)) if bnd == bnd else 1e30
        bound = max(bounds.values()) if bounds else 0.0
        # what vc_flux_load_finish set is remembered as set, so that set_options never overrides the library's values with these
        self._opts.update(qkv_heads=H, fuse_knorm=1, logit_bound_milli=int(math.ceil(bound * 1000)) if 0 < bound < 2e6 else 0)
        return PreparedWeights(w=w, b=b, mod_w=self._view(wp, rows, cols), mod_b=self._view(bp, 1, rows).reshape(rows), mod_off=mods,
                               n_mod=rows, temb_freqs=freqs, ref=None, qkv_heads=H, logit_bound=bound, logit_bounds=bounds)

    def _finish(self, lora_scale: float) -> None:
        base, nbytes = self._aligned(self._arena)
        with torch.cuda.device(self.dev):
            hip._check(hip.lib().vc_flux_load_finish(self.h, float(lora_scale), base, nbytes, hip.cur_stream()), "vc_flux_load_finish")
        self.lora_scale = float(lora_scale)

    def reload(self, lora_scale: float) -> None:
        """vc_flux_load_finish once more with another scale: the same arena (the views of `W` see the new values), the handle
        un-prepared"""
        self._finish(lora_scale)
        self.geom = None

    def _bind(self, name, w, b, rows, cols):
        hip._bf16(w, name)
        if w.stride(-1) != 1 or (b is not None and not b.is_contiguous()):
            raise hip.VclozeHipError(f"{name}: weight rows / bias must be contiguous")
        hip._check(hip.lib().vc_flux_bind_weight(self.h, name.encode(), w.data_ptr(), hip._p(b), rows, cols,
                                                 w.stride(0) if w.dim() == 2 else cols), f"vc_flux_bind_weight({name})")

    def set_options(self, attn_variant=None, tile_cfg=0, fuse_qnorm=2, fuse_vt=True, qkv_heads=None, fuse_knorm=False,
                    logit_bound=0.0, mlp_first=False, splitk=True) -> None:
        wq = int(getattr(self.W, "qkv_heads", 0) or 0)
        if qkv_heads is None:
            qkv_heads = wq
        elif int(qkv_heads) != wq:
            raise hip.VclozeHipError(f"set_options(qkv_heads={qkv_heads}): the bound qkv weights are stored with qkv_heads={wq} "
                                     "(model.prepare / hip.qkv_head_permutation); the option follows the weights")
        want = dict(attn_variant=-1 if attn_variant is None else int(attn_variant), tile_cfg=int(tile_cfg),
                    fuse_qnorm=int(fuse_qnorm), fuse_vt=int(bool(fuse_vt)), qkv_heads=int(qkv_heads),
                    fuse_knorm=int(bool(fuse_knorm)),
                    logit_bound_milli=int(math.ceil(logit_bound * 1000)) if 0 < logit_bound < 2e6 else 0,
                    mlp_first=int(bool(mlp_first)), splitk=int(bool(splitk)))
        for k, v in want.items():
            if self._opts.get(k) != v:
                hip._check(hip.lib().vc_flux_set_option(self.h, k.encode(), v), f"vc_flux_set_option({k})")
                self._opts[k] = v

    def bind_lora(self, name: str, lora_a, lora_b, lora_b_bias=None) -> None:
        """vc_flux_bind_lora: the pair of Linear `name` (bound already) - lora_a [r, in], lora_b [out, r], lora_b's bias [out] or
        None, bf16 on the handle's device, kept alive here.  A rank that is no multiple of 64 is zero-padded (new tensors).  Both
        None removes the pair."""
        if lora_a is None and lora_b is None:
            hip._check(hip.lib().vc_flux_bind_lora(self.h, name.encode(), None, 0, None, 0, None, 0, 0, 0), f"vc_flux_bind_lora({name})")
            self._lora.pop(name, None)
            self._ws.clear()
            self.geom = None
            return
        hip._bf16(lora_a, name + ".lora_A"); hip._bf16(lora_b, name + ".lora_B")
        r = lora_a.shape[0]
        if r % 64:
            rk = (r + 63) // 64 * 64
            A = torch.zeros(rk, lora_a.shape[1], dtype=torch.bfloat16, device=lora_a.device)
            Bm = torch.zeros(lora_b.shape[0], rk, dtype=torch.bfloat16, device=lora_b.device)
            A[:r], Bm[:, :r] = lora_a, lora_b
            lora_a, lora_b = A, Bm
        if lora_a.stride(1) != 1 or lora_b.stride(1) != 1 or (lora_b_bias is not None and not lora_b_bias.is_contiguous()):
            raise hip.VclozeHipError(f"{name}: LoRA factor rows / bias must be contiguous")
        if lora_b_bias is not None:
            hip._bf16(lora_b_bias, name + ".lora_B.bias")
        hip._check(hip.lib().vc_flux_bind_lora(self.h, name.encode(), lora_a.data_ptr(), lora_a.stride(0), lora_b.data_ptr(),
                                               lora_b.stride(0), hip._p(lora_b_bias), lora_b.shape[0], lora_a.shape[1], lora_a.shape[0]),
                   f"vc_flux_bind_lora({name})")
        self._lora[name] = (lora_a, lora_b, lora_b_bias)
        self._ws.clear()          # the widest rank sizes the scratch
        self.geom = None

    def set_lora_mode(self, mode: int) -> None:
        """vc_flux_set_option("lora_mode"): 1 = the bound weights are un-merged base weights and every Linear runs LinearLora's
        three roundings (lora.py:92-98); 0 = plain Linears.  A switch needs a new prepare (other workspace size)."""
        hip._check(hip.lib().vc_flux_set_option(self.h, b"lora_mode", int(mode)), "vc_flux_set_option(lora_mode)")
        if int(bool(mode)) != self.lora_mode:
            self.lora_mode = int(bool(mode))
            self._ws.clear()
            self.geom = None

    # the workspace options: name -> what the workspace holds while the option is 1
    WS_OPTIONS = {"adaptive": "the buffers of the adaptive solve (`sample_dopri5`, `sample_rk`)",
                  "sde": "the buffers of the stochastic sampler (`sample_sde`)",
                  "eval_loss": "u_t of the flow-matching loss (`eval_loss`)",
                  "multistep": "the buffers of the Adams-Bashforth solve (`sample_multistep`)"}

    def set_ws_option(self, name: str, on: bool) -> None:
        """vc_flux_set_option(name) for a name of WS_OPTIONS: 1 = the workspace holds what the table says.  A switch needs a new prepare
        (other workspace size); with it off nothing differs from a handle that never heard of it."""
        if name not in self.WS_OPTIONS:
            raise KeyError(f"set_ws_option: {name!r} is no workspace option ({sorted(self.WS_OPTIONS)})")
        hip._check(hip.lib().vc_flux_set_option(self.h, name.encode(), int(bool(on))), f"vc_flux_set_option({name})")
        if int(bool(on)) != self.ws_options[name]:
            self.ws_options[name] = int(bool(on))
            self.geom = None

    def set_adaptive(self, on: bool) -> None:
        self.set_ws_option("adaptive", on)

    def set_sde(self, on: bool) -> None:
        self.set_ws_option("sde", on)

    def set_eval_loss(self, on: bool) -> None:
        self.set_ws_option("eval_loss", on)

    def set_multistep(self, on: bool) -> None:
        self.set_ws_option("multistep", on)

    def plan_count(self) -> int:
        """vc_flux_plan_count: the captured steps the handle holds"""
        return hip.lib().vc_flux_plan_count(self.h)

    def set_lora_scale(self, scale: float) -> None:
        """vc_flux_set_lora_scale: the scale of every pair; a bf16 value, anything else is refused, and so is a change while a
        trajectory is in flight.  Call `prepare` again after a change (forward / sample_* refuse a prepared state of the old scale);
        captured steps stay and replay with the new scale."""
        hip._check(hip.lib().vc_flux_set_lora_scale(self.h, float(scale)), "vc_flux_set_lora_scale")

    def tap_shape(self, name: str) -> Tuple[int, int]:
        rows, cols = C.c_int64(0), C.c_int32(0)
        hip._check(hip.lib().vc_flux_tap_shape(self.h, name.encode(), C.byref(rows), C.byref(cols)), f"vc_flux_tap_shape({name})")
        return rows.value, cols.value

    def set_tap(self, name: str, dst: Optional[torch.Tensor]) -> None:
        """vc_flux_set_tap: `dst` (bf16, contiguous, tap_shape(name) elements, kept alive here) receives the residual stream `name` -
        img_in, txt_in, double.{i}.img, double.{i}.txt, single.{i} - of every evaluation issued from the next forward / sample_begin on;
        None removes the tap."""
        if dst is not None:
            hip._bf16(dst, name)
            rows, cols = self.tap_shape(name)
            if not dst.is_contiguous() or dst.numel() != rows * cols:
                raise hip.VclozeHipError(f"set_tap({name}): a contiguous bf16 buffer of {rows} x {cols} expected, got {tuple(dst.shape)}")
        hip._check(hip.lib().vc_flux_set_tap(self.h, name.encode(), hip._p(dst)), f"vc_flux_set_tap({name})")
        if dst is None:
            self._taps.pop(name, None)
        else:
            self._taps[name] = dst

    def tap_names(self) -> list:
        p = self.params
        return (["img_in", "txt_in"] + [f"double.{i}.{st}" for i in range(p.depth) for st in ("img", "txt")]
                + [f"single.{i}" for i in range(p.depth_single_blocks)])

    def set_step_cache(self, step_cache=None) -> None:
        """vc_flux_set_step_cache: a `transport.StepCache` (or anything with .threshold / .max_consecutive), or None = off.
        Takes effect at the next prepare + sample_begin (the workspace grows by 3 * B * N * hidden bf16 while it is on)."""
        want = (0.0, 0) if step_cache is None else (float(step_cache.threshold), int(step_cache.max_consecutive))
        if want != self._step_cache:
            hip._check(hip.lib().vc_flux_set_step_cache(self.h, want[0], want[1]), "vc_flux_set_step_cache")
            self._step_cache = want

    def set_cfg(self, cfg_scale: Optional[float] = None) -> None:
        """vc_flux_set_cfg: true classifier-free guidance in the sampling loop (the drift is Flux.forward_with_cfg) with this
        scale, or None = off.  Takes effect at the next sample_begin / sample_ode; the batch then holds the conditional samples
        first and the unconditional ones behind them (an even B)."""
        want = None if cfg_scale is None else float(cfg_scale)
        if want != self._cfg or (want is not None and want != want):
            hip._check(hip.lib().vc_flux_set_cfg(self.h, int(want is not None), 0.0 if want is None else want), "vc_flux_set_cfg")
            self._cfg = want

    def step_cache_stats(self, capacity: int = 256) -> dict:
        """vc_flux_step_cache_stats of the trajectory in flight or just finished: {"computed", "reused", "metrics"}; metrics[i] is
        the m of evaluation i, NaN where none existed (the first evaluation; every evaluation with the cache off)."""
        c, r = C.c_int32(0), C.c_int32(0)
        m = (C.c_float * max(int(capacity), 1))()
        hip._check(hip.lib().vc_flux_step_cache_stats(self.h, C.byref(c), C.byref(r), m, int(capacity)), "vc_flux_step_cache_stats")
        n = min(int(capacity), c.value + r.value)
        return {"computed": c.value, "reused": r.value, "metrics": [float(m[i]) for i in range(n)]}

    def workspace(self, B: int, T: int, N: int, S: int) -> torch.Tensor:
        key = (B, T, N, S, self._step_cache[0] > 0 and self._step_cache[1] != 0) + tuple(k for k, on in self.ws_options.items() if on)
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) > 8:
                self._ws.clear()
            n = hip.lib().vc_flux_workspace_bytes(self.h, B, T, N, S)
            if n <= 0:
                raise hip.VclozeHipError(f"vc_flux_workspace_bytes({key[:4]}) = {n}")
            ws = torch.empty(n + 256, dtype=torch.uint8, device=self.dev)
            self._ws[key] = ws
        return ws

    def prepare(self, txt, y, guidance, guidance_is_bf16: bool, img_ids, txt_ids, max_steps: int,
                kv_len: Optional[Sequence[int]] = None, kv_gap: Optional[Sequence[Tuple[int, int]]] = None, stream=None) -> None:
        """txt [B,T,ctx] / y [B,vec] bf16 device tensors; guidance [B] (any device) or None; ids [B,N|T,3]; kv_len B ints;
        kv_gap B (lo, hi) pairs (model.MaskLayout).  max_steps bounds model EVALUATIONS: steps * hip.solver_evals(method)."""
        hip._bf16(txt, "txt"); hip._bf16(y, "y")
        B, T = txt.shape[0], txt.shape[1]
        N = img_ids.shape[-2]
        txt, y = txt.contiguous(), y.contiguous()
        g = None
        if guidance is not None:
            g = self._host.f32("guidance", guidance).reshape(-1)
            g = np.ascontiguousarray(np.broadcast_to(g, (B,)) if g.size == 1 else g.reshape(B))
        ii, ti = self._host.f32("img_ids", img_ids).reshape(B, N, 3), self._host.f32("txt_ids", txt_ids).reshape(B, T, 3)
        kv = None if kv_len is None or all(int(v) == T + N for v in kv_len) else np.asarray([int(v) for v in kv_len], np.int32)
        gp = None
        if kv_gap is not None and any(hi > lo for lo, hi in kv_gap):
            gp = np.asarray([[int(lo), int(hi)] for lo, hi in kv_gap], np.int32).reshape(-1)
            if kv is None:
                kv = np.full(B, T + N, np.int32)
        ws = self.workspace(B, T, N, max_steps)
        base, nbytes = self._aligned(ws)
        inp = hip.FluxInputs(B, T, N, max_steps, txt.data_ptr(), y.data_ptr(), _fp(g), _fp(ii), _fp(ti), _ip(kv), _ip(gp),
                             int(bool(guidance_is_bf16)), 0)
        hip._check(hip.lib().vc_flux_prepare(self.h, C.byref(inp), base, nbytes,
                                             stream if stream is not None else hip.cur_stream()), "vc_flux_prepare")
        self.geom = (B, T, N, max_steps)
        self._keep = (txt, y, ws)

    def forward(self, img, timesteps, timesteps_is_bf16: bool, out, stream=None) -> None:
        """img [B,N,in] bf16 -> out [B,N,out] bf16 (both contiguous), timesteps: B values"""
        hip._bf16(img, "img"); hip._bf16(out, "out")
        if not (img.is_contiguous() and out.is_contiguous()):
            raise hip.VclozeHipError("vc_flux_forward: contiguous img / out expected")
        t = _f32(timesteps).reshape(-1)
        if t.size != self.geom[0]:
            raise hip.VclozeHipError(f"vc_flux_forward: {t.size} timesteps for a batch of {self.geom[0]}")
        hip._check(hip.lib().vc_flux_forward(self.h, img.data_ptr(), _fp(t), int(bool(timesteps_is_bf16)), out.data_ptr(),
                                             stream if stream is not None else hip.cur_stream()), "vc_flux_forward")

    def eval_loss(self, x1, cond, t, x0=None, seed: int = 0, offset: int = 0, loss=None, stream=None) -> torch.Tensor:
        """vc_flux_eval_loss (after `set_eval_loss(True)` and a prepare): the flow-matching loss of the prepared samples, f32 [B] on the
        device.  x1 [B, N, out] bf16 / f32 contiguous, rows in the handle's order; cond [B, N, in - out] bf16; t: B
        values (host); x0: a contiguous tensor of x1's shape and dtype, or None = drawn in the kernel at (seed, offset + flat index)."""
        if self.geom is None:
            raise hip.VclozeHipError("vc_flux_eval_loss: call prepare first")
        B, _, N, _ = self.geom
        p = self.params
        if x1.dtype not in (torch.bfloat16, torch.float32) or tuple(x1.shape) != (B, N, p.out_channels) or not x1.is_contiguous():
            raise hip.VclozeHipError(f"vc_flux_eval_loss: a contiguous bf16 / f32 x1 of shape {(B, N, p.out_channels)} expected, got "
                                     f"{x1.dtype} {tuple(x1.shape)}")
        if cond is None:
            raise hip.VclozeHipError(f"vc_flux_eval_loss: cond {(B, N, p.in_channels - p.out_channels)} is required (x1 || cond feeds img_in)")
        hip._bf16(cond, "cond")
        if tuple(cond.shape) != (B, N, p.in_channels - p.out_channels) or not cond.is_contiguous():
            raise hip.VclozeHipError(f"vc_flux_eval_loss: a contiguous cond of shape {(B, N, p.in_channels - p.out_channels)} expected")
        if x0 is not None and (x0.dtype != x1.dtype or x0.shape != x1.shape or not x0.is_contiguous()):
            raise hip.VclozeHipError("vc_flux_eval_loss: x0 must be a contiguous tensor of x1's shape and dtype")
        tt = _f32(t).reshape(-1)
        if tt.size != B:
            raise hip.VclozeHipError(f"vc_flux_eval_loss: {tt.size} times for a batch of {B}")
        if loss is None:
            loss = torch.empty(B, dtype=torch.float32, device=self.dev)
        hip._check(hip.lib().vc_flux_eval_loss(self.h, x1.data_ptr(), int(x1.dtype == torch.float32), hip._p(cond), _fp(tt), hip._p(x0),
                                               hip._u64(seed, "seed"), hip._u64(offset, "offset"), loss.data_ptr(),
                                               stream if stream is not None else hip.cur_stream()), "vc_flux_eval_loss")
        return loss

    @staticmethod
    def _method(method) -> int:
        if isinstance(method, str):
            if method not in hip.SOLVERS:
                raise hip.VclozeHipError(f"unknown solver {method!r}: the fused loop implements {sorted(hip.SOLVERS)}")
            return hip.SOLVERS[method]
        return int(method)

    def _sample_args(self, what, method, x, cond, t_grid, state_is_bf16, trajectory=None) -> tuple:
        """the checked leading arguments of vc_flux_sample_begin_ode / vc_flux_sample_ode"""
        want = torch.bfloat16 if state_is_bf16 else torch.float32     # the ABI takes the state in the caller's dtype
        for t, name in ((x, "state"), (trajectory, "trajectory")):
            if t is not None and t.dtype != want:
                raise hip.VclozeHipError(f"{what}: state_is_bf16={bool(state_is_bf16)} needs a {want} {name} tensor, got {t.dtype}")
        hip._bf16(cond, "cond")
        if not all(t.is_contiguous() for t in (x, cond, trajectory) if t is not None):
            raise hip.VclozeHipError(f"{what}: contiguous x / cond / trajectory expected")
        t = _f32(t_grid).reshape(-1)
        return self.h, self._method(method), x.data_ptr(), cond.data_ptr(), _fp(t), t.size, int(bool(state_is_bf16))

    def sample_begin(self, x, cond, t_grid, state_is_bf16: bool, stream, method="euler") -> None:
        args = self._sample_args("vc_flux_sample_begin_ode", method, x, cond, t_grid, state_is_bf16)
        hip._check(hip.lib().vc_flux_sample_begin_ode(*args, stream), "vc_flux_sample_begin_ode")

    def sample_steps(self, n: int, stream, trajectory=None) -> None:
        hip._check(hip.lib().vc_flux_sample_steps(self.h, n, hip._p(trajectory), stream), "vc_flux_sample_steps")

    def profile(self, evaluations: int, stream) -> list:
        """vc_flux_profile: HIP-event times of the launches of `evaluations` evaluations at the current step of the sample in
        flight, class by class - a list of dicts (kind, epi, n, k, launches, flops, bytes, total_us, min_us, max_us)."""
        cap = 32
        out = (hip.FluxLaunchClass * cap)()
        n = C.c_int32(0)
        hip._check(hip.lib().vc_flux_profile(self.h, int(evaluations), out, cap, C.byref(n), stream), "vc_flux_profile")
        return [{k: getattr(out[i], k) for k, _ in hip.FluxLaunchClass._fields_ if not k.startswith("reserved")} for i in range(n.value)]

    def sample_end(self, x_out, stream) -> None:
        hip._check(hip.lib().vc_flux_sample_end(self.h, x_out.data_ptr(), stream), "vc_flux_sample_end")

    def sample_ode(self, method, x, cond, t_grid, state_is_bf16: bool, stream, trajectory=None) -> None:
        """vc_flux_sample_ode with method "euler" | "midpoint" | "rk4" (or a VC_SOLVER_* code).  x [B,N,C] in place (bf16, or f32
        with state_is_bf16 False): x(t_grid[0]) -> x(t_grid[-1]); the prepared max_steps must hold (len(t_grid) - 1) *
        hip.solver_evals(method) evaluations; trajectory: optional [S,B,N,C] buffer of the state's dtype, trajectory[i] = the state
        after STEP i"""
        args = self._sample_args("vc_flux_sample_ode", method, x, cond, t_grid, state_is_bf16, trajectory)
        hip._check(hip.lib().vc_flux_sample_ode(*args, hip._p(trajectory), stream), "vc_flux_sample_ode")

    def sample_euler(self, x, cond, t_grid, state_is_bf16: bool, stream, trajectory=None) -> None:
        self.sample_ode("euler", x, cond, t_grid, state_is_bf16, stream, trajectory)

    def _sample_adaptive(self, name, method, x, cond, t_grid, state_is_bf16, stream, rtol, atol, max_attempts, trajectory) -> None:
        """the adaptive entry point `name`; method: the VC_RK_* argument of vc_flux_sample_rk, None for vc_flux_sample_dopri5, which takes none"""
        args = self._sample_args(name, 0, x, cond, t_grid, state_is_bf16, trajectory)
        pair = () if method is None else (hip._rk_code(method),)
        hip._check(getattr(hip.lib(), name)(args[0], *pair, *args[2:], float(rtol), float(atol), int(max_attempts), hip._p(trajectory), stream),
                   name)

    def sample_dopri5(self, x, cond, t_grid, state_is_bf16: bool, stream, rtol: float = 1e-3, atol: float = 1e-6,
                      max_attempts: int = 1000, trajectory=None) -> None:
        """vc_flux_sample_dopri5 (after `set_adaptive(True)` and a prepare with max_steps >= 7): x [B,N,C] in place, x(t_grid[0]) ->
        x(t_grid[-1]) by the adaptive Dormand-Prince 5(4) solve; trajectory: optional [len(t_grid) - 1, B, N, C] buffer receiving
        x(t_grid[1:]) (dense output).  The state is stepped in f32 whatever its dtype.  `dopri5_log()` tells what the solve did."""
        self._sample_adaptive("vc_flux_sample_dopri5", None, x, cond, t_grid, state_is_bf16, stream, rtol, atol, max_attempts, trajectory)

    def sample_rk(self, method, x, cond, t_grid, state_is_bf16: bool, stream, rtol: float = 1e-3, atol: float = 1e-6,
                  max_attempts: int = 1000, trajectory=None) -> None:
        """vc_flux_sample_rk (after `set_adaptive(True)` and a prepare with max_steps >= the method's stages): `sample_dopri5` with the
        embedded pair `method` - "bosh3" | "adaptive_heun" (hip.RK_METHODS) or a VC_RK_* code; 3 / 2 evaluations per attempt.
        `dopri5_log()` tells what the solve did (one log serves both)."""
        self._sample_adaptive("vc_flux_sample_rk", method, x, cond, t_grid, state_is_bf16, stream, rtol, atol, max_attempts, trajectory)

    def sample_sde(self, method: str, x, cond, t_grid, state_is_bf16: bool, stream, form: str = "SBDM", norm: float = 1.0,
                   last_step="Mean", last_step_size: float = 0.04, seed: int = 0, offset: int = 0, trajectory=None) -> None:
        """vc_flux_sample_sde (after `set_sde(True)` and a prepare with max_steps >= the plan's evaluations): x [B,N,C] in place,
        x(t_grid[0]) -> the sample, by the stochastic sampler `method` ("Euler" | "Heun"); trajectory: optional [len(t_grid), B, N, C]
        buffer: x' after every loop step, the last step's result as the final row.  Draw d takes the positions offset + d * x.numel()
        + i of the stream of `seed`.  The state is stepped in f32 whatever its dtype."""
        args = self._sample_args("vc_flux_sample_sde", 0, x, cond, t_grid, state_is_bf16, trajectory)
        hip._check(hip.lib().vc_flux_sample_sde(self.h, hip._cstr(method), args[2], args[3], args[4], args[5], hip._cstr(form), float(norm),
                                                hip._cstr(last_step), float(last_step_size), hip._u64(seed, "seed"), hip._u64(offset, "offset"),
                                                args[6], hip._p(trajectory), stream), "vc_flux_sample_sde")

    def sample_multistep(self, order: int, x, cond, t_grid, state_is_bf16: bool, stream, trajectory=None) -> None:
        """vc_flux_sample_multistep (after `set_multistep(True)` and a prepare with max_steps >= len(t_grid) - 1): x [B,N,C] in place,
        x(t_grid[0]) -> x(t_grid[-1]) by the Adams-Bashforth rule of `order` (1..4), one evaluation per step; trajectory: optional
        [len(t_grid), B, N, C] buffer: the start state, then the state after every step.  The state is stepped in f32 whatever its
        dtype."""
        args = self._sample_args("vc_flux_sample_multistep", 0, x, cond, t_grid, state_is_bf16, trajectory)
        hip._check(hip.lib().vc_flux_sample_multistep(self.h, int(order), args[2], args[3], args[4], args[5], args[6], hip._p(trajectory),
                                                      stream), "vc_flux_sample_multistep")

    def dopri5_log(self) -> dict:
        """vc_flux_dopri5_log of the last `sample_dopri5`: {"attempts": [(t, dt, ratio, accepted), ...], "evaluations", "rejected"}"""
        n, ev = C.c_int32(0), C.c_int32(0)
        L = hip.lib()
        hip._check(L.vc_flux_dopri5_log(self.h, None, None, None, None, 0, C.byref(n), C.byref(ev)), "vc_flux_dopri5_log")
        cap = max(n.value, 1)
        t, dt, r, a = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_float * cap)(), (C.c_int32 * cap)()
        hip._check(L.vc_flux_dopri5_log(self.h, t, dt, r, a, cap, C.byref(n), C.byref(ev)), "vc_flux_dopri5_log")
        att = [(t[i], dt[i], float(r[i]), bool(a[i])) for i in range(n.value)]
        return {"attempts": att, "evaluations": ev.value, "rejected": sum(1 for x in att if not x[3])}

    def rk_log(self) -> dict:
        """vc_flux_rk_log: `dopri5_log()` under the embedded pairs' name - the log of the last adaptive solve on the handle"""
        return self.dopri5_log()

    # ------------------------------------------------------------------ the numerics monitor (vc_flux_set_monitor)
    def monitor_sites(self) -> list:
        """vc_flux_monitor_sites: the site names of the level set, in log order"""
        out, buf = [], C.create_string_buffer(64)
        while hip.lib().vc_flux_monitor_sites(self.h, len(out), buf, 64) == 0:
            out.append(buf.value.decode())
        return out

    def set_monitor(self, level: int, capacity: int = 0) -> None:
        """vc_flux_set_monitor: level 0 = off; 1 = the statistics of "v" and "x" per evaluation; 2 = those and every tap site.  The
        log of `capacity` evaluations and the scratch are allocated here for the PREPARED batch (call `prepare` first) and kept per
        (level, capacity, B): their addresses are part of the key a captured step is kept under, so a second trajectory of the same
        shape replays the step the first one captured.  Takes effect at the next forward / sample_begin."""
        L = hip.lib()
        if not level:
            hip._check(L.vc_flux_set_monitor(self.h, 0, None, 0, None), "vc_flux_set_monitor")
            self._monitor = None
            return
        if self.geom is None:
            raise hip.VclozeHipError("set_monitor: call prepare first (the log holds the samples of the prepared geometry)")
        B = self.geom[0]
        n_sites = 2 + (len(self.tap_names()) if int(level) >= 2 else 0)
        key = (int(level), int(capacity), B)
        if key not in self._monitor_bufs:
            if len(self._monitor_bufs) > 8:
                self._monitor_bufs.clear()
            self._monitor_bufs[key] = (torch.zeros(max(int(capacity), 0) * n_sites * B * C.sizeof(hip.Stat) + 16, dtype=torch.uint8, device=self.dev),
                                       torch.empty(B * 4 * hip.MONITOR_MAX_BLOCKS, dtype=torch.float32, device=self.dev))
        log, scratch = self._monitor_bufs[key]
        hip._check(L.vc_flux_set_monitor(self.h, int(level), log.data_ptr(), int(capacity), scratch.data_ptr()), "vc_flux_set_monitor")
        lb, sb = C.c_int64(0), C.c_int64(0)
        hip._check(L.vc_flux_monitor_bytes(self.h, int(capacity), C.byref(lb), C.byref(sb)), "vc_flux_monitor_bytes")
        if lb.value > log.numel() or sb.value > scratch.numel() * 4:
            L.vc_flux_set_monitor(self.h, 0, None, 0, None)
            raise hip.VclozeHipError(f"set_monitor: the library asks for {lb.value} + {sb.value} bytes, {log.numel()} + {scratch.numel() * 4} allocated")
        self._monitor = (int(level), int(capacity), B, log, scratch, self.monitor_sites())

    def step_nodes(self) -> tuple:
        """vc_flux_step_nodes: the graph nodes of the captured step of the trajectory begun last (step; with the step cache on head,
        tail-compute, tail-reuse)"""
        n = (C.c_int32 * 3)()
        hip._check(hip.lib().vc_flux_step_nodes(self.h, n), "vc_flux_step_nodes")
        return tuple(n)

    def monitor_report(self, stream=None):
        """vc_flux_monitor_report: (evaluation, site name, sample) of the first logged entry with a NaN / inf - in evaluation, then
        site, then sample order - or None; synchronises the stream"""
        ev, site, b, n = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(0)
        hip._check(hip.lib().vc_flux_monitor_report(self.h, C.byref(ev), C.byref(site), C.byref(b), C.byref(n),
                                                    stream if stream is not None else hip.cur_stream()), "vc_flux_monitor_report")
        self._monitor_evals = n.value
        return None if ev.value < 0 else (ev.value, self._monitor[5][site.value], b.value)

    def monitor_log(self, stream=None) -> dict:
        """the log of the evaluations issued since the last forward / sample_begin: {site name: {"max_abs", "sum_sq", "nonfinite",
        "count": numpy arrays [evaluations, B]}}; synchronises the stream"""
        if getattr(self, "_monitor", None) is None:
            raise hip.VclozeHipError("monitor_log: the monitor is off (set_monitor)")
        self.monitor_report(stream)
        _, cap, B, log, _, names = self._monitor
        rec = hip.stats_to_numpy(log[:cap * len(names) * B * C.sizeof(hip.Stat)]).reshape(cap, len(names), B)[:self._monitor_evals]
        return {name: {f: rec[:, i, :][f].copy() for f in hip.STAT_DTYPE.names} for i, name in enumerate(names)}


class VaeHandle(_Handle):
    """The autoencoder handle of include/vcloze_hip.h (vc_vae_*) behind torch tensors: `AutoEncoder.decode` / `.encode` of ONE
    image as one C call each, one hipGraph launch once the plan is captured.  The launch plan lives in csrc/vae_engine.hip;
    `vae.AutoEncoder`'s own Python-ordered plan is its parity twin (same kernels, same order, same bits).  This class binds the
    module's parameters as `state_dict()` stores them (the library re-lays them out), owns the workspace per image size and - since
    a captured plan holds its argument pointers - one set of input / output tensors per (size, direction, form): arguments are copied
    in, results are returned as fresh tensors."""
    _destroy, _weight_name = "vc_vae_destroy", "vc_vae_weight_name"

    def __init__(self, ae, dev: Optional[torch.device] = None):
        enc, dec = ae.encoder, ae.decoder
        self.dev = torch.device(dev) if dev is not None else next(ae.parameters()).device
        widths = [lvl.block[0].out_channels for lvl in dec.up]
        mult = [w // dec.ch for w in widths]
        self.cfg = hip.VaeConfig(enc.in_channels, dec.ch, dec.out_ch, (C.c_int32 * 8)(*mult), len(mult), enc.num_res_blocks, dec.z_channels,
                                 float(ae.scale_factor), float(ae.shift_factor))
        self.f, self.z, self.in_ch, self.out_ch = dec.ffactor, dec.z_channels, enc.in_channels, dec.out_ch
        self.h = C.c_void_p()
        hip._check(hip.lib().vc_vae_create(C.byref(self.cfg), C.byref(self.h)), "vc_vae_create")
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._io: Dict[tuple, tuple] = {}
        self._prepared = None
        self._side = None
        sd = ae.state_dict()
        names = self.weight_names()
        if [k for k in sd if k.endswith(".weight")] != [n + ".weight" for n in names]:
            raise hip.VclozeHipError("the module's state_dict keys differ from the weights libvcloze_hip.so expects for this configuration")
        with torch.cuda.device(self.dev):
            for n in names:
                self.bind(n, sd[n + ".weight"], sd[n + ".bias"])

    def bind(self, name: str, w: torch.Tensor, b: torch.Tensor, stream=None) -> None:
        """vc_vae_bind_weight: w / b as the checkpoint stores them (bf16 or f32, any device - moved to the handle's first)"""
        w, b = w.detach().to(self.dev).contiguous(), b.detach().to(self.dev).contiguous()
        if w.dtype not in (torch.bfloat16, torch.float32):
            w = w.float()
        b = b.to(w.dtype)
        shape = (C.c_int64 * w.dim())(*w.shape)
        hip._check(hip.lib().vc_vae_bind_weight(self.h, name.encode(), w.data_ptr(), b.data_ptr(), int(w.dtype == torch.float32), shape,
                                                w.dim(), stream if stream is not None else hip.cur_stream()), f"vc_vae_bind_weight({name})")
        self._io.clear()

    def plan_count(self) -> int:
        return hip.lib().vc_vae_plan_count(self.h)

    def workspace_bytes(self, H: int, W: int, which: int = hip.VAE_ENCODER | hip.VAE_DECODER) -> int:
        n = C.c_int64(0)
        hip._check(hip.lib().vc_vae_workspace_bytes(self.h, H, W, which, C.byref(n)), "vc_vae_workspace_bytes")
        return n.value

    def prepare(self, H: int, W: int, which: int = hip.VAE_ENCODER | hip.VAE_DECODER, stream=None) -> None:
        """vc_vae_prepare for a (H, W)-pixel image; the workspaces of the last four (size, halves) are kept (a two-stage pipeline alternates)"""
        key = (H, W, which)
        if self._prepared == key:
            return
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 4:              # two image sizes (a two-stage pipeline) x two halves
                self._ws.clear(); self._io.clear()
            ws = torch.empty(self.workspace_bytes(H, W, which) + 256, dtype=torch.uint8, device=self.dev)
            self._ws[key] = ws
        hip._check(hip.lib().vc_vae_prepare(self.h, H, W, which, *self._aligned(ws), stream), "vc_vae_prepare")
        self._prepared = key

    def _slot(self, key: tuple, shapes) -> tuple:
        """the persistent argument tensors of one (size, direction, form): a captured plan is keyed on their addresses"""
        io = self._io.get(key)
        if io is None:
            io = tuple(None if s is None else torch.empty(s[0], dtype=s[1], device=self.dev) for s in shapes)
            self._io[key] = io
        return io

    def decode(self, z: torch.Tensor, stream=0, pixels_f32: bool = False, which: int = hip.VAE_DECODER) -> torch.Tensor:
        """z [z_channels, h, w] bf16 / f32 -> pixels [out_ch, f h, f w] bf16 (or f32).  `which`: the halves the workspace of this
        size is prepared for - by default only the one the call needs (a decode-only user never allocates the encoder's maps).  stream: a hipStream_t value, 0 = torch's
        current stream (captured), None = the library's un-captured path on the default stream."""
        if z.dim() != 3 or z.shape[0] != self.z or z.dtype not in (torch.bfloat16, torch.float32):
            raise hip.VclozeHipError(f"VaeHandle.decode: [{self.z}, h, w] bf16 / f32 latent expected, got {z.dtype} {tuple(z.shape)}")
        h, w = z.shape[-2:]
        H, W = self.f * h, self.f * w
        pdt = torch.float32 if pixels_f32 else torch.bfloat16
        zin, px = self._slot((H, W, "dec", z.dtype, pdt), (((self.z, h, w), z.dtype), ((self.out_ch, H, W), pdt)))
        zin.copy_(z)
        s, cur = self._stream(stream)
        self.prepare(H, W, which, stream=s)
        form = hip.VAE_LATENT_F32 if z.dtype == torch.float32 else hip.VAE_LATENT_BF16
        hip._check(hip.lib().vc_vae_decode(self.h, zin.data_ptr(), form, 0, 0, px.data_ptr(), int(pixels_f32), s), "vc_vae_decode")
        self._join(stream, cur)
        return px.clone()

    def decode_tokens(self, tokens: torch.Tensor, h: int, w: int, col0: int = 0, stream=0, which: int = hip.VAE_DECODER) -> torch.Tensor:
        """tokens [(h/2)(w/2), >= col0 + 4 z] bf16 rows as the sampler leaves them -> pixels [out_ch, f h, f w] bf16"""
        hip._bf16(tokens, "tokens")
        if tokens.dim() != 2 or tokens.stride(1) != 1 or tokens.shape[0] != (h // 2) * (w // 2):
            raise hip.VclozeHipError("VaeHandle.decode_tokens: [(h/2)(w/2), cols] rows with contiguous columns expected")
        H, W = self.f * h, self.f * w
        tin, px = self._slot((H, W, "dect", tuple(tokens.shape)), ((tuple(tokens.shape), torch.bfloat16), ((self.out_ch, H, W), torch.bfloat16)))
        tin.copy_(tokens)
        s, cur = self._stream(stream)
        self.prepare(H, W, which, stream=s)
        hip._check(hip.lib().vc_vae_decode(self.h, tin.data_ptr(), hip.VAE_TOKENS, tin.stride(0), col0, px.data_ptr(), 0, s), "vc_vae_decode")
        self._join(stream, cur)
        return px.clone()

    def encode(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None, stream=0, tokens: Optional[torch.Tensor] = None, col0: int = 0,
               which: int = hip.VAE_ENCODER) -> torch.Tensor:
        """x [in_channels, H, W] bf16 / f32, noise [z_channels, H/f, W/f] bf16 or None (the mean) -> latent [z_channels, H/f, W/f]
        bf16; with `tokens` (bf16 rows [(h/2)(w/2), >= col0 + 4 z]) a copy of it whose columns col0.. hold the packed latent"""
        if x.dim() != 3 or x.shape[0] != self.in_ch or x.dtype not in (torch.bfloat16, torch.float32):
            raise hip.VclozeHipError(f"VaeHandle.encode: [{self.in_ch}, H, W] bf16 / f32 pixels expected, got {x.dtype} {tuple(x.shape)}")
        H, W = x.shape[-2:]
        h, w = H // self.f, W // self.f
        tshape = None if tokens is None else (tuple(tokens.shape), torch.bfloat16)
        xin, nin, out, tok = self._slot((H, W, "enc", x.dtype, noise is not None, tshape),
                                        (((self.in_ch, H, W), x.dtype), None if noise is None else ((self.z, h, w), torch.bfloat16),
                                         ((self.z, h, w), torch.bfloat16), tshape))
        xin.copy_(x)
        if noise is not None:
            nin.copy_(noise.reshape(self.z, h, w))
        if tokens is not None:
            tok.copy_(tokens)
        s, cur = self._stream(stream)
        self.prepare(H, W, which, stream=s)
        if tokens is not None:
            hip._check(hip.lib().vc_vae_encode(self.h, xin.data_ptr(), int(x.dtype == torch.float32), hip._p(nin), tok.data_ptr(), hip.VAE_TOKENS,
                                               tok.stride(0), col0, s), "vc_vae_encode")
            self._join(stream, cur)
            return tok.clone()
        hip._check(hip.lib().vc_vae_encode(self.h, xin.data_ptr(), int(x.dtype == torch.float32), hip._p(nin), out.data_ptr(),
                                           hip.VAE_LATENT_BF16, 0, 0, s), "vc_vae_encode")
        self._join(stream, cur)
        return out.clone()


class TextHandle(_Handle):
    """The text-encoder handle of include/vcloze_hip.h (vc_text_*) behind torch tensors: `T5EncoderModel.forward` /
    `CLIPTextModel.forward` as one C call, one hipGraph launch per prompt once the plan is captured.  The launch plan lives in
    csrc/text_engine.hip; the modules' own Python-ordered plan (text.py) is its parity twin (same kernels, same order, same bits).
    This class binds the module's bf16 parameters BY POINTER under their state_dict() keys (it keeps them alive; nothing is
    copied) and owns one workspace per sequence length.  The captured plan reads and writes workspace-resident buffers only, so ids
    go in and results come back as the caller's / fresh tensors."""
    _destroy, _weight_name = "vc_text_destroy", "vc_text_weight_name"

    def __init__(self, model, dev: Optional[torch.device] = None):
        from . import text
        c = model.cfg
        self.dev = torch.device(dev) if dev is not None else next(model.parameters()).device
        if isinstance(c, text.T5Config):
            self.cfg = hip.TextConfig(hip.TEXT_T5, c.vocab_size, c.d_model, c.d_kv, c.d_ff, c.num_layers, c.num_heads,
                                      c.relative_attention_num_buckets, c.relative_attention_max_distance, 0, 0, c.layer_norm_epsilon)
        else:
            self.cfg = hip.TextConfig(hip.TEXT_CLIP, c.vocab_size, c.hidden_size, c.hidden_size // c.num_attention_heads, c.intermediate_size,
                                      c.num_hidden_layers, c.num_attention_heads, 0, 0, c.max_position_embeddings, c.eos_token_id,
                                      c.layer_norm_eps)
        self.is_t5, self.D = self.cfg.kind == hip.TEXT_T5, self.cfg.d_model
        self.h = C.c_void_p()
        hip._check(hip.lib().vc_text_create(C.byref(self.cfg), C.byref(self.h)), "vc_text_create")
        self._ws: Dict[int, torch.Tensor] = {}
        self._prepared = None
        self._side = None
        self._bound: Dict[str, torch.Tensor] = {}
        sd = model.state_dict()
        names = self.weight_names()
        if list(sd) != names:
            raise hip.VclozeHipError("the module's state_dict keys differ from the tensors libvcloze_hip.so expects for this configuration")
        for n in names:
            self.bind(n, sd[n])

    def bind(self, key: str, t: torch.Tensor) -> None:
        """vc_text_bind_tensor: a bf16 tensor on the handle's device, bound by pointer and kept alive here"""
        t = t.detach()
        hip._bf16(t, key)
        if t.device != self.dev or not t.is_contiguous():
            raise hip.VclozeHipError(f"{key}: a contiguous tensor on {self.dev} expected")
        shape = (C.c_int64 * t.dim())(*t.shape)
        hip._check(hip.lib().vc_text_bind_tensor(self.h, key.encode(), t.data_ptr(), shape, t.dim()), f"vc_text_bind_tensor({key})")
        self._bound[key] = t

    def plan_count(self) -> int:
        return hip.lib().vc_text_plan_count(self.h)

    def workspace_bytes(self, L: int) -> int:
        n = C.c_int64(0)
        hip._check(hip.lib().vc_text_workspace_bytes(self.h, L, C.byref(n)), "vc_text_workspace_bytes")
        return n.value

    def prepare(self, L: int, stream=None) -> None:
        """vc_text_prepare for prompts of L ids; the workspaces of the last four lengths are kept"""
        if self._prepared == L:
            return
        ws = self._ws.get(L)
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.clear()
            ws = torch.empty(self.workspace_bytes(L) + 256, dtype=torch.uint8, device=self.dev)
            self._ws[L] = ws
        self._prepared = None
        hip._check(hip.lib().vc_text_prepare(self.h, L, *self._aligned(ws), stream), "vc_text_prepare")
        self._prepared = L

    def encode(self, ids: torch.Tensor, stream=0, want_hidden: bool = True, want_pooled: Optional[bool] = None):
        """ids [n, L] (any integer dtype) -> (hidden [n, L, D] bf16 or None, pooled [n, D] bf16 or None); pooled: CLIP only (its
        default there).  stream: a hipStream_t value, 0 = torch's current stream (captured), None = the library's un-captured path on
        the default stream."""
        if ids.dim() != 2 or ids.device != self.dev:
            raise hip.VclozeHipError(f"TextHandle.encode: ids [n, L] on {self.dev} expected, got {tuple(ids.shape)} on {ids.device}")
        want_pooled = (not self.is_t5) if want_pooled is None else want_pooled
        ids = ids.to(torch.int32).contiguous()
        n, L = ids.shape
        hidden = torch.empty(n, L, self.D, dtype=torch.bfloat16, device=self.dev) if want_hidden else None
        pooled = torch.empty(n, self.D, dtype=torch.bfloat16, device=self.dev) if want_pooled else None
        s, cur = self._stream(stream)
        self.prepare(L, stream=s)
        hip._check(hip.lib().vc_text_encode(self.h, ids.data_ptr(), n, hip._p(hidden), hip._p(pooled), s), "vc_text_encode")
        self._join(stream, cur)
        if cur is not None:              # the plan ran on another stream: its tensors must outlive that stream's work
            for t in (ids, hidden, pooled):
                if t is not None:
                    t.record_stream(cur)
        return hidden, pooled


class GridHandle(_Handle):
    """The grid handle of include/vcloze_hip.h (vc_grid_*) behind torch tensors: one grid - pixels and token ids in, pixels out - as
    ONE C call (`generate`), and the SDEdit upsampling of K cells as one more (`sdedit`).  The composition lives in
    csrc/grid_engine.hip; `pipeline.generate_grid` / `pipeline.upsample_images` with a `NoiseStream` and the three sub-handles on are
    its parity twin (same kernels, same operands, same bits).  It borrows the C handles of `model.handle()`, `ae.handle()`,
    `t5.handle()` and `clip.handle()` (it keeps those wrappers, and with them the bound weights, alive), owns ONE workspace that only ever grows - kept between calls, so
    a second job of the same geometry finds every captured plan again - and, because the C call prepares the sub-handles inside that
    workspace, tells their Python wrappers to prepare again before their next direct use."""
    _destroy = "vc_grid_destroy"

    def __init__(self, model, ae, t5, clip):
        self.flux, self.vae, self.t5, self.clip = model.handle(), ae.handle(), t5.handle(), clip.handle()
        if self.flux is None:
            raise hip.VclozeHipError("GridHandle needs the Flux C handle (use_handle True; with lora_mode 'ref': ref_plan 'handle')")
        self.dev = self.flux.dev
        self.h = C.c_void_p()
        cfg = hip.GridConfig(self.flux.h.value, self.vae.h.value, self.t5.h.value, self.clip.h.value)
        hip._check(hip.lib().vc_grid_create(C.byref(cfg), C.byref(self.h)), "vc_grid_create")
        self._ws: Optional[torch.Tensor] = None
        self._side = None

    def set_noise(self, source="own", sm_count: int = 0, threads_per_sm: int = 0) -> None:
        """vc_grid_set_noise: "own" (the default) - `seed` / `noise_offset` of every job are the library's stream (`pipeline.NoiseStream`);
        "torch" - they are a torch generator's seed and Philox offset, every draw is torch's (`pipeline.TorchNoiseStream`).
        sm_count / threads_per_sm: another device's properties, 0 = this device's."""
        src = {"own": hip.NOISE_OWN, "torch": hip.NOISE_TORCH}.get(source, source)
        hip._check(hip.lib().vc_grid_set_noise(self.h, int(src), int(sm_count), int(threads_per_sm)), "vc_grid_set_noise")

    def _workspace(self, need: int) -> Tuple[int, int]:
        if self._ws is None or self._aligned(self._ws)[1] < need:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.dev)
        return self._aligned(self._ws)

    @staticmethod
    def _ids(ids: torch.Tensor, name: str) -> np.ndarray:
        if ids.dim() == 2 and ids.shape[0] == 1:
            ids = ids[0]
        if ids.dim() != 1:
            raise hip.VclozeHipError(f"GridHandle: {name} [1, L] or [L] expected, got {tuple(ids.shape)}")
        return np.ascontiguousarray(ids.detach().to("cpu", torch.int32).numpy())

    def _pixels(self, imgs: Sequence[torch.Tensor]) -> list:
        out = []
        for t in imgs:
            if t.dim() != 3 or t.shape[0] != 3 or t.device != self.dev:
                raise hip.VclozeHipError(f"GridHandle: [3, H, W] pixels on {self.dev} expected, got {tuple(t.shape)} on {t.device}")
            out.append(t.to(torch.bfloat16).contiguous())      # as pipeline.generate_grid hands them to the encoder
        return out

    def _run(self, call, what, job, bytes_fn, shapes, uint8, stream):
        """size the workspace, allocate the outputs, run `call` on the plan's stream; returns (outputs, stream position after)"""
        need = C.c_int64(0)
        hip._check(bytes_fn(self.h, C.byref(job), C.byref(need)), what + "_workspace_bytes")
        base, nbytes = self._workspace(need.value)
        outs = [None if s is None else torch.empty((s[1], s[2], 3) if uint8 else s, dtype=torch.uint8 if uint8 else torch.float32, device=self.dev)
                for s in shapes]
        ptrs = (C.c_void_p * len(outs))(*[None if o is None else o.data_ptr() for o in outs])
        after = C.c_uint64(0)
        job.noise_offset_out = C.pointer(after)
        s, cur = self._stream(stream)
        try:
            hip._check(call(self.h, C.byref(job), base, nbytes, ptrs, s), what)
        finally:
            # the sub-handles are now prepared inside this handle's workspace: their wrappers must not trust what they remember
            self.vae._prepared = self.t5._prepared = self.clip._prepared = None
            self.flux.geom = None
            self._join(stream, cur)
        if cur is not None:
            for o in outs:
                if o is not None:
                    o.record_stream(cur)
        return [o for o in outs if o is not None], after.value

    def generate(self, row_images: Sequence[torch.Tensor], row_masks: Sequence[torch.Tensor], t5_ids: torch.Tensor, clip_ids: torch.Tensor,
                 seed: int, noise_offset: int = 0, cfg: float = 30.0, steps: int = 30, solver="euler", time_shifting_factor=1,
                 decode_rows: Optional[Sequence[int]] = None, uint8: bool = False, max_evals: int = 0, stream=0):
        """vc_grid_generate: row_images[i] [3, H, W_row] in [-1, 1], row_masks[i] [..., H, W_row] (1 = generate), ids [1, L]; the
        noise comes from the library's stream of `seed` from `noise_offset` on.  Returns (the rows `decode_rows` (default: all, in
        row order) as f32 [3, H, W_row] in [0, 1] - or with `uint8` as [H, W_row, 3] bytes -, the stream position after the last draw)."""
        R = len(row_images)
        if not 1 <= R <= hip.GRID_MAX_ROWS or len(row_masks) != R:
            raise hip.VclozeHipError(f"GridHandle.generate: 1..{hip.GRID_MAX_ROWS} rows with one mask each expected, got {R} / {len(row_masks)}")
        px = self._pixels(row_images)
        masks = []
        for m, p in zip(row_masks, px):
            m = m.reshape(m.shape[-2], m.shape[-1]).to(self.dev, torch.bfloat16).contiguous()
            if m.shape != p.shape[-2:]:
                raise hip.VclozeHipError(f"GridHandle.generate: mask {tuple(m.shape)} for a row of {tuple(p.shape[-2:])} pixels")
            masks.append(m.clone() if m.data_ptr() % 16 else m)
        want = set(range(R)) if decode_rows is None else {int(i) for i in decode_rows}
        if not want <= set(range(R)):
            raise hip.VclozeHipError(f"GridHandle.generate: decode_rows {sorted(want)} outside the {R} rows")
        t5a, clipa = self._ids(t5_ids, "t5_ids"), self._ids(clip_ids, "clip_ids")
        job = hip.GridJob()
        job.rows, job.pixels_is_f32 = R, 0
        for i in range(R):
            job.height[i], job.width[i] = px[i].shape[-2:]
            job.pixels[i], job.masks[i], job.decode[i] = px[i].data_ptr(), masks[i].data_ptr(), int(i in want)
        job.t5_ids, job.clip_ids, job.t5_len, job.clip_len = _ip(t5a), _ip(clipa), t5a.size, clipa.size
        job.seed, job.noise_offset = hip._u64(seed, "seed"), hip._u64(noise_offset, "noise_offset")
        job.guidance, job.n_points, job.method = float(cfg), int(steps), FluxHandle._method(solver)
        job.out_form, job.max_evals = hip.PIXELS_U8 if uint8 else hip.PIXELS_F32, int(max_evals)
        job.time_shifting_factor = float(time_shifting_factor or 0.0)
        shapes = [tuple(px[i].shape) if i in want else None for i in range(R)]
        L = hip.lib()
        outs, after = self._run(L.vc_grid_generate, "vc_grid_generate", job, L.vc_grid_workspace_bytes, shapes, uint8, stream)
        if decode_rows is not None:             # in the caller's order, as pipeline.generate_grid returns them
            by_row = dict(zip(sorted(want), outs))
            outs = [by_row[int(i)] for i in decode_rows]
        return outs, after

    def sdedit(self, images: Sequence[torch.Tensor], t5_ids: torch.Tensor, clip_ids: torch.Tensor, seed: int, noise_offset: int = 0,
               cfg: float = 30.0, steps: int = 10, strength: float = 0.4, solver="euler", uint8: bool = False, max_evals: int = 0, stream=0):
        """vc_grid_sdedit: K images [3, H, W] in [-1, 1] of ONE size, already at their final size, refined together from `strength`
        under the content prompt.  Returns (K images, f32 [3, H, W] in [0, 1] or `uint8` [H, W, 3], the stream position after)."""
        K = len(images)
        if not 1 <= K <= hip.GRID_MAX_ROWS:
            raise hip.VclozeHipError(f"GridHandle.sdedit: 1..{hip.GRID_MAX_ROWS} images expected, got {K}")
        px = self._pixels(images)
        if any(p.shape != px[0].shape for p in px):
            raise hip.VclozeHipError("GridHandle.sdedit: all targets must share one size")
        t5a, clipa = self._ids(t5_ids, "t5_ids"), self._ids(clip_ids, "clip_ids")
        job = hip.GridSdedit()
        job.count, job.pixels_is_f32 = K, 0
        job.height, job.width = px[0].shape[-2:]
        for k in range(K):
            job.pixels[k] = px[k].data_ptr()
        job.t5_ids, job.clip_ids, job.t5_len, job.clip_len = _ip(t5a), _ip(clipa), t5a.size, clipa.size
        job.seed, job.noise_offset = hip._u64(seed, "seed"), hip._u64(noise_offset, "noise_offset")
        job.guidance, job.n_points, job.method = float(cfg), int(steps), FluxHandle._method(solver)
        job.out_form, job.max_evals, job.strength = hip.PIXELS_U8 if uint8 else hip.PIXELS_F32, int(max_evals), float(strength)
        L = hip.lib()
        return self._run(L.vc_grid_sdedit, "vc_grid_sdedit", job, L.vc_grid_sdedit_workspace_bytes, [tuple(p.shape) for p in px], uint8, stream)

    @staticmethod
    def _u8(t: torch.Tensor, dev, what: str) -> torch.Tensor:
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or t.device != dev:
            raise hip.VclozeHipError(f"GridHandle.{what}: [H, W, 3] uint8 images on {dev} expected, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.contiguous()

    def generate_photos(self, images: Sequence[Sequence[Optional[torch.Tensor]]], resolution: int, t5_ids: torch.Tensor, clip_ids: torch.Tensor,
                        seed: int, noise_offset: int = 0, cfg: float = 30.0, steps: int = 30, solver="euler", time_shifting_factor=1,
                        decode_rows: Optional[Sequence[int]] = None, uint8: bool = False, max_evals: int = 0, stream=0):
        """vc_grid_generate_photos: images[i][j] the photograph of row i, column j as a device uint8 [H, W, 3] tensor, or None where it
        is absent (last row only: the cell to generate).  The layout rule, the LANCZOS / bicubic resamples, the centre crop,
        ToTensor / Normalize and the masks run on the device, then `generate`'s path.  Returns what `generate` returns."""
        R = len(images)
        gw = len(images[0]) if R else 0
        if not 1 <= R <= hip.GRID_MAX_ROWS or not 1 <= gw <= hip.GRID_MAX_ROWS or any(len(r) != gw for r in images):
            raise hip.VclozeHipError(f"GridHandle.generate_photos: 1..{hip.GRID_MAX_ROWS} rows of equally many cells expected")
        flat = [None if t is None else self._u8(t, self.dev, "generate_photos") for r in images for t in r]
        plans = hip.grid_layout([[None if t is None else (t.shape[1], t.shape[0]) for t in r] for r in images], resolution)
        want = set(range(R)) if decode_rows is None else {int(i) for i in decode_rows}
        if not want <= set(range(R)):
            raise hip.VclozeHipError(f"GridHandle.generate_photos: decode_rows {sorted(want)} outside the {R} rows")
        t5a, clipa = self._ids(t5_ids, "t5_ids"), self._ids(clip_ids, "clip_ids")
        n = R * gw
        ptrs = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in flat])
        ws = (C.c_int32 * n)(*[0 if t is None else t.shape[1] for t in flat])
        hs = (C.c_int32 * n)(*[0 if t is None else t.shape[0] for t in flat])
        job = hip.GridPhotos()
        job.grid_h, job.grid_w, job.resolution = R, gw, int(resolution)
        job.images, job.width, job.height = ptrs, ws, hs
        for i in range(R):
            job.decode[i] = int(i in want)
        job.t5_ids, job.clip_ids, job.t5_len, job.clip_len = _ip(t5a), _ip(clipa), t5a.size, clipa.size
        job.seed, job.noise_offset = hip._u64(seed, "seed"), hip._u64(noise_offset, "noise_offset")
        job.guidance, job.n_points, job.method = float(cfg), int(steps), FluxHandle._method(solver)
        job.out_form, job.max_evals = hip.PIXELS_U8 if uint8 else hip.PIXELS_F32, int(max_evals)
        job.time_shifting_factor = float(time_shifting_factor or 0.0)
        shapes = [(3, plans[i][0].final_h, sum(c.final_w for c in plans[i])) if i in want else None for i in range(R)]
        L = hip.lib()
        outs, after = self._run(L.vc_grid_generate_photos, "vc_grid_generate_photos", job, L.vc_grid_photos_workspace_bytes, shapes, uint8, stream)
        if decode_rows is not None:
            by_row = dict(zip(sorted(want), outs))
            outs = [by_row[int(i)] for i in decode_rows]
        return outs, after

    def sdedit_u8(self, cells: Sequence[torch.Tensor], size, t5_ids: torch.Tensor, clip_ids: torch.Tensor, seed: int, noise_offset: int = 0,
                  cfg: float = 30.0, steps: int = 10, strength: float = 0.4, solver="euler", uint8: bool = False, max_evals: int = 0, stream=0):
        """vc_grid_sdedit_u8: K device uint8 cells [h, w, 3] of ONE size - what `hip.pixels_out(..., uint8=True)` writes - resized
        (bicubic, Pillow's bytes) to size = (w, h) = `hip.upsampling_size(...)` on the device, then `sdedit`'s path.  strength >= 1
        returns the resized uint8 images (needs `uint8`).  Returns what `sdedit` returns."""
        K = len(cells)
        if not 1 <= K <= hip.GRID_MAX_ROWS:
            raise hip.VclozeHipError(f"GridHandle.sdedit_u8: 1..{hip.GRID_MAX_ROWS} cells expected, got {K}")
        px = [self._u8(t, self.dev, "sdedit_u8") for t in cells]
        if any(p.shape != px[0].shape for p in px):
            raise hip.VclozeHipError("GridHandle.sdedit_u8: all cells must share one size")
        t5a, clipa = self._ids(t5_ids, "t5_ids"), self._ids(clip_ids, "clip_ids")
        job = hip.GridSdeditU8()
        job.count, job.cell_h, job.cell_w = K, px[0].shape[0], px[0].shape[1]
        job.width, job.height = int(size[0]), int(size[1])
        for k in range(K):
            job.pixels[k] = px[k].data_ptr()
        job.t5_ids, job.clip_ids, job.t5_len, job.clip_len = _ip(t5a), _ip(clipa), t5a.size, clipa.size
        job.seed, job.noise_offset = hip._u64(seed, "seed"), hip._u64(noise_offset, "noise_offset")
        job.guidance, job.n_points, job.method = float(cfg), int(steps), FluxHandle._method(solver)
        job.out_form, job.max_evals, job.strength = hip.PIXELS_U8 if uint8 else hip.PIXELS_F32, int(max_evals), float(strength)
        L = hip.lib()
        return self._run(L.vc_grid_sdedit_u8, "vc_grid_sdedit_u8", job, L.vc_grid_sdedit_u8_workspace_bytes,
                         [(3, job.height, job.width)] * K, uint8, stream)
