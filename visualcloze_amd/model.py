"""Host-side mirror of the reference's model interface for the denoising path.

`Flux`, `FluxLoraWrapper` and `FluxParams` keep the reference's constructor, `state_dict` key/shape contract
and `forward` keyword surface (models/model.py:18-175), so `visualcloze.py` /
`sample.py` can construct, `.to()`, `load_state_dict(strict=False)` and call `model.forward` unchanged.
The modules below are PARAMETER HOLDERS: every FLOP of `forward` runs in libvcloze_hip.so via
`FluxEngine`.  There is no torch fallback — without a GPU or without the library, forward raises.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch import Tensor, nn

from . import hip
from .engine import FluxEngine, PreparedWeights


@dataclass
class FluxParams:
    in_channels: int
    out_channels: int
    vec_in_dim: int
    context_in_dim: int
    hidden_size: int
    mlp_ratio: float
    num_heads: int
    depth: int
    depth_single_blocks: int
    axes_dim: list
    theta: int
    qkv_bias: bool
    guidance_embed: bool


# "flux-dev-fill-lora" hyper-parameters (models/util.py:132-165)
FLUX_DEV_FILL = dict(in_channels=384, out_channels=64, vec_in_dim=768, context_in_dim=4096, hidden_size=3072,
                     mlp_ratio=4.0, num_heads=24, depth=19, depth_single_blocks=38, axes_dim=[16, 56, 56],
                     theta=10_000, qkv_bias=True, guidance_embed=True)


class _NoTorchForward(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise hip.VclozeHipError(f"{type(self).__name__} is a parameter holder; the denoising path runs in "
                                 "libvcloze_hip.so through Flux.forward (no torch fallback)")


class Linear(_NoTorchForward):
    """nn.Linear-shaped holder (`weight [out,in]`, `bias [out]`); LoRA factors are added by `add_lora`."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        self.scale = 1.0
        self.rank = 0
        bound = 1 / math.sqrt(in_features)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    def add_lora(self, max_rank: int, scale: float) -> None:
        """LinearLora.__init__ (models/modules/lora.py:34-90): rank clipped to min(in,out), lora_B has a bias,
        lora_B initialised to zero."""
        assert isinstance(scale, float), "scale must be a float"
        self.rank = min(max_rank, self.in_features, self.out_features)
        self.scale = scale
        self.lora_A = Linear(self.in_features, self.rank, bias=False)
        self.lora_B = Linear(self.rank, self.out_features, bias=True)
        with torch.no_grad():
            self.lora_A.to(self.weight.device, self.weight.dtype)
            self.lora_B.to(self.weight.device, self.weight.dtype)
            self.lora_B.weight.zero_()
            self.lora_B.bias.zero_()

    def set_scale(self, scale: float) -> None:
        assert isinstance(scale, float), "scalar value must be a float"
        self.scale = scale


class MLPEmbedder(_NoTorchForward):
    def __init__(self, in_dim: int, hidden_dim: int):
        super().__init__()
        self.in_layer = Linear(in_dim, hidden_dim)
        self.out_layer = Linear(hidden_dim, hidden_dim)


class RMSNorm(_NoTorchForward):
    def __init__(self, dim: int):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(dim))


class QKNorm(_NoTorchForward):
    def __init__(self, dim: int):
        super().__init__()
        self.query_norm, self.key_norm = RMSNorm(dim), RMSNorm(dim)


class SelfAttention(_NoTorchForward):
    def __init__(self, dim: int, num_heads: int, qkv_bias: bool):
        super().__init__()
        self.qkv = Linear(dim, dim * 3, bias=qkv_bias)
        self.norm = QKNorm(dim // num_heads)
        self.proj = Linear(dim, dim)


class Modulation(_NoTorchForward):
    def __init__(self, dim: int, double: bool):
        super().__init__()
        self.is_double = double
        self.multiplier = 6 if double else 3
        self.lin = Linear(dim, self.multiplier * dim)


class _Seq(nn.Sequential, _NoTorchForward):
    pass


class _Empty(_NoTorchForward):
    """stands in for parameter-free members (nn.GELU / nn.SiLU / LayerNorm without affine) to keep indices"""


class DoubleStreamBlock(_NoTorchForward):
    def __init__(self, hidden_size: int, num_heads: int, mlp_ratio: float, qkv_bias: bool = False):
        super().__init__()
        mlp = int(hidden_size * mlp_ratio)
        self.img_mod = Modulation(hidden_size, True)
        self.img_attn = SelfAttention(hidden_size, num_heads, qkv_bias)
        self.img_mlp = _Seq(Linear(hidden_size, mlp), _Empty(), Linear(mlp, hidden_size))
        self.txt_mod = Modulation(hidden_size, True)
        self.txt_attn = SelfAttention(hidden_size, num_heads, qkv_bias)
        self.txt_mlp = _Seq(Linear(hidden_size, mlp), _Empty(), Linear(mlp, hidden_size))


class SingleStreamBlock(_NoTorchForward):
    def __init__(self, hidden_size: int, num_heads: int, mlp_ratio: float = 4.0):
        super().__init__()
        self.mlp_hidden_dim = int(hidden_size * mlp_ratio)
        self.linear1 = Linear(hidden_size, hidden_size * 3 + self.mlp_hidden_dim)
        self.linear2 = Linear(hidden_size + self.mlp_hidden_dim, hidden_size)
        self.norm = QKNorm(hidden_size // num_heads)
        self.modulation = Modulation(hidden_size, False)


class LastLayer(_NoTorchForward):
    def __init__(self, hidden_size: int, patch_size: int, out_channels: int):
        super().__init__()
        self.linear = Linear(hidden_size, patch_size * patch_size * out_channels)
        self.adaLN_modulation = _Seq(_Empty(), Linear(hidden_size, 2 * hidden_size))


class MaskLayout:
    """How (txt_mask, img_mask) map onto the kernels' masks.  flash-attn's varlen path (math.py:9-60) drops masked rows
    of the joint sequence wherever they are; attention does not care about key order (RoPE travels with the row), every
    other op of Flux.forward is per-row, so each stream's rows are reordered VALID FIRST (stable), which leaves
        [txt valid | txt masked | img valid | img masked]
    = a prefix length kv_len = T + n_img plus one masked gap (n_txt, T) per sample, and the result rows are scattered
    back.  `sl` selects the samples of a chunk: a slice, or a list of sample indices (the pairs of a true-CFG trajectory,
    transport._sample_fused).  Right-padded masks (all the reference's callers build, sampling.py:41-46,68-70,98) are the identity case."""

    def __init__(self, txt_mask, img_mask, B: int, T: int, N: int):
        self.B, self.T, self.N = B, T, N
        self.perm_t = self.perm_i = self.inv_i = self.inv_t = None
        if txt_mask is None or img_mask is None:
            self.n_txt, self.n_img = [T] * B, [N] * B
            return
        tm = txt_mask.reshape(B, T).to("cpu") != 0
        im = img_mask.reshape(B, N).to("cpu") != 0
        self.n_txt = [int(v) for v in tm.sum(1)]
        self.n_img = [int(v) for v in im.sum(1)]
        pt = torch.sort((~tm).to(torch.uint8), dim=1, stable=True).indices
        pi = torch.sort((~im).to(torch.uint8), dim=1, stable=True).indices
        if not torch.equal(pt, torch.arange(T).expand(B, T)):
            self.perm_t = pt
            self.inv_t = torch.argsort(pt, dim=1)
        if not torch.equal(pi, torch.arange(N).expand(B, N)):
            self.perm_i = pi
            self.inv_i = torch.argsort(pi, dim=1)

    @staticmethod
    def _pick(values: list, sl) -> list:
        return values[sl] if isinstance(sl, slice) else [values[i] for i in sl]

    def kv_len(self, sl) -> List[int]:
        return [self.T + n for n in self._pick(self.n_img, sl)]

    def kv_gap(self, sl):
        gaps = [(n, self.T) if n < self.T else (0, 0) for n in self._pick(self.n_txt, sl)]
        return gaps if any(hi > lo for lo, hi in gaps) else None

    @staticmethod
    def _take(x: Tensor, perm, sl) -> Tensor:
        x = x[sl]
        if perm is None:
            return x
        idx = perm[sl].to(x.device)
        return torch.gather(x, 1, idx.reshape(idx.shape + (1,) * (x.dim() - 2)).expand(x.shape))

    def txt_rows(self, x: Tensor, sl) -> Tensor:
        """rows of a [B, T, ...] text-stream tensor (txt, txt_ids) in kernel order"""
        return self._take(x, self.perm_t, sl)

    def img_rows(self, x: Tensor, sl) -> Tensor:
        """rows of a [B, N, ...] image-stream tensor (img / x, cond, img_ids) in kernel order"""
        return self._take(x, self.perm_i, sl)

    def img_rows_back(self, x: Tensor, sl) -> Tensor:
        """kernel-order [bs, N, ...] image-stream rows back in the caller's order"""
        return self._back(x, self.inv_i, sl)

    def txt_rows_back(self, x: Tensor, sl) -> Tensor:
        """kernel-order [bs, T, ...] text-stream rows back in the caller's order (per-block taps)"""
        return self._back(x, self.inv_t, sl)

    @staticmethod
    def _back(x: Tensor, inv, sl) -> Tensor:
        if inv is None:
            return x
        idx = inv[sl].to(x.device)
        return torch.gather(x, 1, idx.reshape(idx.shape + (1,) * (x.dim() - 2)).expand(x.shape))


def per_sample(v: Optional[Tensor], B: int) -> Optional[Tensor]:
    """A per-sample vector [B]; a single value (the pipeline's `guidance = torch.full((1,), cfg)`, visualcloze.py:413)
    broadcasts over the batch as it does in the reference's `vec + guidance_in(...)`."""
    if v is None:
        return None
    v = v.reshape(-1)
    if v.numel() == 1 and B > 1:
        v = v.expand(B)
    if v.numel() != B:
        raise ValueError(f"expected 1 or {B} per-sample values, got {v.numel()}")
    return v


class ChunkPlan:
    """How one call's batch becomes chunks of handle calls - written down once, for Flux.forward, Flux.block_taps and the fused
    solves of transport.py.  Built per call from the caller's tensors: checks them, broadcasts the guidance, lays the masks out
    (`lay`) and cuts the B samples into `chunks` of at most `max_batch`: slices, or with `pairs` (true CFG) `transport.cfg_chunks`'
    index lists.  `channels`: (of the state x, of cond) where x || cond feeds img_in.  Plain arguments only: no GPU needed."""

    def __init__(self, B: int, N: int, txt, y, guidance, img_ids, txt_ids, txt_mask, img_mask, params: FluxParams,
                 dev: torch.device, max_batch: int, pairs: bool = False, channels=None):
        if channels is not None and sum(channels) != params.in_channels:
            raise hip.VclozeHipError(f"x ({channels[0]}) || cond ({channels[1]}) does not match in_channels {params.in_channels}")
        if params.guidance_embed and guidance is None:
            raise ValueError("Didn't get guidance strength for guidance distilled model.")
        self.B, self.N, self.T, self.dev = B, N, txt.shape[1], dev
        self.txt, self.y, self.img_ids, self.txt_ids = txt, y, img_ids, txt_ids
        self.gbf16 = guidance is not None and guidance.dtype == torch.bfloat16
        self.guidance = per_sample(guidance, B)
        self.lay = MaskLayout(txt_mask, img_mask, B, self.T, N)
        self.img_back, self.txt_back = self.lay.img_rows_back, self.lay.txt_rows_back      # (kernel-order rows, sl) -> the caller's order
        if pairs:
            from .transport import cfg_chunks
            self.chunks = cfg_chunks(B, max_batch)
        else:                                          # samples of a chunk run as ONE stacked launch sequence
            self.chunks = [slice(b0, min(b0 + max_batch, B)) for b0 in range(0, B, max_batch)]

    def size(self, sl) -> int:
        return len(range(self.B)[sl]) if isinstance(sl, slice) else len(sl)

    def _inputs(self, sl) -> tuple:
        # the ids and the guidance stay views of the caller's storage (`MaskLayout._take`): handle._HostCopies keys on that memory
        bf = lambda t: t.to(self.dev, torch.bfloat16).contiguous()  # noqa: E731
        return (bf(self.lay.txt_rows(self.txt, sl)), bf(self.y[sl]), None if self.guidance is None else self.guidance[sl], self.gbf16,
                self.lay.img_rows(self.img_ids, sl), self.lay.txt_rows(self.txt_ids, sl))

    def prepare_args(self, sl, max_evals: int) -> tuple:
        """the positional arguments of `FluxHandle.prepare` for a chunk: h.prepare(*plan.prepare_args(sl, n), stream=s)"""
        return self._inputs(sl) + (max_evals, self.lay.kv_len(sl), self.lay.kv_gap(sl))

    def twin_prepare_args(self, sl, timesteps):
        """(args behind the workspace, kwargs) of the Python-ordered twin's `FluxEngine.prepare_sample`: the same tensors"""
        return self._inputs(sl) + (timesteps, self.lay.kv_len(sl)), dict(kv_gap=self.lay.kv_gap(sl))

    def img_rows(self, x: Tensor, sl, dtype, copy: bool = False) -> Tensor:
        """kernel-order rows of a chunk of a [B, N, ...] image-stream tensor, contiguous on the device; `copy`: never x's memory"""
        return self.lay.img_rows(x, sl).to(self.dev, dtype, copy=copy).contiguous()

    def joint_back(self, o: Tensor, sl) -> Tensor:
        """a chunk of the joint stream [bs, T + N, ...] (text rows, then image rows: the SingleStream taps) in the caller's order"""
        return torch.cat((self.txt_back(o[:, :self.T], sl), self.img_back(o[:, self.T:], sl)), dim=1)


class Flux(nn.Module):
    """Drop-in for models/model.py:35-151 (inference surface)."""

    def __init__(self, params: FluxParams):
        super().__init__()
        self.params = params
        self.in_channels, self.out_channels = params.in_channels, params.out_channels
        if params.hidden_size % params.num_heads != 0:
            raise ValueError(f"Hidden size {params.hidden_size} must be divisible by num_heads {params.num_heads}")
        pe_dim = params.hidden_size // params.num_heads
        if sum(params.axes_dim) != pe_dim:
            raise ValueError(f"Got {params.axes_dim} but expected positional dim {pe_dim}")
        if pe_dim != 128:
            raise ValueError("the gfx950 attention kernel is specialised for head_dim 128 (FLUX)")
        self.hidden_size, self.num_heads = params.hidden_size, params.num_heads
        self.img_in = Linear(self.in_channels, self.hidden_size)
        self.time_in = MLPEmbedder(256, self.hidden_size)
        self.vector_in = MLPEmbedder(params.vec_in_dim, self.hidden_size)
        self.guidance_in = MLPEmbedder(256, self.hidden_size) if params.guidance_embed else nn.Identity()
        self.txt_in = Linear(params.context_in_dim, self.hidden_size)
        self.double_blocks = nn.ModuleList(
            [DoubleStreamBlock(self.hidden_size, self.num_heads, params.mlp_ratio, params.qkv_bias)
             for _ in range(params.depth)])
        self.single_blocks = nn.ModuleList(
            [SingleStreamBlock(self.hidden_size, self.num_heads, params.mlp_ratio)
             for _ in range(params.depth_single_blocks)])
        self.final_layer = LastLayer(self.hidden_size, 1, self.out_channels)
        self._engine: Optional[FluxEngine] = None
        self._handle = None
        self._fingerprint = None
        # True: Flux.forward and the fused sampler run through the C handle API (vc_flux_*, csrc/flux_engine.hip), one
        # call per evaluation / per trajectory.  False (or lora_mode "ref"): the same launch plan ordered from Python
        # (engine.FluxEngine) over the op-level ABI - bit-identical results, kept for the parity mode and per-block taps.
        self.use_handle = True
        self.last_step_cache_stats = None      # of the last trajectory sampled with a transport.StepCache: one dict per chunk
        # the numerics monitor of the C handle (vc_flux_set_monitor): 0 = off, 1 = per evaluation the statistics of the model's output
        # "v" and of the state "x", 2 = those and every residual stream.  Handle-only: with the Python-ordered plan a non-zero value
        # raises ValueError.  After a fused solve or a forward last_monitor_log holds one `FluxHandle.monitor_log()` dict per chunk
        # of samples, last_monitor_report the first bad (chunk, evaluation, site, sample of the chunk) or None; with monitor_strict
        # both raise FloatingPointError on one.  0 leaves the handle's monitor alone (a caller may have set it on `handle()` itself).
        self.monitor = 0
        self.monitor_strict = False
        self.last_monitor_log = None
        self.last_monitor_report = None
        # "merged": W + s*B@A folded once (the product mode).  "ref": LinearLora.forward executed as the
        # reference does - base GEMM, two skinny GEMMs, three bf16 roundings (models/modules/lora.py:92-98) - so that
        # the merge's one-rounding deviation is a choice, not a necessity; slower (+8 % FLOPs, unfused epilogues).
        self.lora_mode = "merged"
        # who runs lora_mode "ref": "python" = the Python-ordered plan (engine.FluxEngine: one sample per launch sequence, Euler on a
        # bf16 state only), "handle" = the C handle's un-merged mode (vc_flux_bind_lora, option lora_mode 1: the same launches in the
        # same order, and with them batches, f32 states, midpoint / rk4, true CFG, the step cache and a runtime lora scale)
        self.ref_plan = "python"
        # the prepared qkv weights (merged mode) are stored HEAD-PERMUTED - every key head inside one 192-column GEMM tile -
        # so that QKNorm + RoPE of k can ride the projection's epilogue (hip.qkv_head_permutation, VcGemmProblem.kn_heads)
        self.qkv_permute = True
        # who forms W + s*B@A in prepare(): "torch" (an f32 matmul of the vendor BLAS plus f32 temporaries, the path every parity
        # number of DESIGN.md was taken on) or "hip" (vc_lora_merge, csrc/lora_merge.hip: one launch per Linear, no f32 copy, no
        # vendor GEMM; the same arithmetic up to the order of the f32 sums)
        self.lora_merge = "torch"
        # True (opt-in): the C handle prepares the weights ITSELF from this module's state_dict (handle.FluxHandle.from_state_dict:
        # vc_flux_load_*, csrc/flux_load.hip) - merged mode only, no torch arithmetic on a weight, no Python-ordered twin: engine()
        # and lora_mode "ref" with ref_plan "python" raise.  False: prepare() as it always was.
        self.load_in_library = False

    # ------------------------------------------------------------------ weights -> engine
    def _linears(self):
        for name, m in self.named_modules():
            if isinstance(m, Linear) and ".lora_" not in name:
                yield name, m

    def _weights_fingerprint(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters()) + tuple(
            m.scale for _, m in self._linears()) + (self.lora_mode, self.qkv_permute, self.lora_merge)

    def _check_ref_plan(self) -> None:
        if self.ref_plan not in ("python", "handle"):
            raise ValueError(f"ref_plan must be 'python' or 'handle', got {self.ref_plan!r}")

    def set_lora_scale(self, scale: float) -> None:
        """models/model.py:172-175.  With lora_mode "ref" on the C handle (ref_plan "handle") a prepared model takes the new scale
        at run time - vc_flux_set_lora_scale: no re-preparation of the weights, captured steps stay, the next forward's vc_flux_prepare fills it in - and, as that mode promises the
        reference's roundings, refuses a scale that is no bf16 value.  Otherwise the next forward re-prepares (merged mode: re-merges)."""
        assert isinstance(scale, float), "scalar value must be a float"
        self._check_ref_plan()
        live = (self.lora_mode == "ref" and self.ref_plan == "handle" and self._handle is not None and self._engine is not None
                and self._handle.W is self._engine.W and self._fingerprint == self._weights_fingerprint())
        if live:
            self._handle.set_lora_scale(scale)            # raises for a scale bf16 cannot hold, before anything changes
            for R in self._engine.W.ref.values():         # the twin's operands say the same
                if R.scale is not None:
                    R.scale.fill_(scale)
        for _, m in self._linears():
            m.set_scale(scale=scale)
        if live:
            self._fingerprint = self._weights_fingerprint()

    @staticmethod
    @torch.no_grad()
    def merged_linear(m: "Linear", consume: bool = False, out: Optional[Tensor] = None, backend: str = "torch"):
        """(W', b') of one Linear as the engine executes it: bf16(W + s*B@A), bf16(b + s*b_B) - LinearLora
        (models/modules/lora.py:92-98) with its LoRA pair folded in, exact in f32 and rounded to bf16 once.
        `out`: write W' into this [out, in] bf16 view instead of a new tensor (the stacked modulation matrix).
        `consume`: the module gives its storage away - W' overwrites m.weight's own memory (when that is a contiguous bf16
        tensor) and every parameter of the Linear is left EMPTY, so that preparing a sampling-only rank never holds the
        un-merged and the merged set at once (26.3 GB peak instead of 56.7).
        `backend`: "torch" forms the merge with torch ops (f32 temporaries, the vendor BLAS); "hip" with vc_lora_merge - bf16 or
        f32 weight / bias read as they are, bf16 factors only, no temporary of the size of W."""
        if backend == "hip":
            W = m.weight.detach()
            A = Bm = bB = None
            if m.rank:
                A, Bm = m.lora_A.weight.detach(), m.lora_B.weight.detach()
                bB = None if m.lora_B.bias is None else m.lora_B.bias.detach()
                if bB is not None and bB.dtype != torch.bfloat16:
                    raise hip.VclozeHipError(f"lora_merge='hip': lora_B.bias is {bB.dtype}, not bf16; use lora_merge=\"torch\"")
            if out is None and consume and W.dtype == torch.bfloat16 and W.is_contiguous():
                out = W                      # in place: each tile of W is read before it is written (csrc/lora_merge.hip)
            if out is W and not m.rank and (m.bias is None or (m.bias.dtype == torch.bfloat16 and m.bias.is_contiguous())):
                bias = None if m.bias is None else m.bias.detach()       # nothing to merge: the storage changes hands untouched
                for p in m.parameters():
                    p.data = torch.empty(0, dtype=p.dtype, device=p.device)
                return out, bias
            out, bias = hip.lora_merge(W, A, Bm, m.scale, out=out, bias=None if m.bias is None else m.bias.detach(), lora_b_bias=bB)
            if consume:
                for p in m.parameters():
                    p.data = torch.empty(0, dtype=p.dtype, device=p.device)
            return out, bias
        if backend != "torch":
            raise ValueError(f"merged_linear backend must be 'torch' or 'hip', got {backend!r}")
        W = m.weight.detach()
        W32 = W.float()                   # NOT a copy when the parameter is f32 already: never update it in place
        B32 = None if m.bias is None else m.bias.detach().float()
        if m.rank:
            delta = m.scale * (m.lora_B.weight.detach().float() @ m.lora_A.weight.detach().float())
            if W32.data_ptr() == W.data_ptr() and not consume:
                W32 = W32 + delta                 # out of place: the module keeps its un-merged weight
            else:
                W32 += delta                      # our own f32 temporary (or storage the module gives away)
            del delta
            if m.lora_B.bias is not None:
                B32 = (B32 if B32 is not None else 0) + m.scale * m.lora_B.bias.detach().float()
        if out is None and consume and W.dtype == torch.bfloat16 and W.is_contiguous():
            out = W
        if out is None:
            out = W32.to(torch.bfloat16).contiguous()
        else:
            out.copy_(W32)
        del W32
        bias = None if B32 is None else B32.to(torch.bfloat16).contiguous()
        if consume:
            for p in m.parameters():
                p.data = torch.empty(0, dtype=p.dtype, device=p.device)
        return out, bias

    @torch.no_grad()
    def prepare(self, free_parameters: bool = False) -> FluxEngine:
        """(Re)build the engine's device weights: bf16, contiguous, LoRA merged as W + s*B@A, b + s*b_B
        (exact in f32, rounded to bf16 once — DESIGN.md §numerics).  One-time preprocessing; uses torch ops.
        `free_parameters`: release the module's own parameter storage afterwards (sampling-only ranks of a
        data-parallel job: 23.8 GB of merged weights stay, the 26.3 GB of un-merged parameters go; the module can
        then no longer be re-prepared or saved until weights are loaded again)."""
        hip.require_gpu()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise hip.VclozeHipError("Flux weights must live on the GPU (model.to('cuda')) — there is no CPU path")
        if getattr(self, "_params_freed", False):
            raise hip.VclozeHipError("parameters were released by prepare(free_parameters=True); load weights again first")
        if self.lora_mode not in ("merged", "ref"):
            raise ValueError(f"lora_mode must be 'merged' or 'ref', got {self.lora_mode!r}")
        if self.lora_merge not in ("torch", "hip"):
            raise ValueError(f"lora_merge must be 'torch' or 'hip', got {self.lora_merge!r}")
        self._check_ref_plan()
        w, b, ref = {}, {}, ({} if self.lora_mode == "ref" else None)
        bf = lambda t: None if t is None else t.detach().to(torch.bfloat16).contiguous()  # noqa: E731
        # all modulation projections are stacked: one GEMM yields every shift/scale/gate of a step.  Their merged rows
        # are written straight into the stacked matrix (no 6.5 GB concatenation copy).
        mods: List[str] = []
        for i in range(self.params.depth):
            mods += [f"double_blocks.{i}.img_mod.lin", f"double_blocks.{i}.txt_mod.lin"]
        mods += [f"single_blocks.{i}.modulation.lin" for i in range(self.params.depth_single_blocks)]
        mods.append("final_layer.adaLN_modulation.1")
        lin = dict(self._linears())
        off, o = {}, 0
        for n in mods:
            off[n] = o
            o += lin[n].out_features
        mod_w = torch.empty(o, self.hidden_size, dtype=torch.bfloat16, device=dev)
        mod_b = torch.zeros(o, dtype=torch.bfloat16, device=dev)
        consume = free_parameters and ref is None
        for name, m in lin.items():
            if ref is None:
                if name in off:
                    _, bb = self.merged_linear(m, consume, out=mod_w[off[name]:off[name] + m.out_features], backend=self.lora_merge)
                    if bb is not None:
                        mod_b[off[name]:off[name] + m.out_features] = bb
                else:
                    w[name], b[name] = self.merged_linear(m, consume, backend=self.lora_merge)
                continue
            w[name], b[name] = bf(m.weight), bf(m.bias)
            A = B = bB = sc = None
            if m.rank:
                rk = (m.rank + 63) // 64 * 64            # zero-pad the rank to the GEMM's K granularity
                A = torch.zeros(rk, m.in_features, dtype=torch.bfloat16, device=dev)
                B = torch.zeros(m.out_features, rk, dtype=torch.bfloat16, device=dev)
                A[:m.rank], B[:, :m.rank] = bf(m.lora_A.weight), bf(m.lora_B.weight)
                bB = bf(m.lora_B.bias)
                # the reference multiplies the bf16 lora output by a python float (lora.py:96: f32 arithmetic, ONE rounding);
                # this mode applies it as the bf16 gate vector of the gated-residual epilogue - identical iff the scale
                # itself is a bf16 value (1.0, 0.5, 0.75 ...); anything else would be rounded once more, so refuse it
                if float(torch.tensor(m.scale, dtype=torch.bfloat16)) != float(m.scale):
                    raise ValueError(f"lora_mode='ref': lora scale {m.scale} of {name} is not representable in bf16; the parity "
                                     "mode would round it (use the merged mode, which applies it exactly in f32)")
                sc = torch.full((m.out_features,), m.scale, dtype=torch.bfloat16, device=dev)
            from .engine import RefLinear
            ref[name] = RefLinear(w[name], b[name], A, B, bB, sc)
        for name, p in self.named_parameters():
            if name.endswith("norm.scale"):
                w[name] = p.detach().to(torch.bfloat16).contiguous().clone()
        if ref is not None:              # parity mode: the modulation Linears were collected un-stacked above
            for n in mods:
                mod_w[off[n]:off[n] + w[n].shape[0]] = w[n]
                if b[n] is not None:
                    mod_b[off[n]:off[n] + w[n].shape[0]] = b[n]
        D = self.hidden_size
        qkv_heads = 0
        if ref is None and self.qkv_permute:
            qkv_heads = self.num_heads
            perm = hip.qkv_head_permutation(qkv_heads).to(dev)
            names = [f"double_blocks.{i}.{st}_attn.qkv" for i in range(self.params.depth) for st in ("img", "txt")]
            names += [f"single_blocks.{i}.linear1" for i in range(self.params.depth_single_blocks)]
            for n in names:          # in place, one matrix at a time (a 57 MB temporary): linear1's rows [0, 3D) only
                w[n][:3 * D] = w[n][:3 * D][perm]
                if b[n] is not None:
                    b[n][:3 * D] = b[n][:3 * D][perm]
        for i in range(self.params.depth_single_blocks):
            n = f"single_blocks.{i}.linear1"
            w[n + ".qkv"], w[n + ".mlp"] = w[n][: 3 * D], w[n][3 * D:]
            b[n + ".qkv"], b[n + ".mlp"] = b[n][: 3 * D], b[n][3 * D:]
            if ref is not None:         # linear1's two column ranges share lora_A
                from .engine import RefLinear
                r = ref[n]
                for sfx, sl in ((".qkv", slice(0, 3 * D)), (".mlp", slice(3 * D, None))):
                    ref[n + sfx] = RefLinear(r.w[sl], r.b[sl], r.A, None if r.B is None else r.B[sl],
                                             None if r.bB is None else r.bB[sl], None if r.scale is None else r.scale[sl])
        for n in mods:
            w.pop(n, None)
            b.pop(n, None)
        half = 128
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).to(dev)
        # |q|, |k| <= sqrt(128) * max|scale| after QKNorm (layers.py:75-84; RoPE is a rotation), so with c = 128^-0.5 * log2(e)
        # every attention logit obeys |c q.k| <= 128 c max|q scale| max|k scale| (+2 %: q and k pass three bf16 roundings each - norm, scale, RoPE -
        # worth (1 + 2^-9)^6 = 1.012 on the product; the kernel only compares the bound with its <= 100 cutoff)
        # The bound is kept per BLOCK (a double block: both streams share one attention): each launch gets its own, so outlier
        # scales in a few blocks of a checkpoint cost the running-max template there and nowhere else; `logit_bound` = the
        # largest of them, the cap handed to the C handle (which computes the per-block values itself: flux_weights.hip resolve()).
        amax = {n: float(t.float().abs().max()) for n, t in w.items() if n.endswith(("query_norm.scale", "key_norm.scale"))}
        blocks = sorted({n.split(".img_attn.")[0].split(".txt_attn.")[0].split(".norm.")[0] for n in amax})
        c_log = 1.02 * 11.313708498984761 * 1.4426950408889634          # 1.02 sqrt(128) log2(e), the constant of csrc/flux_rules.h
        logit_bounds = {}
        for pf in blocks:
            qm = max(v for n, v in amax.items() if n.startswith(pf + ".") and n.endswith("query_norm.scale"))
            km = max(v for n, v in amax.items() if n.startswith(pf + ".") and n.endswith("key_norm.scale"))
            bnd = c_log * qm * km
            logit_bounds[pf] = float(torch.tensor(bnd, dtype=torch.float32)) if bnd == bnd else 1e30      # (f32, as the C plan holds it)
        logit_bound = max(logit_bounds.values())
        pw = PreparedWeights(w=w, b=b, mod_w=mod_w, mod_b=mod_b, mod_off=off, n_mod=o, temb_freqs=freqs, ref=ref, qkv_heads=qkv_heads,
                             logit_bound=logit_bound, logit_bounds=logit_bounds)
        self._engine = FluxEngine(self.params, pw, dev)
        self._handle = None
        if free_parameters:
            for p in self.parameters():
                p.data = torch.empty(0, dtype=p.dtype, device=p.device)
            self._params_freed = True
            torch.cuda.empty_cache()
        self._fingerprint = self._weights_fingerprint()
        return self._engine

    def invalidate_engine(self) -> None:
        """Forget the prepared (merged, bf16) weights; the next forward / sample re-prepares.  Call after writing the
        parameters through a path that does not bump `_version` (`.data`, dist.broadcast).  Refused on a model whose
        parameters were released by prepare(free_parameters=True): the engine then holds the ONLY copy of the weights and
        dropping it would leave the module unusable (its parameters are empty, load_state_dict cannot fill them)."""
        if getattr(self, "_params_freed", False):
            raise hip.VclozeHipError("invalidate_engine: this model's parameters were released by prepare(free_parameters="
                                     "True); the prepared engine is the only copy of the weights - build a new model to "
                                     "load other weights")
        self._engine = None
        self._handle = None
        self._fingerprint = None

    def _library_handle(self):
        """load_in_library: the handle over this module's own state_dict, rebuilt when a parameter or the scale changed"""
        if not self.use_handle or self.lora_mode != "merged":
            raise hip.VclozeHipError("load_in_library prepares merged weights behind the C handle: it needs use_handle True and lora_mode "
                                     f"'merged' (got use_handle={self.use_handle}, lora_mode={self.lora_mode!r})")
        fp = self._weights_fingerprint()
        if self._handle is None or self._fingerprint != fp or not getattr(self._handle, "_loaded", None):
            hip.require_gpu()
            scales = {m.scale for _, m in self._linears() if m.rank}
            if len(scales) > 1:
                raise hip.VclozeHipError(f"load_in_library merges with ONE lora scale, the model holds {sorted(scales)}")
            from .handle import FluxHandle
            self._engine = None
            self._handle = FluxHandle.from_state_dict(self.params, self.state_dict(), scales.pop() if scales else 1.0,
                                                      next(self.parameters()).device)
            self._handle.stream = torch.cuda.Stream(device=self._handle.dev)      # capture needs a non-default stream
            self._fingerprint = fp
        return self._handle

    def plan(self):
        """whoever holds the device and the capture stream of this model's launches (`.dev`, `.stream`): the engine, or with
        load_in_library the C handle alone"""
        return self._library_handle() if self.load_in_library else self.engine()

    def engine(self) -> FluxEngine:
        if self.load_in_library:
            raise hip.VclozeHipError("load_in_library: the weights are prepared inside libvcloze_hip.so and there is no Python-ordered "
                                     "twin of them (engine()); set load_in_library = False for the parity paths")
        if self._engine is None or self._fingerprint != self._weights_fingerprint():
            self.prepare()
        return self._engine

    def handle(self):
        """The C-side engine (`handle.FluxHandle`) over the prepared weights, or None when this model runs the
        Python-ordered plan (use_handle False, or the un-merged LoRA mode unless ref_plan is "handle").  Test / A-B knobs set on
        `engine()` apply to both."""
        self._check_ref_plan()
        if self.load_in_library:
            return self._library_handle()
        eng = self.engine()
        if not self.use_handle or (eng.W.ref is not None and self.ref_plan != "handle"):
            return None
        if self._handle is None or self._handle.W is not eng.W:
            from .handle import FluxHandle
            self._handle = FluxHandle(self.params, eng.W, eng.dev)
        self._handle.set_options(attn_variant=eng.attn_variant, tile_cfg=eng.tile_cfg, fuse_qnorm=eng.fuse_qnorm, fuse_vt=eng.fuse_vt,
                                 qkv_heads=eng.W.qkv_heads, fuse_knorm=eng.fuse_knorm,
                                 logit_bound=eng.W.logit_bound if eng.bounded_softmax else 0.0, mlp_first=eng.mlp_first,
                                 splitk=eng.splitk)
        return self._handle

    # ------------------------------------------------------------------ the B1 boundary
    @torch.no_grad()
    def forward(self, img: Tensor, img_ids: Tensor, txt: Tensor, txt_ids: Tensor, timesteps: Tensor, y: Tensor,
                txt_mask: Tensor = None, img_mask: Tensor = None, guidance: Optional[Tensor] = None) -> Tensor:
        out = self._forward_bf16(img, img_ids, txt, txt_ids, timesteps, y, txt_mask, img_mask, guidance)
        return out.to(img.dtype) if img.dtype.is_floating_point else out

    @torch.no_grad()
    def forward_with_cfg(self, img: Tensor, img_ids: Tensor, txt: Tensor, txt_ids: Tensor, timesteps: Tensor, y: Tensor,
                         txt_mask: Tensor = None, img_mask: Tensor = None, guidance: Optional[Tensor] = None,
                         cfg_scale: float = 1.0) -> Tensor:
        """models/model.py:126-145: true classifier-free guidance over a batch whose first half is the conditional samples and
        whose second half the unconditional ones (negative prompt, other y, other guidance).  `forward` runs on the batch as given
        (the reference's `combined` is never used, so both halves keep their own state); returned is
        cat([uncond_v + cfg_scale * (cond_v - uncond_v), uncond_v]).  The combine (vc_cfg_combine, torch's bf16 roundings) acts on
        the kernels' bf16 output BEFORE the cast to the caller's dtype: the fused sampling loop sees the same bits."""
        if img.ndim == 3 and img.shape[0] % 2:
            raise ValueError(f"forward_with_cfg: the batch holds the conditional samples and then the unconditional ones, "
                             f"got an odd batch of {img.shape[0]}")
        out = self._forward_bf16(img, img_ids, txt, txt_ids, timesteps, y, txt_mask, img_mask, guidance)
        h = out.shape[0] // 2
        hip.cfg_combine(out[:h], out[h:], cfg_scale, out=out[:h])
        return out.to(img.dtype) if img.dtype.is_floating_point else out

    def chunk_plan(self, B: int, N: int, kw: dict, pairs: bool = False, channels=None) -> ChunkPlan:
        """the `ChunkPlan` of one call on this model, with forward's arguments in `kw`"""
        return ChunkPlan(B, N, kw["txt"], kw["y"], kw.get("guidance"), kw["img_ids"], kw["txt_ids"], kw.get("txt_mask"), kw.get("img_mask"),
                         self.params, self.plan().dev, self.max_batch(), pairs, channels)

    def _forward_plan(self, img, timesteps, **kw):
        """(the ChunkPlan of one forward, its per-sample timesteps)"""
        if img.ndim != 3 or kw["txt"].ndim != 3:
            raise ValueError("Input img and txt tensors must have 3 dimensions.")
        B, N, _ = img.shape
        return self.chunk_plan(B, N, kw), per_sample(timesteps, B)

    def _forward_bf16(self, img, img_ids, txt, txt_ids, timesteps, y, txt_mask=None, img_mask=None, guidance=None) -> Tensor:
        """Flux.forward as the kernels leave it: bf16 [B, N, out_channels] on the engine's device"""
        plan, timesteps = self._forward_plan(img, timesteps, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y=y, txt_mask=txt_mask,
                                             img_mask=img_mask, guidance=guidance)
        out = torch.empty(plan.B, plan.N, self.out_channels, dtype=torch.bfloat16, device=plan.dev)
        h = self.handle()
        with self.monitored(h) as monitored:
            if h is None:
                return self._forward_twin(plan, img, timesteps, out)
            for sl in plan.chunks:                      # one C call per chunk: vc_flux_prepare + vc_flux_forward
                h.prepare(*plan.prepare_args(sl, 1))
                o = torch.empty(plan.size(sl), plan.N, self.out_channels, dtype=torch.bfloat16, device=plan.dev)
                with monitored(1):
                    h.forward(plan.img_rows(img, sl, torch.bfloat16), timesteps[sl], timesteps.dtype == torch.bfloat16, o)
                out[sl].copy_(plan.img_back(o, sl))
        return out

    def _forward_twin(self, plan: ChunkPlan, img, timesteps, out) -> Tensor:
        """`_forward_bf16` with the Python-ordered plan (engine.FluxEngine): the same launches, ordered from here"""
        eng = self.engine()
        for sl in plan.chunks:
            bs = plan.size(sl)
            ws = eng.workspace(plan.T, plan.N, 1, bs)
            args, kwargs = plan.twin_prepare_args(sl, timesteps[sl].float().reshape(1, bs))
            eng.prepare_sample(ws, *args, timesteps_is_bf16=timesteps.dtype == torch.bfloat16, **kwargs)
            ws.XIN.copy_(plan.img_rows(img, sl, torch.bfloat16).reshape(bs * plan.N, -1))
            eng.eval_once(ws, None, euler=False, concat=False)
            out[sl].copy_(plan.img_back(ws.V.reshape(bs, plan.N, -1), sl))
        return out

    @contextmanager
    def monitored(self, h):
        """The numerics monitor around one call on the handle `h`, at the checked `monitor_level(h)`: yields chunk(capacity, stream),
        the bracket of one chunk's run.  A call that ends well leaves last_monitor_log / last_monitor_report."""
        level, logs, bad = self.monitor_level(h), [], []

        @contextmanager
        def chunk(capacity: int, stream=None):
            if level:
                h.set_monitor(level, capacity)
            try:
                yield
                if level:
                    first = h.monitor_report(stream)
                    if first is not None and not bad:
                        bad.append((len(logs),) + first)
                    logs.append(h.monitor_log(stream))
            finally:
                if level:
                    h.set_monitor(0)                    # the log was sized for this chunk

        yield chunk
        if level:
            self.last_monitor_log, self.last_monitor_report = logs, bad[0] if bad else None
            if bad and self.monitor_strict:
                raise FloatingPointError("the numerics monitor found a NaN / inf: chunk %d, evaluation %d, site '%s', sample %d of the chunk "
                                         "(Flux.last_monitor_log holds the statistics)" % bad[0])

    def monitor_level(self, h) -> int:
        """`monitor`, checked: 0, 1 or 2, and never silently ignored - only the C handle `h` implements it"""
        if self.monitor not in (0, 1, 2):
            raise ValueError(f"monitor must be 0, 1 or 2, got {self.monitor!r}")
        if self.monitor and h is None:
            raise ValueError("monitor needs the C handle: not available with the Python-ordered plan (use_handle False, or "
                             "lora_mode='ref' unless ref_plan='handle')")
        return int(self.monitor)

    def max_batch(self) -> int:
        """samples per launch sequence: the engine's (one in the Python-ordered un-merged mode), the handle's where it runs that mode"""
        if self.load_in_library:
            return self._library_handle().MAX_BATCH
        eng, h = self.engine(), self.handle()
        return h.MAX_BATCH if h is not None and eng.W.ref is not None else eng.MAX_BATCH

    @torch.no_grad()
    def block_taps(self, img: Tensor, img_ids: Tensor, txt: Tensor, txt_ids: Tensor, timesteps: Tensor, y: Tensor,
                   txt_mask: Tensor = None, img_mask: Tensor = None, guidance: Optional[Tensor] = None) -> dict:
        """One `forward` through the C handle with every per-block tap set (vc_flux_set_tap): the residual streams after img_in /
        txt_in ("img_in" [B, N, D], "txt_in" [B, T, D]), after every DoubleStream block ("double.{i}.img", "double.{i}.txt") and after
        every SingleStream block ("single.{i}" [B, T + N, D]: text rows, then image rows), as bf16 device tensors in the CALLER's row
        order (the reference's), plus "out" [B, N, out_channels].  Either LoRA mode; the taps are cleared afterwards."""
        h = self.handle()
        if h is None:
            raise hip.VclozeHipError("block_taps needs the C handle (use_handle True; with lora_mode 'ref': ref_plan 'handle')")
        plan, timesteps = self._forward_plan(img, timesteps, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y=y, txt_mask=txt_mask,
                                             img_mask=img_mask, guidance=guidance)
        T, N, D, dev = plan.T, plan.N, self.hidden_size, plan.dev
        names = h.tap_names()
        parts = {n: [] for n in names + ["out"]}
        for sl in plan.chunks:
            bs = plan.size(sl)
            h.prepare(*plan.prepare_args(sl, 1))
            bufs = {n: torch.empty(*h.tap_shape(n), dtype=torch.bfloat16, device=dev) for n in names}
            try:
                for n, t in bufs.items():
                    h.set_tap(n, t)
                o = torch.empty(bs, N, self.out_channels, dtype=torch.bfloat16, device=dev)
                h.forward(plan.img_rows(img, sl, torch.bfloat16), timesteps[sl], timesteps.dtype == torch.bfloat16, o)
            finally:
                for n in names:
                    h.set_tap(n, None)
            parts["out"].append(plan.img_back(o, sl))
            for n, t in bufs.items():
                if n.startswith("single."):
                    parts[n].append(plan.joint_back(t.reshape(bs, T + N, D), sl))
                elif n == "txt_in" or n.endswith(".txt"):
                    parts[n].append(plan.txt_back(t.reshape(bs, T, D), sl))
                else:
                    parts[n].append(plan.img_back(t.reshape(bs, N, D), sl))
        return {n: torch.cat(v, dim=0) for n, v in parts.items()}


class FluxLoraWrapper(Flux):
    """models/model.py:154-175: Flux with a LoRA pair on EVERY Linear (`replace_linear_with_lora`)."""

    def __init__(self, lora_rank: int = 128, lora_scale: float = 1.0, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.lora_rank = lora_rank
        for _, m in list(self._linears()):
            m.add_lora(lora_rank, lora_scale)
