"""Per-token view of the T5 and CLIP encoders: the counterpart of tests/rowview.py for an encoder output [L, D].

A whole-tensor rel-L2 cannot see one wrong token.  tests/test_text_gpu.py and tests/test_text_handle_gpu.py assert
rel_l2(out, o32) <= 3 * noise + 2e-3; the bf16 oracle's own output with ONE row scaled by 1.25 (T5, 64 or 128 rows) or by 1.05
(CLIP, 24 or 16 rows) passes that line (tests/test_tokenview_cpu.py), and at L = 512 a row that is zero measures 4.4e-2 beside a
tolerance of the same order.

Statistic.  err[r] = ||x[r] - o32[r]||_2 in fp64, o32 = the oracle's fp32 run, o16 = its "bf16" run on the same ids.

Regions: rows one code path treats alike.  T5: the first and the last row of every 64-row tile, each on its own, and the interior
rows as a whole.  CLIP: row 0 (the causal block's first row), the EOS row (it becomes `pooled`), the last live row (the one beside
the pad rows: L = 7 runs as 64 rows, 77 as 128), the rest.  `pooled` is one more row.  No live row is left out: the share left out
is 0, asserted by `assert_tokens_within_bf16_noise` on every call.  The regions say WHERE the worst row is (every region's worst
ratio and row are logged); the bound holds for every row alike.

Yardstick: the 0.9 quantile, over all live rows of the case, of the bf16 oracle's own row errors (`pooled` takes the yardstick of the
hidden rows).  T5's bf16 row errors are uneven (t5_a: max 0.437, median 0.138, min 0.080; heavy on a few rows whose softmax is
peaked) and, row by row, the two bf16 executions below agree badly: with max(err_o16[r], median) as a yardstick per row their
largest two-way ratio is 3.31, which makes a margin of 7 and lets a loud row times 1.32 pass; with the plain maximum it is 1.53
(margin 4, a row times 1.19 passes everywhere); with the 0.9 quantile 2.39 (margin 5, 1.13).  CLIP's row errors are flat (0.045 to
0.064) and the choice changes nothing there.  Compared on the oracle alone, before any GPU run.

Assertion.  For every row: err_got[r] <= TOKEN_M[encoder] * yardstick.

TOKEN_M: NOT fitted to what the GPU returns.  oracle/text_oracle.py has two legitimate bf16 executions: "bf16" rounds every tensor
the HF module materialises, "bf16_fused" drops the roundings a fused implementation does not make (Linear + bias + residual once,
Linear + activation once, the score once after scale / bias) - the two ends of what a correct bf16 implementation rounds.  Both run
against fp32 on the CPU on every case of CASES and WIDTH_CASES (= what tests/test_text_tokens_gpu.py and the two width tests of
tests/test_text_gpu.py run), each judged with the other as the yardstick; per encoder the margin is twice the largest ratio, rounded
up to one significant digit (the rule of PIXEL_M and ROW_M).  T5 and CLIP get a margin each, since their noise differs in kind; one
margin for both would be T5's.  `derive_token_m()` re-measures it (python -m tests.tokenview, 25 s, most of it the XXL-width case);
tests/test_tokenview_cpu.py asserts it and that both executions pass both ways.

Measured (largest two-way ratio of the case and where; then: the smallest s at which ONE row of the bf16 oracle's output times s
fails at EVERY row / at the quietest row):
  t5_a           1.647 interior row 54    1.128 / 1.123    clip_a          1.229 rest row 6     1.015 / 1.015
  t5_b           2.269 interior row 114   1.127 / 1.123    clip_b          1.114 rest row 2     1.015 / 1.015
  t5_64          2.033 interior row 54    1.117 / 1.115    clip_7_last     1.139 rest row 4     1.014 / 1.014
  t5_128         1.972 interior row 1     1.125 / 1.121    clip_24_mid     1.233 rest row 22    1.015 / 1.015
  t5_192         1.936 interior row 19    1.120 / 1.118    clip_64_first   1.196 rest row 43    1.015 / 1.014
  t5_64_prompt   1.411 interior row 4     1.081 / 1.077    clip_64_last    1.228 rest row 6     1.015 / 1.014
  t5_128_prompt  1.437 interior row 20    1.088 / 1.084    clip_77_eospad  1.262 rest row 1     1.015 / 1.014
  t5_192_prompt  1.757 interior row 175   1.072 / 1.071    clip_77_last    1.216 rest row 66    1.015 / 1.014
  t5_depth1      2.171 interior row 27    1.062 / 1.060    clip_depth1     1.206 rest row 51    1.012 / 1.011
  t5_depth2      2.390 interior row 67    1.103 / 1.100    clip_depth2     1.164 rest row 43    1.015 / 1.015
  t5_outlier     1.613 interior row 14    1.035 / 1.029    clip_outlier    1.094 rest row 1     1.018 / 1.016
  t5_xxl         1.579 interior row 362   1.384 / 1.384    clip_l          1.163 rest row 15    1.018 / 1.017
  T5: 2 * 2.390 = 4.78 -> TOKEN_M["t5"] = 5.        CLIP: 2 * 1.262 = 2.52 -> TOKEN_M["clip"] = 3.
What that means for one row: at the tiny width a T5 row off by 13 % of itself and a CLIP row off by 2 % fail wherever they are; a
row that is zero or another token's is 3.6 - 90 times beyond the bound (3.6: a neighbour's row in T5's outlier-channel case, where
the rows share the one loud channel; otherwise from 7.8).  Two limits, both properties of the reference and stated in
tests/test_tokenview_cpu.py: (1) at XXL width (procedural weights, 2 layers) the bf16 oracle's own row error is 4 - 10 % of a row,
so a scaled row fails only from 1.39 on - the x 1.25 mutation is a condition at every tiny-width case and at CLIP-L width, not at
XXL width, where a zero or a neighbour's row still is 2.6 - 4.4 times beyond the bound; (2) T5 has no absolute positions, so
neighbouring rows that hold the same token (the pad rows of a prompt) are 0.000 - 0.002 apart in fp32 and a swap of two of them is
no wrong result: the neighbour mutation takes the nearest row that holds another token there.
"""
import functools
import math
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import text_oracle as TO
from tests.procedural import TINY_CLIP, TINY_T5, procedural_text_param, tiny_ids

TOKEN_M = {"t5": 5.0, "clip": 3.0}
TILE = 64                                            # rows of a GEMM / attention tile, and the multiple CLIP's rows are padded to

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_golden.npz")
TINY_CLIP77 = dict(TINY_CLIP, max_position_embeddings=77)     # TINY_CLIP with the product's 77 positions, for L = 64 and 77
# the two width cases of tests/test_text_gpu.py: t5-v1_1-xxl and clip-vit-large-patch14 geometry, 2 / 3 layers, small vocabulary
T5_XXL_2 = dict(vocab_size=512, d_model=4096, d_kv=64, d_ff=10240, num_layers=2, num_heads=64,
                relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
CLIP_L_3 = dict(vocab_size=512, hidden_size=768, intermediate_size=3072, num_hidden_layers=3, num_attention_heads=12,
                max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=511)


# ------------------------------------------------------------------------------------------------ regions
@dataclass(frozen=True)
class Region:
    name: str
    rows: Tuple[int, ...]


def t5_regions(L: int):
    """first and last row of every 64-row tile, each a region of its own, and the interior rows as a whole"""
    assert L > 0 and L % TILE == 0, L
    out, interior = [], []
    for t in range(L // TILE):
        out += [Region(f"tile {t} first", (t * TILE,)), Region(f"tile {t} last", (t * TILE + TILE - 1,))]
        interior += range(t * TILE + 1, t * TILE + TILE - 1)
    return out + [Region("interior", tuple(interior))]


def clip_regions(L: int, eos: int):
    """row 0, the EOS row (the one that becomes `pooled`), the last live row, the rest; a row that is two of these is listed under
    the first of them in that order"""
    assert 0 <= eos < L
    named = {}
    for name, r in (("row 0", 0), ("eos", eos), ("last", L - 1)):
        named.setdefault(r, name)
    out = [Region(name, (r,)) for r, name in sorted(named.items(), key=lambda kv: ("row 0", "eos", "last").index(kv[1]))]
    rest = tuple(r for r in range(L) if r not in named)
    return out + ([Region("rest", rest)] if rest else [])


def share_left_out(regions, L: int) -> float:
    """share of the L live rows outside every region; asserts the regions are disjoint.  0.0 for every case here (asserted where
    the regions are used): no live row is ever left out"""
    seen = np.zeros(L, dtype=np.int64)
    for reg in regions:
        assert len(reg.rows) > 0, reg
        seen[list(reg.rows)] += 1
    assert seen.max() <= 1, "regions overlap"
    return float((seen == 0).sum()) / L


# ------------------------------------------------------------------------------------------------ the statistic
def row_errors(x, o32) -> torch.Tensor:
    """[L]: per-row L2 error in fp64"""
    x, o32 = torch.as_tensor(x).double().cpu(), torch.as_tensor(o32).double().cpu()
    assert x.shape == o32.shape and x.dim() == 2, (x.shape, o32.shape)
    return (x - o32).norm(dim=-1)


YARD_Q = 0.9


def yardstick(o16, o32) -> float:
    """the 90th percentile over all live rows of the bf16 oracle's own row errors (module docstring: why not the row's own error,
    the median or the maximum)"""
    return float(row_errors(o16, o32).quantile(YARD_Q))


def region_ratios(got, o16, o32, regions, pooled=None):
    """[(region name, worst row, its error, the yardstick, ratio)]; `pooled` = (got, o16, o32) of the pooled vector, judged as one
    more row (row -1 of region "pooled") with the yardstick of the hidden rows"""
    e, y = row_errors(got, o32), yardstick(o16, o32)
    out = []
    for reg in regions:
        rows = torch.tensor(reg.rows, dtype=torch.long)
        r = reg.rows[int(e[rows].argmax())]
        out.append((reg.name, r, float(e[r]), y, float(e[r]) / y))
    if pooled is not None:
        pg, _, p32 = (torch.as_tensor(t).reshape(1, -1) for t in pooled)
        ep = float(row_errors(pg, p32))
        out.append(("pooled", -1, ep, y, ep / y))
    return out


def assert_tokens_within_bf16_noise(got, o16, o32, regions, what, m: float, pooled=None):
    """Every row of `got` (and `pooled`) is within m = TOKEN_M[encoder] times the yardstick.  Always writes the worst ratio and its row for every region to the
    parity log; returns the largest ratio."""
    from tests.helpers import parity_log
    L = torch.as_tensor(o32).shape[0]
    assert share_left_out(regions, L) == 0.0, f"{what}: live rows outside every region"
    assert torch.isfinite(torch.as_tensor(got).float()).all(), what
    res = region_ratios(got, o16, o32, regions, pooled)
    parity_log(f"[tokens] {what}: " + ", ".join(f"{name} {ratio:.3f} (row {row})" for name, row, _, _, ratio in res))
    for name, row, err, yard, ratio in res:
        assert err <= m * yard, (f"{what}: region '{name}', row {row}: error {err:.4e} against the fp32 oracle, yardstick (the {YARD_Q:g} quantile of the "
                                 f"bf16 oracle's row errors) {yard:.4e}, ratio {ratio:.3f} > {m}")
    return max(r[-1] for r in res)


# ------------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    kind: str                                 # "t5" | "clip"
    ids: Tuple[int, ...]
    wide_positions: bool = False              # clip: TINY_CLIP77 instead of TINY_CLIP
    depth: Optional[int] = None               # run the first `depth` layers only (the same weights), then the final norm
    outlier: Optional[int] = None             # this embedding channel is scaled by 2^7 (the massive activations of real T5 weights)
    width: bool = False                       # T5_XXL_2 / CLIP_L_3 instead of the tiny configuration

    @property
    def cfg(self):
        if self.width:
            return T5_XXL_2 if self.kind == "t5" else CLIP_L_3
        return TINY_T5 if self.kind == "t5" else (TINY_CLIP77 if self.wide_positions else TINY_CLIP)

    @property
    def L(self):
        return len(self.ids)

    @property
    def eos(self):
        """CLIPTextTransformer.forward's index: the first EOS"""
        return self.ids.index(self.cfg["eos_token_id"])

    def regions(self):
        return t5_regions(self.L) if self.kind == "t5" else clip_regions(self.L, self.eos)


def _t5_random(L, seed, **kw):
    return Case("t5", tuple(tiny_ids(L, TINY_T5["vocab_size"], seed=seed).tolist()), **kw)


def _t5_prompt(L, n, seed):
    """what HFEmbedder feeds with attention_mask=None: n live ids (none of them 0 or 1), EOS (1), pad id 0 up to L"""
    live = (2 + tiny_ids(n, TINY_T5["vocab_size"] - 2, seed=seed)).tolist()
    return Case("t5", tuple(live + [1] + [0] * (L - n - 1)))


def _clip(L, seed, eos_at, eos_padding=False, **kw):
    eos = TINY_CLIP["eos_token_id"]
    ids = tiny_ids(L, TINY_CLIP["vocab_size"], seed=seed, eos=eos, eos_at=eos_at)
    if eos_padding:                               # the CLIP tokenizer pads with EOS
        ids[eos_at:] = eos
    return Case("clip", tuple(ids.tolist()), wide_positions=L > TINY_CLIP["max_position_embeddings"], **kw)


def _golden(name):
    kind = name.split("_")[0]
    return Case(kind, tuple(int(i) for i in np.load(GOLDEN)[name + "_ids"]))


CASES = {
    # the four cases with transformers goldens (tests/golden/text_golden.npz)
    "t5_a": lambda: _golden("t5_a"), "t5_b": lambda: _golden("t5_b"),
    "clip_a": lambda: _golden("clip_a"), "clip_b": lambda: _golden("clip_b"),
    # T5: one, two, three tiles (192: distances past relative_attention_max_distance = 128), random ids and prompt-shaped ids
    "t5_64": lambda: _t5_random(64, 51), "t5_128": lambda: _t5_random(128, 52), "t5_192": lambda: _t5_random(192, 53),
    "t5_64_prompt": lambda: _t5_prompt(64, 9, 54), "t5_128_prompt": lambda: _t5_prompt(128, 20, 55),
    "t5_192_prompt": lambda: _t5_prompt(192, 5, 56),
    "t5_depth1": lambda: _t5_random(192, 57, depth=1), "t5_depth2": lambda: _t5_random(192, 57, depth=2),
    "t5_outlier": lambda: _t5_random(128, 58, outlier=5),
    # CLIP: L = 7 (Lp = 64, L % 8 != 0), 24, 64 (no pad rows), 77 (Lp = 128); EOS last / in the middle / first / followed by EOS padding
    "clip_7_last": lambda: _clip(7, 61, 6), "clip_24_mid": lambda: _clip(24, 62, 9),
    "clip_64_first": lambda: _clip(64, 63, 0), "clip_64_last": lambda: _clip(64, 64, 63),
    "clip_77_eospad": lambda: _clip(77, 65, 20, eos_padding=True), "clip_77_last": lambda: _clip(77, 66, 76),
    "clip_depth1": lambda: _clip(77, 67, 40, depth=1), "clip_depth2": lambda: _clip(77, 67, 40, depth=2),
    "clip_outlier": lambda: _clip(24, 68, 13, outlier=5),
}
# width: the inputs of test_xxl_width_t5_layers_match_oracle and test_clip_l_width_matches_oracle (tests/test_text_gpu.py).  They feed
# TOKEN_M and pass both ways; of the three mutations the x 1.25 one is NOT a condition at XXL width (module docstring)
WIDTH_CASES = {
    "t5_xxl": lambda: Case("t5", tuple(tiny_ids(512, 512, seed=77).tolist()), width=True),
    "clip_l": lambda: Case("clip", tuple(tiny_ids(77, 512, seed=78, eos=511, eos_at=20).tolist()), width=True),
}

OUTLIER_SCALE = 2.0 ** 7


def _make_sd(kind: str, cfg: dict):
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    with torch.device("meta"):                               # the key list and the shapes only
        m = T5EncoderModel(T5Config(**cfg)) if kind == "t5" else CLIPTextModel(CLIPTextConfig(**cfg))
    sd = {k: procedural_text_param(k, v.shape) for k, v in m.state_dict().items()}
    if kind == "t5":
        sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    return sd


@functools.lru_cache(maxsize=None)
def _base_sd(kind: str, wide_positions: bool):
    return _make_sd(kind, TINY_T5 if kind == "t5" else (TINY_CLIP77 if wide_positions else TINY_CLIP))


def state_dict(case: Case) -> dict:
    """the procedural weights of the case's configuration (every value exact in bf16), never written to; the 0.4 B parameters of
    the XXL-width case are made anew at every call and not kept"""
    if case.width:
        return _make_sd(case.kind, case.cfg)
    sd = _base_sd(case.kind, case.wide_positions)
    if case.outlier is not None:
        sd = dict(sd)
        for key in (("shared.weight", "encoder.embed_tokens.weight") if case.kind == "t5" else ("text_model.embeddings.token_embedding.weight",)):
            w = sd[key].clone()
            w[:, case.outlier] *= OUTLIER_SCALE            # |e| <= 1.5 * 2^7 = 192 with 7 significant bits: still exact in bf16
            sd[key] = w
    return sd


def oracle_run(case: Case, mode: str, sd: Optional[dict] = None):
    """(hidden [L, D], pooled [D] | None) of the oracle in `mode`"""
    ids, sd = torch.tensor(case.ids), state_dict(case) if sd is None else sd
    if case.kind == "t5":
        return TO.t5_encode(sd, ids, case.cfg, mode, num_layers=case.depth), None
    pooled, hs = TO.clip_text(sd, ids, case.cfg, mode, num_layers=case.depth)
    return hs, pooled


@functools.lru_cache(maxsize=None)
def oracle_runs(name: str):
    """(case, regions, {"o32" | "o16" | "o16f": (hidden, pooled | None)}) of CASES[name]: fp32, "bf16" and "bf16_fused"; computed
    once, shared by every test that needs it and never written to"""
    case = (CASES.get(name) or WIDTH_CASES[name])()
    regions = case.regions()
    assert share_left_out(regions, case.L) == 0.0
    sd = state_dict(case)
    return case, regions, {"o32": oracle_run(case, "fp32", sd), "o16": oracle_run(case, "bf16", sd), "o16f": oracle_run(case, "bf16_fused", sd)}


def pooled_triple(runs, got_pooled, yard="o16"):
    return None if runs["o32"][1] is None else (got_pooled, runs[yard][1], runs["o32"][1])


# ------------------------------------------------------------------------------------------------ the derivation of TOKEN_M
def two_way_ratios(runs, regions):
    """per region (and `pooled`): (name, row, the larger of the statistic of "bf16_fused" under the yardstick of "bf16" and the reverse)"""
    o32 = runs["o32"][0]
    a = region_ratios(runs["o16f"][0], runs["o16"][0], o32, regions, pooled_triple(runs, runs["o16f"][1], "o16"))
    b = region_ratios(runs["o16"][0], runs["o16f"][0], o32, regions, pooled_triple(runs, runs["o16"][1], "o16f"))
    return [(ra[0], ra[1] if ra[4] >= rb[4] else rb[1], max(ra[4], rb[4])) for ra, rb in zip(a, b)]


def margin_from(ratio: float) -> float:
    """twice the ratio, rounded up to one significant digit (the rule of PIXEL_M and ROW_M)"""
    x = 2.0 * ratio
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


def scale_that_fails(o16, o32, m: float) -> torch.Tensor:
    """[L]: per row, the smallest s > 1 at which that row of the bf16 oracle's output times s misses the bound:
    |s a - b| = m y with a = o16[r], b = o32[r]"""
    a, b = torch.as_tensor(o16).double(), torch.as_tensor(o32).double()
    y = m * yardstick(o16, o32)
    aa, ab, bb = (a * a).sum(-1), (a * b).sum(-1), (b * b).sum(-1)
    return (ab + torch.sqrt(ab * ab - aa * (bb - y * y))) / aa


def derive_token_m(verbose=print):
    """{"t5" | "clip": the largest two-way ratio over the encoder's CASES, every region and `pooled`}"""
    worst = {"t5": (0.0, None), "clip": (0.0, None)}
    for name in list(CASES) + list(WIDTH_CASES):
        case, regions, runs = oracle_runs(name)
        top = max(two_way_ratios(runs, regions), key=lambda v: v[2])
        e = row_errors(runs["o16"][0], runs["o32"][0])
        s = scale_that_fails(runs["o16"][0], runs["o32"][0], TOKEN_M[case.kind])
        quiet = int(e.argmin())
        verbose(f"{name:15s} L {case.L:3d}  largest ratio {top[2]:.3f} at {top[0]} (row {top[1]});  bf16 row error max {float(e.max()):.3f} "
                f"median {float(e.median()):.3f} min {float(e.min()):.3f} yardstick {yardstick(runs['o16'][0], runs['o32'][0]):.3f};  one row "
                f"times s fails on every row from s = {float(s.max()):.3f}, on the quietest (row {quiet}) from {float(s[quiet]):.3f}")
        worst[case.kind] = max(worst[case.kind], (top[2], f"{name}: {top[0]} (row {top[1]})"), key=lambda v: v[0])
    for kind, (ratio, where) in worst.items():
        verbose(f"{kind}: largest two-way ratio {ratio:.3f} at {where}; 2 x {ratio:.3f} = {2 * ratio:.2f} -> TOKEN_M[{kind!r}] = {margin_from(ratio):g} "
                f"(the module has {TOKEN_M[kind]:g})")
    return {kind: v[0] for kind, v in worst.items()}


if __name__ == "__main__":
    derive_token_m()
