"""Per-token view of the Flux step: the counterpart of tests/test_vae_gpu.py's per-pixel view (`assert_pixels_within_bf16_noise`).

A whole-tensor rel-L2 cannot see one wrong token: on `tiny_inputs(B=1)` (24 image rows) the bf16 oracle's own output with ONE row
scaled by 1.05 still measures 1.1e-2 against the bf16 oracle and 1.3e-2 against the fp32 one - inside TOL_ORACLE = 1.5e-2 and
TOL_GOLDEN = 3e-2 of tests/test_model_gpu.py - while that row's own error is 5.8 times the largest row error the bf16 oracle makes.

Statistic.  For tensors [B, rows, width]: err[b, r] = ||x[b, r, :] - o32[b, r, :]||_2 in fp64, o32 = the oracle's fp32 / "ref" run,
o16 = its bf16 / "merged" run on the same inputs.

Regions (`RowRegions`, built from the masks per sample): rows one code path treats alike - the live text rows and the live image
rows of a sample, and the masked rows of a RIGHT-PADDED stream, each in a region of their own (what
test_model_gpu.py::test_forward_b2_ragged_vs_golden already compares).  Masked rows of a stream whose mask has holes are left out
(they carry no meaning in either implementation, test_forward_randomised_geometry_sweep_vs_oracle); their share is reported and is
exactly the share of such rows in the inputs.  No live row is ever left out.

Assertion.  For every region: max_r err_got[r] <= m * max_r err_o16[r].  Every row is bounded on its own; the yardstick is the
maximum over the region of the reference's own bf16 error, a statistic over many rows.

ROW_M, ROW_M_TRAJ: NOT fitted to what the GPU returns.  The oracle has two legitimate bf16 executions, Prec("bf16", "merged")
and Prec("bf16", "ref") (LoRA un-merged: three more roundings per Linear).  Both are run against fp32 / "ref" on the CPU on every
input set of `CASES` (= what tests/test_rowview_gpu.py runs), and for the final output and every tap the per-region ratio of the
region maxima err_ref / err_merged and its inverse are taken; the bound is twice the largest of them, rounded up to one
significant digit (the rule of PIXEL_M in tests/test_vae_gpu.py).  `derive_row_m()` below re-measures it (python -m tests.rowview);
tests/test_rowview_cpu.py asserts that both executions pass with it in both directions.

Measured (largest two-way ratio of the case, and where):
  single evaluation (ROW_M)                            | sampler, 4 points = 3 evaluations (ROW_M_TRAJ)
    b1          1.155  single.1 / txt live[0]          |   final state, general masks of `sampler_inputs`:
    b2_ragged   1.164  double.0.img / img live[0]      |     img live[0] 1.041, img live[1] 1.019
    general     1.190  double.1.txt / txt padded[0]    |   2 * 1.041 = 2.08 -> ROW_M_TRAJ = 3
    notext      1.204  single.1 / txt live[0]
    T1          1.167  single.1 / txt live[0]
    L255        1.176  img_in / img live[0]
    L256        1.209  double.0.txt / txt live[0]
    L257        1.141  img_in / img live[0]
    L326        1.296  double.0.txt / txt live[0]
    b3_lengths  1.321  double.0.img / img live[2]
  largest 1.321; 2 * 1.321 = 2.64 -> ROW_M = 3.  (On tiny_inputs(B=1) and (B=2) alone: 1.16, which gives 3 as well.)
What ROW_M = 3 means for one row: a live image row of the B = 1 output scaled by 1.05 is 5.8 x its region's yardstick, by 1.03
3.6 x, by 1.025 3.0 x and by 1.02 2.5 x - detection ends at 2.5 % of ONE row (tests/test_rowview_cpu.py).
"""
import functools
import os
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch

ROW_M = 3.0
ROW_M_TRAJ = 3.0

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_golden.npz")


# ------------------------------------------------------------------------------------------------ regions
@dataclass(frozen=True)
class Region:
    name: str                 # "txt live" / "img live" / "txt padded" / "img padded"
    sample: int
    rows: Tuple[int, ...]     # indices on the row axis of the tensor the region is applied to


def _is_right_padded(m: torch.Tensor) -> bool:
    """1 ... 1 0 ... 0 (no live row behind a masked one); all live and all masked are the two ends of it"""
    n = int(m.sum())
    return bool(m[:n].all())


class RowRegions:
    """The regions of one input set.  `.txt` applies to [B, T, .] tensors (txt_in, double.i.txt), `.img` to [B, N, .] ones (the
    output, img_in, double.i.img, the sampler's state) and `.joint` to [B, T + N, .] ones (single.i: text rows, then image rows)."""

    def __init__(self, txt_mask: torch.Tensor, img_mask: torch.Tensor):
        tm, im = txt_mask.bool().cpu(), img_mask.bool().cpu()
        assert tm.dim() == 2 and im.dim() == 2 and tm.shape[0] == im.shape[0]
        self.B, self.T, self.N = tm.shape[0], tm.shape[1], im.shape[1]
        self.txt, self.left_out_txt = self._stream(tm, "txt")
        self.img, self.left_out_img = self._stream(im, "img")
        self.joint = self.txt + [Region(r.name, r.sample, tuple(i + self.T for i in r.rows)) for r in self.img]
        self.holes_txt = sum(int((~tm[b]).sum()) for b in range(self.B) if not _is_right_padded(tm[b]))
        self.holes_img = sum(int((~im[b]).sum()) for b in range(self.B) if not _is_right_padded(im[b]))

    @staticmethod
    def _stream(m: torch.Tensor, stream: str):
        regions: List[Region] = []
        left_out = 0
        for b in range(m.shape[0]):
            live = tuple(int(i) for i in torch.nonzero(m[b]).flatten())
            dead = tuple(int(i) for i in torch.nonzero(~m[b]).flatten())
            if live:
                regions.append(Region(f"{stream} live", b, live))
            if dead and _is_right_padded(m[b]):
                regions.append(Region(f"{stream} padded", b, dead))
            else:
                left_out += len(dead)
        return regions, left_out

    def for_tensor(self, name: str) -> List[Region]:
        """the regions of the tap `name` of flux_forward(..., taps=...) / FluxEngine.eval_once(..., taps=...); "out" = the output"""
        if name.startswith("single."):
            return self.joint
        return self.txt if name == "txt_in" or name.endswith(".txt") else self.img

    def share_left_out(self) -> float:
        """of all B * (T + N) rows; by construction equal to the share of masked rows of streams whose mask has holes"""
        return (self.left_out_txt + self.left_out_img) / (self.B * (self.T + self.N))


# ------------------------------------------------------------------------------------------------ the statistic
def row_errors(x, o32) -> torch.Tensor:
    """[B, rows]: per-row L2 error in fp64"""
    x, o32 = torch.as_tensor(x).double().cpu(), torch.as_tensor(o32).double().cpu()
    assert x.shape == o32.shape and x.dim() == 3, (x.shape, o32.shape)
    return (x - o32).norm(dim=-1)


def region_ratios(got, o16, o32, regions):
    """[(region, worst row, its error, the region's yardstick, ratio)]"""
    e_got, e_16 = row_errors(got, o32), row_errors(o16, o32)
    out = []
    for reg in regions:
        rows = torch.tensor(reg.rows, dtype=torch.long)
        eg, ey = e_got[reg.sample, rows], e_16[reg.sample, rows]
        k = int(eg.argmax())
        err, yard = float(eg[k]), float(ey.max())
        ratio = 0.0 if err == 0.0 else (err / yard if yard > 0.0 else float("inf"))
        out.append((reg, reg.rows[k], err, yard, ratio))
    return out


def assert_rows_within_bf16_noise(got, o16, o32, regions, what, m: float = ROW_M):
    """Every row of `got` is within m times the largest error the oracle's own bf16 run makes in the row's region.  Always
    writes the per-region ratios to the parity log; returns the largest ratio."""
    from tests.helpers import parity_log
    assert len(regions) > 0, what
    res = region_ratios(got, o16, o32, regions)
    parity_log(f"[rows] {what}: " + ", ".join(f"{reg.name}[{reg.sample}] {ratio:.3f}" for reg, _, _, _, ratio in res))
    for reg, row, err, yard, ratio in res:
        assert err <= m * yard, (f"{what}: region '{reg.name}' of sample {reg.sample}, row {row}: error {err:.4e} against the fp32 oracle, "
                                 f"the bf16 oracle's largest in the region {yard:.4e}, ratio {ratio:.3f} > {m}")
    return max(r[-1] for r in res)


# ------------------------------------------------------------------------------------------------ the input sets
def _b1():
    from tests.procedural import tiny_inputs
    return tiny_inputs(B=1), torch.tensor([0.7])


def _b2_ragged():
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=2, seed=7)
    inp["img_mask"][1, -12:] = 0
    return inp, torch.tensor([0.9, 0.25])


def _general():
    from tests.procedural import tiny_inputs
    g = np.load(GOLDEN)
    inp = tiny_inputs(B=2, seed=7)
    inp["txt_mask"], inp["img_mask"] = torch.tensor(g["flux_general_txt_mask"]), torch.tensor(g["flux_general_img_mask"])
    return inp, torch.tensor([0.9, 0.25])


def _notext():
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=2, seed=13)
    inp["txt_mask"][1] = 0
    inp["img_mask"][0, [0, 3]] = 0
    return inp, torch.tensor([0.8, 0.3])


def _edge(T, rows_hw, seed, t=0.6):
    def make():
        from tests.procedural import tiny_inputs
        return tiny_inputs(B=1, rows_hw=rows_hw, T=T, seed=seed), torch.tensor([t])
    return make


def _b3_lengths():
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=3, rows_hw=((4, 12), (6, 10)), T=19, seed=21)     # N = 12 + 15 = 27
    inp["txt_mask"][1, -3:] = 0
    inp["txt_mask"][2, -7:] = 0
    inp["img_mask"][1, -5:] = 0
    inp["img_mask"][2, -11:] = 0
    inp["guidance"] = torch.tensor([30.0, 10.0, 3.5])
    return inp, torch.tensor([0.9, 0.5, 0.1])


_N192 = ((8, 48), (8, 48))                       # 2 x (4 x 24) = 192 image rows
# name -> () -> (inputs of tests.procedural.tiny_inputs, per-sample timesteps): every single-evaluation case of test_rowview_gpu.py
CASES = {
    "b1": _b1,                                   # test_forward_b1_vs_golden_and_oracle
    "b2_ragged": _b2_ragged,                     # test_forward_b2_ragged_vs_golden: sample 1 right-padded by 12 image rows
    "general": _general,                         # test_forward_general_masks_vs_golden: holes in both streams
    "notext": _notext,                           # test_forward_sample_without_text_vs_reference
    "T1": _edge(1, ((4, 12), (4, 12)), 31),      # a text stream of one row
    "L255": _edge(63, _N192, 32),                # the seam one row before / on / one row behind a 64-row tile edge and
    "L256": _edge(64, _N192, 33),                # the sequence one row short of / exactly / one row over 256
    "L257": _edge(65, _N192, 34),
    "L326": _edge(40, ((8, 40), (6, 44), (10, 56)), 35),   # 40 + 80 + 66 + 140: over the 64 / 128 / 256 / 320 edges, seam inside a tile
    "b3_lengths": _b3_lengths,                   # three lengths, three timesteps, three guidance values
}


def sampler_inputs():
    """test_model_gpu.py::test_sampler_general_masks_vs_oracle"""
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=2, seed=11)
    inp["txt_mask"][0, [0, 5]] = 0
    inp["txt_mask"][1, -4:] = 0
    inp["img_mask"][0, [1, 2, 9]] = 0
    return inp


SAMPLER_POINTS = 4


@functools.lru_cache(maxsize=None)
def tiny_state_dict():
    from tests.procedural import procedural_state_dict
    g = np.load(GOLDEN)
    keys = [str(k) for k in g["keys"]]
    shapes = [tuple(int(x) for x in str(s).split(",")) for s in g["shapes"]]
    return procedural_state_dict(zip(keys, shapes))


def tap_names():
    from tests.procedural import TINY
    return (["img_in", "txt_in"] + [f"double.{i}.{s}" for i in range(TINY["depth"]) for s in ("img", "txt")]
            + [f"single.{i}" for i in range(TINY["depth_single_blocks"])])


# ------------------------------------------------------------------------------------------------ the oracle's runs
class _f32_guidance:
    """the tests hand Flux.forward an f32 guidance tensor: no bf16 rounding of 1000 g (as test_model_gpu.py::_oracle)"""

    def __enter__(self):
        import oracle.flux_oracle as O
        self.orig = orig = O.compute_vec
        O.compute_vec = lambda *a, **k: orig(*a, **{**k, "guidance_is_bf16": False})

    def __exit__(self, *exc):
        import oracle.flux_oracle as O
        O.compute_vec = self.orig


def oracle_forward(inp, t, mode, lora):
    """{"out": flux_forward's result, tap name: tensor} in the caller's row order (the oracle never reorders)"""
    import oracle.flux_oracle as O
    from tests.procedural import TINY
    taps = {}
    with _f32_guidance():
        out = O.flux_forward(tiny_state_dict(), O.FluxGeometry(**TINY), torch.cat((inp["x"], inp["cond"]), -1), inp["img_ids"],
                             inp["txt"], inp["txt_ids"], t, inp["y"], inp["txt_mask"], inp["img_mask"], inp["guidance"],
                             P=O.Prec(mode, lora), taps=taps)
    taps.pop("vec")
    taps["out"] = out
    return taps


@functools.lru_cache(maxsize=None)
def oracle_runs(case: str):
    """(inputs, timesteps, regions, {"o32" | "o16" | "o16ref": {"out" / tap: tensor}}) of CASES[case]; computed once, shared by
    every test that needs it and never written to"""
    inp, t = CASES[case]()
    runs = {"o32": oracle_forward(inp, t, "fp32", "ref"), "o16": oracle_forward(inp, t, "bf16", "merged"),
            "o16ref": oracle_forward(inp, t, "bf16", "ref")}
    return inp, t, RowRegions(inp["txt_mask"], inp["img_mask"]), runs


def oracle_sample(inp, mode, lora, points=SAMPLER_POINTS):
    """final state of O.sample_euler over `points` time points (points - 1 evaluations), bf16 state in bf16 mode"""
    import oracle.flux_oracle as O
    from tests.procedural import TINY
    G, P = O.FluxGeometry(**TINY), O.Prec(mode, lora)

    def model_fn(xin, tm):
        return O.flux_forward(tiny_state_dict(), G, xin, inp["img_ids"], inp["txt"], inp["txt_ids"], tm, inp["y"], inp["txt_mask"],
                              inp["img_mask"], inp["guidance"], P=P)
    with _f32_guidance():
        states, _ = O.sample_euler(model_fn, inp["x"], inp["cond"], O.time_grid(points, inp["x"].shape[1], True, 1), P)
    return states[-1]


@functools.lru_cache(maxsize=None)
def oracle_sampler_runs():
    inp = sampler_inputs()
    runs = {"o32": oracle_sample(inp, "fp32", "ref"), "o16": oracle_sample(inp, "bf16", "merged"), "o16ref": oracle_sample(inp, "bf16", "ref")}
    return inp, RowRegions(inp["txt_mask"], inp["img_mask"]), runs


# ------------------------------------------------------------------------------------------------ the derivation of ROW_M
def two_way_ratios(a, b, o32, regions):
    """per region: max(err_a / err_b, err_b / err_a) of the region maxima"""
    ea, eb = row_errors(a, o32), row_errors(b, o32)
    out = []
    for reg in regions:
        rows = torch.tensor(reg.rows, dtype=torch.long)
        ma, mb = float(ea[reg.sample, rows].max()), float(eb[reg.sample, rows].max())
        out.append((reg, 1.0 if ma == mb else max(ma / mb, mb / ma)))
    return out


def derive_row_m(verbose=print):
    """(largest two-way ratio over CASES, output and every tap; the same for the sampler's final state)"""
    worst = (0.0, None)
    for case in CASES:
        _, _, regs, runs = oracle_runs(case)
        top = (0.0, None)
        for name in ["out"] + tap_names():
            for reg, ratio in two_way_ratios(runs["o16ref"][name], runs["o16"][name], runs["o32"][name], regs.for_tensor(name)):
                top = max(top, (ratio, f"{name} / {reg.name}[{reg.sample}]"), key=lambda v: v[0])
        verbose(f"{case:11s} largest ratio {top[0]:.3f} at {top[1]}")
        worst = max(worst, (top[0], f"{case}: {top[1]}"), key=lambda v: v[0])
    _, regs, runs = oracle_sampler_runs()
    traj = max(two_way_ratios(runs["o16ref"], runs["o16"], runs["o32"], regs.img), key=lambda v: v[1])
    verbose(f"single evaluation: {worst[0]:.3f} at {worst[1]}")
    verbose(f"sampler, {SAMPLER_POINTS} points: {traj[1]:.3f} at {traj[0].name}[{traj[0].sample}]")
    return worst[0], traj[1]


if __name__ == "__main__":
    derive_row_m()
