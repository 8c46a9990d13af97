"""-m gpu: the assembled Flux step judged PER TOKEN (tests/rowview.py) - `Flux.forward`, every per-block tap of the same evaluation
and the fused Euler sampler on the tiny model (hidden 256, 2 heads of 128), against the CPU oracle's fp32 run with the oracle's own
bf16 run as the yardstick, region by region: row order after the valid-first reorder, the text / image seam, per-sample
modulation / gate / RoPE rows, the scatter back and the last layer.  The bound ROW_M comes from the oracle alone
(tests/rowview.py's docstring; tests/test_rowview_cpu.py shows what it catches); the ratios measured on the MI355X stand in the
docstrings below as records."""
import pytest
import torch

from tests import rowview as RV

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    m, sd = tiny_model()
    want = RV.tiny_state_dict()                          # the oracle runs of tests/rowview.py use the same weights
    assert sorted(sd) == sorted(want) and all(torch.equal(sd[k], want[k]) for k in sd)
    return m


def _args(inp):
    return dict(img_ids=inp["img_ids"].to(DEV), txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), txt_mask=inp["txt_mask"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                guidance=inp["guidance"].to(DEV))


def hip_forward_and_taps(m, inp, t):
    """{"out": Flux.forward's result, tap name: tensor}, f32 on the host, [B, rows, width] in the CALLER's row order.

    The plain call goes through `Flux.forward`; the taps come from the same evaluation through the Python-ordered plan
    (FluxEngine.eval_once(..., taps=..., concat=False), Flux._forward_twin's route), whose output must equal the plain call's bit
    for bit.  Row order: the engine runs every stream VALID ROWS FIRST (model.MaskLayout: a stable sort of each sample's text rows
    and image rows by mask), so its buffers hold, samples stacked, XT [B * T, D] / XI [B * N, D] / X [B * (T + N), D] (per sample
    text rows, then image rows) in that kernel order.  Kernel-order rows go back to the caller's order with the layout's own
    inverse permutations: `txt_rows_back` for txt_in / double.i.txt, `img_rows_back` for img_in / double.i.img / the output, and
    for single.i the first T rows of each sample with the former and the other N with the latter."""
    from visualcloze_amd.model import MaskLayout
    img = torch.cat((inp["x"], inp["cond"]), -1)
    plain = m(img.to(DEV, torch.bfloat16), timesteps=t.to(DEV), **_args(inp))
    torch.cuda.synchronize()
    eng = m.engine()
    B, N = inp["x"].shape[:2]
    T, D = inp["txt"].shape[1], m.hidden_size
    assert B <= eng.MAX_BATCH
    bf = lambda a: a.to(DEV, torch.bfloat16).contiguous()  # noqa: E731
    lay = MaskLayout(inp["txt_mask"], inp["img_mask"], B, T, N)
    sl = slice(0, B)
    ws = eng.workspace(T, N, 1, B)
    eng.prepare_sample(ws, bf(lay.txt_rows(inp["txt"], sl)), bf(inp["y"]), inp["guidance"].to(DEV), False,
                       lay.img_rows(inp["img_ids"], sl), lay.txt_rows(inp["txt_ids"], sl), t.float().reshape(1, B), lay.kv_len(sl),
                       kv_gap=lay.kv_gap(sl))
    ws.XIN.copy_(bf(lay.img_rows(img, sl)).reshape(B * N, -1))
    taps = {}
    eng.eval_once(ws, None, euler=False, taps=taps, concat=False)
    torch.cuda.synchronize()
    tapped = lay.img_rows_back(ws.V.reshape(B, N, -1), sl)
    assert plain.dtype == torch.bfloat16 and torch.equal(tapped, plain), "the tapped evaluation is not the plain call's"
    out = {"out": plain.float().cpu()}
    for name, v in taps.items():
        if name.startswith("single."):
            j = v.reshape(B, T + N, D)
            out[name] = torch.cat((lay.txt_rows_back(j[:, :T], sl), lay.img_rows_back(j[:, T:], sl)), dim=1)
        elif name == "txt_in" or name.endswith(".txt"):
            out[name] = lay.txt_rows_back(v.reshape(B, T, D), sl)
        else:
            out[name] = lay.img_rows_back(v.reshape(B, N, D), sl)
    assert sorted(out) == sorted(["out"] + RV.tap_names())
    return out


def judge(m, case, variant):
    """Flux.forward and every tap of CASES[case] by region; every tensor is judged (and logged) before the first failure is raised"""
    inp, t, regs, runs = RV.oracle_runs(case)
    eng = m.engine()
    eng.attn_variant = variant
    try:
        got = hip_forward_and_taps(m, inp, t)
    finally:
        eng.attn_variant = None
    failures, worst = [], 0.0
    for name in ["out"] + RV.tap_names():
        assert torch.isfinite(got[name]).all(), (case, name)
        try:
            worst = max(worst, RV.assert_rows_within_bf16_noise(got[name], runs["o16"][name], runs["o32"][name], regs.for_tensor(name),
                                                                f"{case}, attention {variant}: {name}"))
        except AssertionError as e:
            failures.append(str(e))
    from tests.helpers import parity_log
    parity_log(f"[rows] {case}, attention {variant}: largest region ratio {'> ROW_M' if failures else f'{worst:.3f}'}, "
               f"{regs.share_left_out():.3f} of the rows left out")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", ["b1", "b2_ragged", "b3_lengths"])
def test_rows_of_the_golden_inputs(model, case):
    """The inputs of test_forward_b1_vs_golden_and_oracle and test_forward_b2_ragged_vs_golden (sample 1 right-padded by 12 image
    rows: its padded rows are a region of their own), and B = 3 with three lengths, three timesteps and three guidance values, so
    that a per-sample row of the modulation, gate, RoPE or kv_len tables cannot be right by accident.
    Measured on the MI355X (largest region ratio of the case, and where; ROW_M = 3): b1 1.030 (single.1 / txt live), output 1.014;
    b2_ragged 1.029 (single.1 / txt live[1]), output 1.025 / 0.942 and its padded rows 1.000; b3_lengths 1.110 (single.1 /
    txt live[1]), output 1.021 / 0.962 / 0.987, every padded region 0.998 - 1.000.  img_in and txt_in: 1.000 everywhere."""
    judge(model, case, None)


@pytest.mark.parametrize("variant", [3, 12])
@pytest.mark.parametrize("case", ["general", "notext"])
def test_rows_under_general_masks(model, case, variant):
    """Holes in both streams (the golden file's masks) and a sample without any text (seed 13), through both attention kernels:
    the valid-first reorder, kv_len + one gap per sample, the scatter back.  The masked rows of the streams with holes are left
    out (0.100 / 0.025 of the rows); the right-padded text rows (sample 0 of `general`, all of sample 1's text in `notext`) count.
    Measured on the MI355X: general 1.089 (attention 3) / 1.116 (12), both at the output's img live[1]; notext 1.046 / 1.055
    (single.1 / double.0.img, img live[1]); the padded text regions 0.993 - 1.000."""
    judge(model, case, variant)


@pytest.mark.parametrize("variant", [None, 12])
@pytest.mark.parametrize("case", ["T1", "L255", "L256", "L257", "L326"])
def test_rows_at_seam_and_tile_edges(model, case, variant):
    """A text stream of ONE row; the seam at row 63 / 64 / 65 with the sequence ending at 255 / 256 / 257; and L = 326 from three
    grid rows of unequal latent sizes with the seam at row 40, inside a tile, across the 64-, 128- and 256-row edges - with the
    kernel the engine picks by size (the 32-queries-per-wave one) and with the one-wave-per-SIMD kernel the product runs (12).
    Measured on the MI355X (by size / 12): T1 1.085 / 1.138 (the one text row after double.1 / single.1), L255 1.032 / 1.033,
    L256 1.056 / 1.070, L257 1.065 / 1.055, L326 1.021 / 1.034; at the output 0.94 - 1.07."""
    judge(model, case, variant)


def test_rows_of_the_fused_sampler_under_general_masks(model):
    """The fused Euler sampler, 4 points (3 evaluations in one captured loop, the state kept in kernel row order and scattered back
    at the end) on the inputs of test_sampler_general_masks_vs_oracle: the final state per row against O.sample_euler in fp32,
    yardstick = O.sample_euler in bf16, bound ROW_M_TRAJ (derived for this trajectory, tests/rowview.py).
    Measured on the MI355X: img live[0] 0.979, img live[1] 0.969 (ROW_M_TRAJ = 3)."""
    from visualcloze_amd.transport import Sampler, create_transport
    m = model
    inp, regs, runs = RV.oracle_sampler_runs()
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=RV.SAMPLER_POINTS, do_shift=True, time_shifting_factor=1)
    kw = dict(_args(inp), cond=inp["cond"].to(DEV, torch.bfloat16))
    fused = fn(inp["x"].to(DEV, torch.bfloat16), m.forward, kw)[-1].float().cpu()
    assert fused.shape == runs["o32"].shape and torch.isfinite(fused).all()
    RV.assert_rows_within_bf16_noise(fused, runs["o16"], runs["o32"], regs.img, f"fused sampler, {RV.SAMPLER_POINTS} points, general masks",
                                     m=RV.ROW_M_TRAJ)
