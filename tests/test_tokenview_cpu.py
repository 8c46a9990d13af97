"""tests/tokenview.py on a machine without a GPU: the instrument is shown to work before it judges a kernel (as test_rowview_cpu.py
does for tests/rowview.py).  On every case of tests/test_text_tokens_gpu.py the oracle's two legitimate bf16 executions ("bf16" and
"bf16_fused") pass with each other as the yardstick; the bf16 oracle's output with ONE row zeroed, replaced by its neighbour or
scaled by 1.25 fails at EVERY row, and so does `pooled` - while the whole-tensor rel-L2 line of tests/test_text_gpu.py accepts a
scaled row."""
import numpy as np
import pytest
import torch

from oracle import text_oracle as TO
from tests import tokenview as TV
from tests.procedural import TINY_CLIP, TINY_T5

G = np.load(TV.GOLDEN)
ALL = list(TV.CASES)
GOLDEN_CASES = ["t5_a", "t5_b", "clip_a", "clip_b"]


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def old_line_passes(out, o16, o32):
    """the whole-tensor assertion of tests/test_text_gpu.py and tests/test_text_handle_gpu.py"""
    return rel_l2(out, o32) <= 3.0 * rel_l2(o16, o32) + 2e-3


# ------------------------------------------------------------------------------------------------ regions
def test_regions_leave_no_live_row_out():
    for name in ALL:
        case = TV.CASES[name]()
        regs = case.regions()
        assert TV.share_left_out(regs, case.L) == 0.0, name
        assert sorted(r for reg in regs for r in reg.rows) == list(range(case.L)), name
    assert [r.name for r in TV.t5_regions(192)] == ["tile 0 first", "tile 0 last", "tile 1 first", "tile 1 last", "tile 2 first", "tile 2 last",
                                                    "interior"]
    assert [r.rows for r in TV.t5_regions(128)[:4]] == [(0,), (63,), (64,), (127,)] and len(TV.t5_regions(128)[4].rows) == 124
    R = TV.Region
    assert TV.clip_regions(7, 3) == [R("row 0", (0,)), R("eos", (3,)), R("last", (6,)), R("rest", (1, 2, 4, 5))]
    assert TV.clip_regions(4, 0) == [R("row 0", (0,)), R("last", (3,)), R("rest", (1, 2))]          # EOS first: it is row 0
    assert TV.clip_regions(4, 3) == [R("row 0", (0,)), R("eos", (3,)), R("rest", (1, 2))]           # EOS last
    assert TV.share_left_out([R("a", (0, 1))], 4) == 0.5
    with pytest.raises(AssertionError):
        TV.share_left_out([R("a", (0, 1)), R("b", (1,))], 4)


def test_the_cases_are_the_shapes_the_issue_names():
    c = {n: TV.CASES[n]() for n in ALL}
    assert {c[n].L for n in ALL if c[n].kind == "t5"} == {64, 128, 192} and {c[n].L for n in ALL if c[n].kind == "clip"} >= {7, 24, 64, 77}
    p = c["t5_192_prompt"].ids
    assert p[5] == 1 and set(p[6:]) == {0} and 0 not in p[:5] and 1 not in p[:5]
    eos = TINY_CLIP["eos_token_id"]
    assert (c["clip_64_first"].eos, c["clip_24_mid"].eos, c["clip_64_last"].eos, c["clip_77_last"].eos, c["clip_7_last"].eos) == (0, 9, 63, 76, 6)
    assert c["clip_77_eospad"].eos == 20 and set(c["clip_77_eospad"].ids[20:]) == {eos}
    assert c["clip_64_first"].cfg["max_position_embeddings"] == 77 and c["clip_24_mid"].cfg is TINY_CLIP
    for n in ("t5_outlier", "clip_outlier"):                        # one embedding channel is 2^7 times the others', still exact in bf16
        sd = TV.state_dict(c[n])
        key = "shared.weight" if c[n].kind == "t5" else "text_model.embeddings.token_embedding.weight"
        base = TV._base_sd(c[n].kind, c[n].wide_positions)[key]
        assert torch.equal(sd[key][:, 5], base[:, 5] * 128) and torch.equal(sd[key][:, :5], base[:, :5])
        assert torch.equal(sd[key].to(torch.bfloat16).float(), sd[key]) and float(base[:, 5].abs().max()) <= 1.5


# ------------------------------------------------------------------------------------------------ the oracle's modes
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_fp32_oracle_is_the_transformers_golden(name):
    """why new lengths need no new goldens: measured 6e-7"""
    _, _, runs = TV.oracle_runs(name)
    if name.startswith("t5"):
        assert rel_l2(runs["o32"][0], G[name + "_fp32"]) < 1e-5
    else:
        assert rel_l2(runs["o32"][0], G[name + "_hidden_fp32"]) < 1e-5 and rel_l2(runs["o32"][1], G[name + "_pooled_fp32"]) < 1e-5


def test_the_fused_mode_leaves_the_other_two_alone():
    _, _, runs = TV.oracle_runs("t5_a")
    o16, o16f = runs["o16"][0], runs["o16f"][0]
    noise = rel_l2(G["t5_a_refbf16"], G["t5_a_fp32"])                # transformers' own bf16 run: "bf16" is pinned to it as before
    assert rel_l2(o16, G["t5_a_fp32"]) < 2.0 * noise + 1e-3 and rel_l2(o16, G["t5_a_refbf16"]) < 2.0 * noise + 1e-3
    assert not torch.equal(o16, o16f) and rel_l2(o16f, G["t5_a_fp32"]) < 2.0 * noise + 1e-3
    for name in ("t5_a", "clip_a"):                                  # every result of a rounding mode is bf16-valued; fp32 is not
        _, _, runs = TV.oracle_runs(name)
        for k in ("o16", "o16f"):
            assert torch.equal(runs[k][0].to(torch.bfloat16).float(), runs[k][0])
        assert not torch.equal(runs["o32"][0].to(torch.bfloat16).float(), runs["o32"][0])
        assert not torch.equal(runs["o16"][0], runs["o16f"][0])
    with pytest.raises(ValueError):
        TO.t5_encode(TV.state_dict(TV.CASES["t5_a"]()), torch.tensor(G["t5_a_ids"]), TINY_T5, "bf16_merged")


def test_a_depth_prefix_is_the_shallower_model():
    """num_layers = the full depth changes nothing; a prefix differs from it"""
    for name in ("t5_depth2", "clip_depth2"):
        case, _, runs = TV.oracle_runs(name)
        full = TV.oracle_run(TV.Case(case.kind, case.ids, case.wide_positions), "fp32")[0]
        assert torch.equal(full, runs["o32"][0])
        assert not torch.equal(TV.oracle_runs(name.replace("2", "1"))[2]["o32"][0], full)


# ------------------------------------------------------------------------------------------------ the margin
def test_token_m_is_what_the_two_bf16_executions_give():
    """TOKEN_M follows from the derivation in tests/tokenview.py's docstring: twice the largest two-way ratio of the encoder's cases,
    rounded up to one significant digit"""
    worst = TV.derive_token_m(verbose=lambda s: None)
    print(f"\nlargest two-way region ratio: T5 {worst['t5']:.3f}, CLIP {worst['clip']:.3f}")
    assert {k: TV.margin_from(v) for k, v in worst.items()} == TV.TOKEN_M == {"t5": 5.0, "clip": 3.0}
    assert [TV.margin_from(x) for x in (1.0, 1.26, 1.5, 1.51, 2.39, 2.5, 4.9, 5.1)] == [2, 3, 3, 4, 5, 5, 10, 20]


@pytest.mark.parametrize("name", ALL + list(TV.WIDTH_CASES))
def test_both_executions_pass_both_ways(name):
    case, regs, runs = TV.oracle_runs(name)
    o32, m = runs["o32"][0], TV.TOKEN_M[case.kind]
    TV.assert_tokens_within_bf16_noise(runs["o16f"][0], runs["o16"][0], o32, regs, f"{name}: fused vs bf16", m,
                                       pooled=TV.pooled_triple(runs, runs["o16f"][1], "o16"))
    TV.assert_tokens_within_bf16_noise(runs["o16"][0], runs["o16f"][0], o32, regs, f"{name}: bf16 vs fused", m,
                                       pooled=TV.pooled_triple(runs, runs["o16"][1], "o16f"))
    # ... and the whole-tensor line of tests/test_text_gpu.py alongside
    assert old_line_passes(runs["o16f"][0], runs["o16"][0], o32) and old_line_passes(runs["o16"][0], runs["o16f"][0], o32)


# ------------------------------------------------------------------------------------------------ mutants fail
def neighbour(case, r):
    """The stale / off-by-one row: r - 1 (r + 1 for row 0).  T5 has no absolute positions, so where that row holds the SAME token
    it is no wrong result: in the fp32 oracle two neighbouring pad rows of the prompt-shaped cases are 0.000 - 0.002 apart (the
    bf16 oracle's own row error there is 0.06 - 0.13), and neighbours with a repeated id among random ids 0.49 - 3.4 (t5_b row 80,
    t5_a row 9) beside a largest legitimate row error of 0.44 - nothing that passes both bf16 executions can tell these from the
    row itself (test_same_token_neighbours_in_t5_are_no_wrong_result).  There the stale row is the nearest row that holds another
    token, the one before first.  CLIP adds a position embedding: always the literal neighbour."""
    nb = r - 1 if r else 1
    if case.kind == "clip" or case.ids[nb] != case.ids[r]:
        return nb
    for d in range(1, case.L):
        for c in (r - d, r + d):
            if 0 <= c < case.L and case.ids[c] != case.ids[r]:
                return c
    raise AssertionError("one token only")


def mutants(case, o16, r):
    """the three wrong rows of the issue, as (name, the row's new value)"""
    return (("zero", torch.zeros_like(o16[r])), ("neighbour", o16[neighbour(case, r)].clone()), ("x 1.25", o16[r] * 1.25))


def test_same_token_neighbours_in_t5_are_no_wrong_result():
    """what `neighbour` says about T5, measured on the fp32 oracle alone: the pad rows of a prompt-shaped case next to another pad row
    are closer to it than a tenth of the yardstick - a result with two of them swapped is a correct result"""
    seen = 0
    for name in ("t5_64_prompt", "t5_128_prompt", "t5_192_prompt"):
        case, _, runs = TV.oracle_runs(name)
        o32 = runs["o32"][0].double()
        y = TV.yardstick(runs["o16"][0], o32)
        pads = [r for r in range(2, case.L) if case.ids[r] == 0 and case.ids[r - 1] == 0]
        d = torch.stack([(o32[r] - o32[r - 1]).norm() for r in pads])
        assert float(d.min()) < 0.1 * y and len(pads) > case.L // 2
        seen += len(pads)
        assert all(case.ids[neighbour(case, r)] != 0 for r in pads)
    assert seen == 53 + 106 + 185
    c = TV.CASES["clip_77_eospad"]()                                  # CLIP: the literal neighbour, same token or not
    assert [neighbour(c, r) for r in (0, 1, 30, 76)] == [1, 0, 29, 75]


@pytest.mark.parametrize("yard", ["o16", "o16f"])
@pytest.mark.parametrize("name", ALL + list(TV.WIDTH_CASES))
def test_a_wrong_row_fails_at_every_row(name, yard):
    """CONDITIONS, not measurements: each row of the subject (one bf16 execution's output, the other being the yardstick) set to zero,
    replaced by its neighbour (the stale / off-by-one row) or scaled by 1.25 is beyond TOKEN_M.  At XXL width the bf16 oracle's own
    row error is 4 - 10 % of a row (2.6 - 6.4 of |row| = 64, yardstick 4.96): a row times 1.25 is only 2.1 times the largest error
    a legitimate execution makes there and cannot be a condition for any margin made by the rule of TOKEN_M; it fails at every
    row from 1.39 on (test_where_detection_of_a_scaled_row_ends).  Zero and the neighbour stay conditions there."""
    case, regs, runs = TV.oracle_runs(name)
    o32, ref, subject = runs["o32"][0].double(), runs[yard][0], runs["o16f" if yard == "o16" else "o16"][0]
    bound = TV.TOKEN_M[case.kind] * TV.yardstick(ref, o32)
    weakest = {}
    for r in range(case.L):
        for what, row in mutants(case, subject, r):
            if name == "t5_xxl" and what == "x 1.25":
                continue
            err = float((row.double() - o32[r]).norm())
            assert err > bound, f"{name}: row {r} {what} passes: error {err:.4e} <= {bound:.4e}"
            weakest[what] = min(weakest.get(what, float("inf")), err / bound)
    print(f"\n{name} (yardstick {yard}): the weakest mutant of each kind is at " + ", ".join(f"{k} {v:.2f}" for k, v in weakest.items()) + " x the bound")


@pytest.mark.parametrize("name", ALL)
def test_a_wrong_row_is_named_by_the_assertion(name):
    """through the assertion itself, at the rows kernels get wrong: the first and the last row of every region"""
    case, regs, runs = TV.oracle_runs(name)
    o32, o16 = runs["o32"][0], runs["o16"][0]
    for reg in regs:
        for r in {reg.rows[0], reg.rows[-1]}:
            for what, row in mutants(case, o16, r):
                got = o16.clone()
                got[r] = row
                with pytest.raises(AssertionError, match=rf"region '{reg.name}', row {r}:"):
                    TV.assert_tokens_within_bf16_noise(got, o16, o32, regs, f"{name} row {r} {what}", TV.TOKEN_M[case.kind])


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("clip")])
def test_a_wrong_pooled_fails(name):
    case, regs, runs = TV.oracle_runs(name)
    o32, o16 = runs["o32"][0], runs["o16"][0]
    assert torch.equal(runs["o16"][1], o16[case.eos]) and torch.equal(runs["o32"][1], o32[case.eos])
    TV.assert_tokens_within_bf16_noise(o16, o16, o32, regs, name, TV.TOKEN_M["clip"], pooled=TV.pooled_triple(runs, runs["o16"][1]))
    for what, row in mutants(case, o16, case.eos):                        # the hidden rows stay right: only `pooled` is wrong
        with pytest.raises(AssertionError, match=r"region 'pooled', row -1:"):
            TV.assert_tokens_within_bf16_noise(o16, o16, o32, regs, f"{name} pooled {what}", TV.TOKEN_M["clip"], pooled=TV.pooled_triple(runs, row))


@pytest.mark.parametrize("name,s", [("t5_a", 1.25), ("t5_b", 1.25), ("clip_a", 1.05), ("clip_b", 1.05)])
def test_one_scaled_row_passes_rel_l2_and_fails_the_token_view(name, s):
    """THE blind spot: the two lines see different things.  The quietest row, the loudest row and the last row of the bf16 oracle's
    own output times s pass the whole-tensor line of tests/test_text_gpu.py and fail the token view."""
    case, regs, runs = TV.oracle_runs(name)
    o32, o16 = runs["o32"][0], runs["o16"][0]
    e = TV.row_errors(o16, o32)
    for r in {int(e.argmin()), int(e.argmax()), case.L - 1}:
        got = o16.clone()
        got[r] *= s
        assert old_line_passes(got, o16, o32), (name, r, rel_l2(got, o32))
        with pytest.raises(AssertionError, match=rf", row {r}:"):
            TV.assert_tokens_within_bf16_noise(got, o16, o32, regs, f"{name} row {r} x {s}", TV.TOKEN_M[case.kind])


def test_where_detection_of_a_scaled_row_ends():
    """the record in tests/tokenview.py's docstring: one row of the bf16 oracle's output times s fails at EVERY row from s = 1.13 (T5) /
    1.02 (CLIP) on, and s = 1.05 (T5) / 1.008 (CLIP) passes somewhere"""
    top = {"t5": 0.0, "clip": 0.0}
    low = {"t5": 9.0, "clip": 9.0}
    _, _, runs = TV.oracle_runs("t5_xxl")
    wide = TV.scale_that_fails(runs["o16"][0], runs["o32"][0], TV.TOKEN_M["t5"])
    print(f"\nXXL width: one row times s fails at every row from s = {float(wide.max()):.3f}, at some row from {float(wide.min()):.3f}")
    assert 1.25 < float(wide.max()) < 1.39
    for name in ALL + ["clip_l"]:
        case, _, runs = TV.oracle_runs(name)
        s = TV.scale_that_fails(runs["o16"][0], runs["o32"][0], TV.TOKEN_M[case.kind])
        r = int(s.argmax())
        got = runs["o16"][0].double().clone()
        got[r] *= float(s[r]) + 1e-6                                # the closed form is the bound itself
        assert float((got[r] - runs["o32"][0][r].double()).norm()) > TV.TOKEN_M[case.kind] * TV.yardstick(runs["o16"][0], runs["o32"][0])
        top[case.kind], low[case.kind] = max(top[case.kind], float(s.max())), min(low[case.kind], float(s.min()))
    print(f"\nsmallest scale that fails at every row: T5 {top['t5']:.3f}, CLIP {top['clip']:.3f}; that fails at some row: T5 {low['t5']:.3f}, "
          f"CLIP {low['clip']:.3f}")
    assert 1.05 < top["t5"] < 1.13 and 1.008 < top["clip"] < 1.02 and low["t5"] > 1.02 and low["clip"] > 1.008


def test_assertion_reports_every_region():
    o32 = torch.zeros(64, 8)
    o16 = o32 + 0.01
    regs = TV.t5_regions(64)
    assert TV.assert_tokens_within_bf16_noise(o16.clone(), o16, o32, regs, "toy", 5.0) == pytest.approx(1.0)
    got = o16.clone()
    got[63] *= 5.5
    with pytest.raises(AssertionError, match=r"region 'tile 0 last', row 63: .* ratio 5\.500 > 5\.0"):
        TV.assert_tokens_within_bf16_noise(got, o16, o32, regs, "toy", 5.0)
    got[63] = o16[63] * 4.99
    TV.assert_tokens_within_bf16_noise(got, o16, o32, regs, "toy", 5.0)
    with pytest.raises(AssertionError, match="live rows outside every region"):
        TV.assert_tokens_within_bf16_noise(o16, o16, o32, regs[:-1], "toy", 5.0)
