"""tests/rowview.py on a machine without a GPU: the instrument is shown to work before it judges a kernel (as test_budget_cpu.py
does for tests/budget.py).  The oracle's two legitimate bf16 executions pass each other's yardstick on every input set of
test_rowview_gpu.py, output and every tap; results that are wrong in ONE row fail it - among them one that today's whole-tensor
thresholds (TOL_GOLDEN / TOL_ORACLE of test_model_gpu.py) accept."""
import contextlib

import pytest
import torch

import oracle.flux_oracle as O
from tests import rowview as RV
from tests.helpers import rel_l2

TOL_GOLDEN, TOL_ORACLE = 3e-2, 1.5e-2          # tests/test_model_gpu.py


# ------------------------------------------------------------------------------------------------ the region builder
def _check_partition(txt_mask, img_mask):
    regs = RV.RowRegions(txt_mask, img_mask)
    B, T, N = regs.B, regs.T, regs.N
    for regions, mask, rows in ((regs.txt, txt_mask, T), (regs.img, img_mask, N),
                                (regs.joint, torch.cat((txt_mask, img_mask), 1), T + N)):
        seen = torch.zeros(B, rows, dtype=torch.int32)
        for r in regions:
            assert len(r.rows) > 0 and len(set(r.rows)) == len(r.rows)
            seen[r.sample, list(r.rows)] += 1
            live = mask[r.sample, list(r.rows)].bool()
            assert bool(live.all()) if r.name.endswith("live") else not bool(live.any()), r     # a region never mixes live and masked rows
        assert int(seen.max()) <= 1                                                             # disjoint
        assert bool((seen[mask.bool()] == 1).all())                                             # every live row in exactly one region
    # what is left out: the masked rows of streams whose mask has holes, nothing else
    holes = 0
    for m in (txt_mask, img_mask):
        for b in range(B):
            n = int(m[b].sum())
            if not bool(m[b, :n].all()):
                holes += int((m[b] == 0).sum())
    assert regs.left_out_txt + regs.left_out_img == holes == regs.holes_txt + regs.holes_img
    covered = sum(len(r.rows) for r in regs.joint)
    assert covered + holes == B * (T + N)
    assert regs.share_left_out() == holes / (B * (T + N))
    return regs


def test_regions_partition_the_rows():
    shares = {}
    for case, make in list(RV.CASES.items()) + [("sampler", lambda: (RV.sampler_inputs(), None))]:
        inp, _ = make()
        shares[case] = _check_partition(inp["txt_mask"], inp["img_mask"]).share_left_out()
    # only the inputs whose masks have holes leave rows out, and exactly those rows
    assert {k for k, v in shares.items() if v > 0} == {"general", "notext", "sampler"}
    assert shares["general"] == (3 + 5) / 80 and shares["notext"] == 2 / 80 and shares["sampler"] == (2 + 3) / 80
    g = torch.Generator().manual_seed(3)
    for _ in range(50):
        B, T, N = (int(torch.randint(1, 5, (1,), generator=g)) for _ in range(3))
        _check_partition((torch.rand(B, T, generator=g) > 0.4).int(), (torch.rand(B, N, generator=g) > 0.4).int())


def test_region_kinds():
    txt = torch.tensor([[1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]])
    img = torch.tensor([[1, 1, 1], [1, 1, 0], [0, 1, 1]])
    regs = RV.RowRegions(txt, img)
    R = RV.Region
    assert regs.txt == [R("txt live", 0, (0, 1)), R("txt padded", 0, (2, 3)), R("txt live", 1, (0, 2)), R("txt padded", 2, (0, 1, 2, 3))]
    assert regs.img == [R("img live", 0, (0, 1, 2)), R("img live", 1, (0, 1)), R("img padded", 1, (2,)), R("img live", 2, (1, 2))]
    assert regs.joint[:4] == regs.txt and regs.joint[4] == R("img live", 0, (4, 5, 6))
    assert (regs.left_out_txt, regs.left_out_img) == (2, 1)
    assert regs.for_tensor("single.0") is regs.joint and regs.for_tensor("double.1.txt") is regs.txt
    assert regs.for_tensor("txt_in") is regs.txt and regs.for_tensor("img_in") is regs.img and regs.for_tensor("out") is regs.img


def test_assertion_names_the_row():
    o32 = torch.zeros(2, 4, 8)
    o16 = o32 + 0.01
    got = o16.clone()
    regs = RV.RowRegions(torch.ones(2, 1), torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]])).img
    assert RV.assert_rows_within_bf16_noise(got, o16, o32, regs, "toy") == pytest.approx(1.0)
    got[1, 3] *= RV.ROW_M + 0.5
    with pytest.raises(AssertionError, match=r"region 'img padded' of sample 1, row 3: .* ratio 3\.500 > 3\.0"):
        RV.assert_rows_within_bf16_noise(got, o16, o32, regs, "toy")
    got[1, 3] = o16[1, 3] * (RV.ROW_M - 0.01)
    RV.assert_rows_within_bf16_noise(got, o16, o32, regs, "toy")


# ------------------------------------------------------------------------------------------------ the reference passes
def test_row_m_is_what_the_two_bf16_executions_give():
    """ROW_M and ROW_M_TRAJ follow from the derivation in tests/rowview.py's docstring: twice the largest two-way ratio, rounded up
    to one significant digit (here: anything in (1, 1.5] gives 3)"""
    single, traj = RV.derive_row_m(verbose=lambda s: None)
    print(f"\nlargest two-way region ratio: single evaluation {single:.3f}, sampler {traj:.3f}")
    assert 1.0 < single <= 1.5 and RV.ROW_M == 3.0
    assert 1.0 < traj <= 1.5 and RV.ROW_M_TRAJ == 3.0


@pytest.mark.parametrize("case", list(RV.CASES))
def test_the_reference_passes_both_ways(case):
    _, _, regs, runs = RV.oracle_runs(case)
    for name in ["out"] + RV.tap_names():
        r = regs.for_tensor(name)
        RV.assert_rows_within_bf16_noise(runs["o16ref"][name], runs["o16"][name], runs["o32"][name], r, f"{case} {name}: ref LoRA vs merged")
        RV.assert_rows_within_bf16_noise(runs["o16"][name], runs["o16ref"][name], runs["o32"][name], r, f"{case} {name}: merged vs ref LoRA")


def test_the_reference_sampler_passes_both_ways():
    _, regs, runs = RV.oracle_sampler_runs()
    RV.assert_rows_within_bf16_noise(runs["o16ref"], runs["o16"], runs["o32"], regs.img, "sampler: ref LoRA vs merged", m=RV.ROW_M_TRAJ)
    RV.assert_rows_within_bf16_noise(runs["o16"], runs["o16ref"], runs["o32"], regs.img, "sampler: merged vs ref LoRA", m=RV.ROW_M_TRAJ)


# ------------------------------------------------------------------------------------------------ mutants fail
def _fails_at(got, o16, o32, regions, what, row, sample=0):
    with pytest.raises(AssertionError) as e:
        RV.assert_rows_within_bf16_noise(got, o16, o32, regions, what)
    assert f"of sample {sample}, row {row}:" in str(e.value), str(e.value)
    return float(str(e.value).split("ratio ")[1].split(" ")[0])


def test_one_scaled_row_passes_rel_l2_and_fails_the_row_view():
    """THE blind spot: row 5 of the bf16 oracle's own B = 1 output times 1.05 passes both whole-tensor thresholds of
    test_model_gpu.py and fails the row view (measured: rel-L2 1.27e-2 vs fp32, 1.05e-2 vs bf16; the row at 5.8 x the yardstick, and
    5.6 - 6.3 x for rows 0, 11 and 23)."""
    _, _, regs, runs = RV.oracle_runs("b1")
    o32, o16 = runs["o32"]["out"], runs["o16"]["out"]
    got = o16.clone()
    got[0, 5] *= 1.05
    e32, e16 = rel_l2(got, o32), rel_l2(got, o16)
    ratio = _fails_at(got, o16, o32, regs.img, "row 5 x 1.05", 5)
    print(f"\nrow 5 x 1.05: rel-L2 vs fp32 oracle {e32:.3e}, vs bf16 oracle {e16:.3e}, row-view ratio {ratio:.2f}")
    assert e32 < TOL_GOLDEN and e16 < TOL_ORACLE
    assert ratio > 1.5 * RV.ROW_M


def test_where_detection_of_a_scaled_row_ends():
    """A row scaled by 1 + s has error ~ s |row| on top of its own bf16 error, against a yardstick of ~ 0.9 % of |row|: measured on
    row 5, s = 0.05 is 5.8 x the yardstick and 0.03 is 3.6 x (caught); 0.025 is 3.0 x (on the bound), 0.02 is 2.5 x and 0.01 is
    1.4 x (inside ROW_M = 3: not caught).  Detection ends at 2.5 % of one row here, i.e. at ROW_M times the largest bf16 error of
    the row's region."""
    _, _, regs, runs = RV.oracle_runs("b1")
    o32, o16 = runs["o32"]["out"], runs["o16"]["out"]
    for s, caught in ((0.05, True), (0.03, True), (0.02, False), (0.01, False)):
        got = o16.clone()
        got[0, 5] *= 1 + s
        if caught:
            _fails_at(got, o16, o32, regs.img, f"row 5 x {1 + s}", 5)
        else:
            RV.assert_rows_within_bf16_noise(got, o16, o32, regs.img, f"row 5 x {1 + s}")


@pytest.mark.parametrize("case,sample,row", [("b1", 0, 23), ("b2_ragged", 1, 11), ("L257", 0, 0)])
def test_a_row_replaced_by_its_neighbour_fails(case, sample, row):
    """the last row, the last live row of a ragged sample, the first row behind the seam: each replaced by the row next to it"""
    _, _, regs, runs = RV.oracle_runs(case)
    for name in ("out", "double.1.img"):
        o32, o16 = runs["o32"][name], runs["o16"][name]
        got = o16.clone()
        got[sample, row] = o16[sample, row - 1 if row else 1]
        ratio = _fails_at(got, o16, o32, regs.for_tensor(name), f"{case} {name} row {row} := its neighbour", row, sample)
        assert ratio > 10 * RV.ROW_M           # an unrelated row is O(1) wrong against a yardstick of O(1e-2)


# Three wrong results made INSIDE the oracle, by patching its functions for the length of a test (as the tests patch O.compute_vec)


@contextlib.contextmanager
def _patched(name, fn):
    orig = getattr(O, name)
    setattr(O, name, fn(orig))
    try:
        yield
    finally:
        setattr(O, name, orig)


def drop_one_key(block, sample, head, query):
    """the `block`-th attention call of the evaluation loses, for ONE query row of ONE head, the key it weighs most"""
    calls = []

    def wrap(orig):
        def sdpa(q, k, v, P, kv_len=None):
            out = orig(q, k, v, P, kv_len)
            calls.append(1)
            if len(calls) - 1 == block:
                assert kv_len is None
                D = q.shape[-1]
                s = (q[sample, head, query].float() @ k[sample, head].float().t()) * D ** -0.5
                keep = torch.ones_like(s, dtype=torch.bool)
                keep[int(s.argmax())] = False
                o = torch.softmax(s[keep], dim=-1) @ v[sample, head][keep].float()
                out[sample, query, head * D:(head + 1) * D] = P.r(o)
            return out
        return sdpa
    return _patched("sdpa", wrap)


def rope_from_next(sample, joint_row):
    """one row of the RoPE table holds the entry of the next position"""
    def wrap(orig):
        def rope_cos_sin(ids, axes_dim, theta):
            cs = orig(ids, axes_dim, theta).clone()
            cs[sample, joint_row] = cs[sample, joint_row + 1]
            return cs
        return rope_cos_sin
    return _patched("rope_cos_sin", wrap)


def seam_row_gets_text_modulation(block):
    """in DoubleStreamBlock `block` the first image row behind the seam is LayerNorm-modulated with the TEXT stream's shift / scale"""
    def wrap(orig):
        def double_block(sd, pfx, img, txt, vec, cs, G, P, kv_len=None, ls=1.0):
            if pfx != f"double_blocks.{block}":
                return orig(sd, pfx, img, txt, vec, cs, G, P, kv_len, ls)
            tm = O.modulation(sd, pfx + ".txt_mod", vec, 6, P, ls)
            img_calls = []                                   # modulate is called img, txt, img, txt

            def wrap_mod(orig_mod):
                def modulate(x, shift, scale, P):
                    y = orig_mod(x, shift, scale, P)
                    img_calls.append(1)
                    k = len(img_calls) - 1
                    if k % 2 == 0:                           # an image-stream call: (shift1, scale1) then (shift2, scale2)
                        y = y.clone()
                        y[:, :1] = orig_mod(x[:, :1], tm[0 if k == 0 else 3], tm[1 if k == 0 else 4], P)
                    return y
                return modulate
            with _patched("modulate", wrap_mod):
                return orig(sd, pfx, img, txt, vec, cs, G, P, kv_len, ls)
        return double_block
    return _patched("double_block", wrap)


def _mutant(ctx, case="b1"):
    """(the bf16 / merged oracle run under the patch `ctx`, regions, the unpatched runs)"""
    inp, t, regs, runs = RV.oracle_runs(case)
    with ctx:
        mut = RV.oracle_forward(inp, t, "bf16", "merged")
    assert O.sdpa is _ORIG["sdpa"] and O.rope_cos_sin is _ORIG["rope_cos_sin"] and O.double_block is _ORIG["double_block"] \
        and O.modulate is _ORIG["modulate"]
    for name in ("img_in", "txt_in"):                            # upstream of every patch: untouched
        assert torch.equal(mut[name], runs["o16"][name])
    return mut, regs, runs


def _ratio(mut, runs, regs, name, region="img live"):
    """(worst row, ratio) of the named region of sample 0"""
    for reg, row, _, _, ratio in RV.region_ratios(mut[name], runs["o16"][name], runs["o32"][name], regs.for_tensor(name)):
        if reg.name == region and reg.sample == 0:
            return row, ratio
    raise KeyError(region)


_ORIG = {n: getattr(O, n) for n in ("sdpa", "rope_cos_sin", "double_block", "modulate")}
T_B1 = 16                                                        # text rows of tiny_inputs(B=1): joint row = 16 + image row


@pytest.mark.parametrize("head,row,at_output", [(0, 7, True), (0, 0, False)])
def test_mutant_one_key_dropped_for_one_query_row(head, row, at_output):
    """DoubleStreamBlock 1, one head, one image query row: its strongest key of 40 is dropped from the softmax.  Neither
    whole-tensor threshold sees either case (asserted).  Row 7 / head 0 (the key weighs 0.165): 5.2 x the yardstick at the output,
    7.9 x at the block's own tap - caught at both.  Row 0 / head 0 (the key weighs 0.093, about the median of 0.13): 4.5 x at the
    block's tap, 3.8 x after the last SingleStream block, but only 2.6 x at the output - a key of average weight in ONE of two
    heads of ONE of four blocks does NOT move its output row beyond ROW_M; it is the taps that catch it."""
    mut, regs, runs = _mutant(drop_one_key(block=1, sample=0, head=head, query=T_B1 + row))
    e32, e16 = rel_l2(mut["out"], runs["o32"]["out"]), rel_l2(mut["out"], runs["o16"]["out"])
    r_out, r_tap, r_last = (_ratio(mut, runs, regs, n) for n in ("out", "double.1.img", "single.1"))
    print(f"\nkey dropped, head {head} row {row}: rel-L2 vs fp32 {e32:.3e}, vs bf16 {e16:.3e}; row-view ratio at the output {r_out[1]:.2f}, "
          f"double.1.img {r_tap[1]:.2f}, single.1 {r_last[1]:.2f}")
    assert e32 < TOL_GOLDEN and e16 < TOL_ORACLE                 # today's thresholds accept it
    assert torch.equal(mut["double.0.img"], runs["o16"]["double.0.img"])
    _fails_at(mut["double.1.img"], runs["o16"]["double.1.img"], runs["o32"]["double.1.img"], regs.img, "key dropped: double.1.img", row)
    _fails_at(mut["single.1"], runs["o16"]["single.1"], runs["o32"]["single.1"], regs.joint, "key dropped: single.1", T_B1 + row)
    if at_output:
        _fails_at(mut["out"], runs["o16"]["out"], runs["o32"]["out"], regs.img, "key dropped: output", row)
    else:
        assert r_out == (row, r_out[1]) and 1.5 < r_out[1] < r_tap[1]      # its row is the worst one, and still inside ROW_M there


@pytest.mark.parametrize("row,caught", [(11, True), (7, False)])
def test_mutant_rope_row_from_the_next_position(row, caught):
    """One image row's RoPE entry is the next row's, in every block.  Row 11 is the last token of the first grid row, its successor
    the first token of the second (ids (1, 1, 5) -> (2, 0, 0)): 5.9 x the yardstick at the output, 6.7 - 8.5 x at the taps; rel-L2
    1.5e-2 vs fp32 passes TOL_GOLDEN (asserted), 1.44e-2 vs bf16 sits on TOL_ORACLE = 1.5e-2 (printed, not asserted).  Row 7 has its
    successor one step along x ((1, 1, 1) -> (1, 1, 2)), a rotation by one position of the 28 x-frequencies only: 2.4 x at the
    output and 3.0 - 3.4 x at the taps - this one does NOT move its row clearly beyond ROW_M, and no threshold of today sees it."""
    mut, regs, runs = _mutant(rope_from_next(sample=0, joint_row=T_B1 + row))
    e32, e16 = rel_l2(mut["out"], runs["o32"]["out"]), rel_l2(mut["out"], runs["o16"]["out"])
    r_out = _ratio(mut, runs, regs, "out")
    print(f"\nRoPE row {row} from row {row + 1}: rel-L2 vs fp32 {e32:.3e}, vs bf16 {e16:.3e}; row-view ratio at the output {r_out[1]:.2f}, "
          + ", ".join(f"{n} {_ratio(mut, runs, regs, n)[1]:.2f}" for n in ("double.0.img", "double.1.img", "single.1")))
    assert e32 < TOL_GOLDEN
    if caught:
        for name in ("out", "double.0.img", "double.1.img"):
            _fails_at(mut[name], runs["o16"][name], runs["o32"][name], regs.img, f"RoPE row {row}: {name}", row)
    else:
        assert e16 < TOL_ORACLE
        assert r_out[0] == row and 1.5 < r_out[1] < RV.ROW_M


def test_mutant_seam_row_with_the_text_streams_modulation():
    """DoubleStreamBlock 1 LayerNorm-modulates the first image row behind the seam with the TEXT stream's shift / scale (both
    modulations of the block).  13 x the yardstick at the output, 22 x at the block's tap, 19 x after the last block.  One row of
    24 this wrong IS seen by TOL_ORACLE here (rel-L2 2.6e-2 vs bf16, asserted; 2.6e-2 vs fp32 is just inside TOL_GOLDEN = 3e-2,
    printed); at N = 192 the same row error is 2.6e-2 / sqrt(8) = 9e-3 and passes both."""
    mut, regs, runs = _mutant(seam_row_gets_text_modulation(block=1))
    e32, e16 = rel_l2(mut["out"], runs["o32"]["out"]), rel_l2(mut["out"], runs["o16"]["out"])
    print(f"\nseam row: rel-L2 vs fp32 {e32:.3e}, vs bf16 {e16:.3e}; row-view ratio at the output {_ratio(mut, runs, regs, 'out')[1]:.2f}, "
          f"double.1.img {_ratio(mut, runs, regs, 'double.1.img')[1]:.2f}, single.1 {_ratio(mut, runs, regs, 'single.1')[1]:.2f}")
    assert e16 > TOL_ORACLE
    assert torch.equal(mut["double.0.img"], runs["o16"]["double.0.img"])
    for name in ("out", "double.1.img"):
        assert _fails_at(mut[name], runs["o16"][name], runs["o32"][name], regs.img, f"seam row: {name}", 0) > 2 * RV.ROW_M
    _fails_at(mut["single.1"], runs["o16"]["single.1"], runs["o32"]["single.1"], regs.joint, "seam row: single.1", T_B1)
    # the text rows and the other image rows stay inside the bound: the view points at the one row
    RV.assert_rows_within_bf16_noise(mut["double.1.txt"], runs["o16"]["double.1.txt"], runs["o32"]["double.1.txt"], regs.txt, "seam row: double.1.txt")
