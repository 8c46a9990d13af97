"""The handle's un-merged LoRA mode (vc_flux_bind_lora, option lora_mode 1, vc_flux_set_lora_scale) and its per-block taps
(vc_flux_set_tap): the C plan in csrc/flux_engine.hip against its Python-ordered twin (engine.FluxEngine with lora_mode "ref":
same kernels, same order, same operands - bit equality), against the reference's own vectors (tests/golden/tiny_golden.npz,
fullwidth_reference.npz) at the bounds the existing tests hold the twin to, and what the twin cannot do at all: batches, f32
states, rk4, true CFG.  Tiny geometry: T = 16, N = 24, L = 40 (no multiple of 64, far off the 256-row tile), 2 + 2 blocks, LoRA
rank 8 zero-padded to the GEMM's K granularity of 64.

Not compared: `double0_img` / `double0_txt` / `single0` of tiny_golden.npz with the taps double.0.* / single.0.  Those arrays are
the reference's block outputs for SYNTHETIC block inputs (`blk_img_in`, `blk_txt_in`, `mod_vec`: tests/golden/make_golden.py:157-165),
not intermediate activations of a forward, and the handle has no entry point that runs a block on given inputs.  The block-level
comparison with the reference's own activations is the full-width one below (fullwidth_reference.npz samples real taps)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_GOLDEN = 3e-2          # tests/test_model_gpu.py: HIP vs the reference's runs (test_unmerged_lora_mode_vs_reference_bf16_run)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


def _model(lora_mode="ref", ref_plan="handle", scale=None):
    from tests.helpers import tiny_model
    m, _ = tiny_model()
    if scale is not None:
        m.set_lora_scale(scale)
    m.lora_mode, m.ref_plan = lora_mode, ref_plan
    return m


@pytest.fixture(scope="module")
def ref_model():
    """un-merged mode; ref_plan switches between the C handle and the twin over ONE set of prepared weights"""
    return _model()


@pytest.fixture(scope="module")
def merged_model():
    return _model("merged", "python")


def _plan(m, plan):
    m.ref_plan = plan
    return m


def _gap(inp):
    """masks that leave a gap: holes in both streams of sample 0 (MaskLayout moves the valid rows first: kv_len + kv_gap)"""
    inp["txt_mask"][0, [0, 5]] = 0
    inp["img_mask"][0, [1, 2, 9]] = 0
    return inp


def _args(inp, gdt=torch.float32):
    return dict(img_ids=inp["img_ids"].to(DEV), txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), txt_mask=inp["txt_mask"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                guidance=inp["guidance"].to(DEV, gdt))


def _fwd(m, inp, t, gdt=torch.float32):
    img = torch.cat((inp["x"], inp["cond"]), -1).to(DEV, torch.bfloat16)
    out = m(img, timesteps=t.to(DEV), **_args(inp, gdt))
    torch.cuda.synchronize()
    return out


def _taps(m, inp, t, gdt=torch.float32):
    img = torch.cat((inp["x"], inp["cond"]), -1).to(DEV, torch.bfloat16)
    out = m.block_taps(img, timesteps=t.to(DEV), **_args(inp, gdt))
    torch.cuda.synchronize()
    return out


def _twin_taps(m, inp, t, gdt=torch.float32):
    """the twin's eval_once(..., taps=...) on the same evaluation (Flux._forward_bf16's Python-ordered route), its kernel-order
    rows brought back to the caller's order; bf16 device tensors keyed as block_taps keys them"""
    from visualcloze_amd.model import MaskLayout
    eng = m.engine()
    B, N = inp["x"].shape[:2]
    T, D = inp["txt"].shape[1], m.hidden_size
    assert B == 1 or eng.MAX_BATCH >= B
    bf = lambda a: a.to(DEV, torch.bfloat16).contiguous()  # noqa: E731
    lay = MaskLayout(inp["txt_mask"], inp["img_mask"], B, T, N)
    sl = slice(0, B)
    ws = eng.workspace(T, N, 1, B)
    eng.prepare_sample(ws, bf(lay.txt_rows(inp["txt"], sl)), bf(inp["y"]), inp["guidance"].to(DEV, gdt), gdt == torch.bfloat16,
                       lay.img_rows(inp["img_ids"], sl), lay.txt_rows(inp["txt_ids"], sl), t.float().reshape(1, B), lay.kv_len(sl),
                       kv_gap=lay.kv_gap(sl))
    ws.XIN.copy_(bf(lay.img_rows(torch.cat((inp["x"], inp["cond"]), -1), sl)).reshape(B * N, -1))
    taps = {}
    eng.eval_once(ws, None, euler=False, taps=taps, concat=False)
    torch.cuda.synchronize()
    out = {"out": lay.img_rows_back(ws.V.reshape(B, N, -1), sl)}
    for n, v in taps.items():
        v = v.to(DEV, torch.bfloat16)
        if n.startswith("single."):
            j = v.reshape(B, T + N, D)
            out[n] = torch.cat((lay.txt_rows_back(j[:, :T], sl), lay.img_rows_back(j[:, T:], sl)), dim=1)
        elif n == "txt_in" or n.endswith(".txt"):
            out[n] = lay.txt_rows_back(v.reshape(B, T, D), sl)
        else:
            out[n] = lay.img_rows_back(v.reshape(B, N, D), sl)
    return out


def _kw(inp, gdt=torch.float32, rows=slice(None), **more):
    kw = dict(txt=inp["txt"][rows].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"][rows].to(DEV), txt_mask=inp["txt_mask"][rows].to(DEV),
              y=inp["y"][rows].to(DEV, torch.bfloat16), img_ids=inp["img_ids"][rows].to(DEV), img_mask=inp["img_mask"][rows].to(DEV),
              cond=inp["cond"][rows].to(DEV, torch.bfloat16), guidance=inp["guidance"][rows].to(DEV, gdt))
    kw.update(more)
    return kw


def _fn(method, points, **over):
    from visualcloze_amd.transport import Sampler, create_transport
    opts = dict(sampling_method=method, num_steps=points, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    opts.update(over)
    return Sampler(create_transport()).sample_ode(**opts)


# ------------------------------------------------------------------------------------------ 1. + 2. the un-merged forward
def test_unmerged_forward_equals_the_twin_bitwise(ref_model):
    from tests.procedural import tiny_inputs
    m = ref_model
    inp, t = _gap(tiny_inputs(B=1)), torch.tensor([0.7])
    a = _fwd(_plan(m, "handle"), inp, t)
    h = m.handle()
    assert h is not None and h.lora_mode == 1 and len(h._lora) > 30 and m.engine().W.ref is not None
    b = _fwd(_plan(m, "python"), inp, t)
    assert m.handle() is None
    assert a.dtype == torch.bfloat16 and torch.isfinite(a.float()).all()
    assert torch.equal(a, b), f"{(a != b).float().mean().item():.4f} of the elements differ, rel-L2 {rel_l2(a, b):.3e}"
    assert not torch.equal(a, _fwd(_model("merged", "python"), inp, t))         # (and it is not the merged plan that ran)


def test_unmerged_forward_vs_the_reference_vectors(ref_model, golden):
    """flux_b1_ref_bf16: the reference model's own bf16 autocast run with bf16 guidance; flux_b1: its fp32 run.  Bounds: those of
    tests/test_model_gpu.py::test_unmerged_lora_mode_vs_reference_bf16_run for the twin."""
    from tests.procedural import tiny_inputs
    m = _plan(ref_model, "handle")
    inp, t = tiny_inputs(B=1), torch.tensor([0.7])
    e_run = rel_l2(_fwd(m, inp, t, torch.bfloat16), golden["flux_b1_ref_bf16"])
    e_f32 = rel_l2(_fwd(m, inp, t), golden["flux_b1"])
    print(f"\n[tiny, handle lora_mode 1] vs the reference's bf16 run {e_run:.3e}, vs its fp32 run {e_f32:.3e}")
    assert e_run < TOL_GOLDEN and e_f32 < TOL_GOLDEN


# ------------------------------------------------------------------------------------------ 3. taps
@pytest.mark.parametrize("mode", ["ref", "merged"])
def test_block_taps_equal_the_twins_bitwise(ref_model, merged_model, mode):
    from tests.procedural import tiny_inputs
    m = _plan(ref_model, "handle") if mode == "ref" else merged_model
    inp, t = _gap(tiny_inputs(B=1)), torch.tensor([0.7])
    got = _taps(m, inp, t)
    want = _twin_taps(m, inp, t)
    p = m.params
    names = ["img_in", "txt_in"] + [f"double.{i}.{s}" for i in range(p.depth) for s in ("img", "txt")] + [f"single.{i}" for i in range(p.depth_single_blocks)]
    assert p.depth == 2 and p.depth_single_blocks == 2 and sorted(got) == sorted(names + ["out"]) and sorted(want) == sorted(got)
    N, T, D = inp["x"].shape[1], inp["txt"].shape[1], p.hidden_size
    assert got["img_in"].shape == (1, N, D) and got["double.1.txt"].shape == (1, T, D) and got["single.1"].shape == (1, T + N, D)
    for n in names + ["out"]:
        assert got[n].dtype == torch.bfloat16 and got[n].is_cuda
        assert torch.equal(got[n], want[n]), f"{n}: {(got[n] != want[n]).float().mean().item():.4f} of the elements differ"
    assert torch.equal(got["out"], _fwd(m, inp, t))                              # the taps leave the evaluation alone
    assert not torch.equal(got["double.0.img"], got["double.1.img"]) and not torch.equal(got["single.0"], got["single.1"])
    assert not m.handle()._taps                                                  # ... and are cleared afterwards


# ------------------------------------------------------------------------------------------ 4. off = nothing changes
def test_taps_off_leave_the_plan_as_it_was(merged_model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd.transport import solver_time_grid
    m = merged_model
    inp = tiny_inputs(B=2, seed=7)
    inp["img_mask"][1, -12:] = 0
    kw = _kw(inp)
    h = m.handle()
    assert h.lora_mode == 0
    B, N, T, D = 2, inp["x"].shape[1], inp["txt"].shape[1], m.hidden_size
    img = torch.cat((inp["x"], inp["cond"]), -1).to(DEV, torch.bfloat16)
    tg = solver_time_grid(4, N, 0.0, 1, True, 1)
    st = m.engine().stream
    kv = [T + N, T + N - 12]

    def run():
        with torch.cuda.stream(st):
            s = st.cuda_stream
            h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 3, kv_len=kv, stream=s)
            out = torch.empty(B, N, 64, dtype=torch.bfloat16, device=DEV)
            h.forward(img, torch.tensor([0.9, 0.25]), False, out, stream=s)
            x = inp["x"].to(DEV, torch.bfloat16).clone()
            h.sample_euler(x, kw["cond"], tg, True, s)                           # the captured step
            h.sample_begin(x, kw["cond"], tg, True, s)
            n = sum(r["launches"] for r in h.profile(1, s))
            h.sample_end(torch.empty_like(x), s)
        torch.cuda.synchronize()
        return out, x, n

    out0, x0, n0 = run()
    bufs = {"double.1.img": torch.zeros(B * N, D, dtype=torch.bfloat16, device=DEV), "single.0": torch.zeros(B * (T + N), D, dtype=torch.bfloat16, device=DEV)}
    for name, buf in bufs.items():
        assert h.tap_shape(name) == tuple(buf.shape)
        h.set_tap(name, buf)
    out1, x1, n1 = run()
    assert n1 == n0 + len(bufs)                                                  # one copy per tap and evaluation, nothing else
    assert torch.equal(out1, out0) and torch.equal(x1, x0)
    assert all(t.float().abs().sum().item() > 0 for t in bufs.values())
    for name in bufs:
        h.set_tap(name, None)
    out2, x2, n2 = run()
    assert n2 == n0 and torch.equal(out2, out0) and torch.equal(x2, x0)


# ------------------------------------------------------------------------------------------ 5. the scale at run time
def test_lora_scale_at_run_time(ref_model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    m = _plan(ref_model, "handle")
    inp, t = _gap(tiny_inputs(B=1)), torch.tensor([0.7])
    x = inp["x"].to(DEV, torch.bfloat16)
    fn = _fn("euler", 3)
    try:
        a1, tr1 = _fwd(m, inp, t), fn(x, m.forward, _kw(inp))                    # has run, and has captured its step
        h, eng = m.handle(), m.engine()
        m.set_lora_scale(0.5)
        assert m.handle() is h and m.engine() is eng                             # no re-preparation, no new handle
        a2, tr2 = _fwd(m, inp, t), fn(x, m.forward, _kw(inp))
        fresh = _model(scale=0.5)
        b2, trb = _fwd(fresh, inp, t), fn(x, fresh.forward, _kw(inp))
        assert torch.equal(a2, b2) and torch.equal(tr2, trb) and not torch.equal(a1, a2) and not torch.equal(tr1[-1], tr2[-1])
        m.set_lora_scale(0.0)
        assert m.handle() is h
        twin0 = _model(ref_plan="python", scale=0.0)
        assert torch.equal(_fwd(m, inp, t), _fwd(twin0, inp, t))
        # no bf16 value: refused by the library (and by the model before anything changed)
        L = hip.lib()
        assert L.vc_flux_set_lora_scale(h.h, 0.3) == -1 and b"scale" in L.vc_last_error()
        with pytest.raises(hip.VclozeHipError, match="bf16"):
            m.set_lora_scale(0.3)
        assert all(mod.scale == 0.0 for _, mod in m._linears())
        m.set_lora_scale(1.0)
        assert m.handle() is h and torch.equal(_fwd(m, inp, t), a1) and torch.equal(fn(x, m.forward, _kw(inp)), tr1)
    finally:
        for _, mod in m._linears():
            mod.set_scale(1.0)
        m.invalidate_engine()


def test_lora_scale_change_on_a_prepared_handle(ref_model):
    """The handle alone, no model in between: vc_flux_prepare runs txt_in / vector_in / guidance_in with the scale of that moment
    and sample_begin the trajectory's modulation rows.  A changed scale must therefore never meet that state: forward and
    sample_begin refuse until prepare has run again, a change inside a trajectory is refused - and after the new prepare, on the
    same workspace with the steps captured before, the results are those of a handle that never knew another scale."""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import solver_time_grid
    m = _plan(ref_model, "handle")
    h, L = m.handle(), hip.lib()
    inp = _gap(tiny_inputs(B=1))
    from visualcloze_amd.model import MaskLayout
    N, T = inp["x"].shape[1], inp["txt"].shape[1]
    lay = MaskLayout(inp["txt_mask"], inp["img_mask"], 1, T, N)
    sl = slice(0, 1)
    bf = lambda a: a.to(DEV, torch.bfloat16).contiguous()  # noqa: E731
    txt, y, g = bf(lay.txt_rows(inp["txt"], sl)), bf(inp["y"]), inp["guidance"].to(DEV)
    ii, ti = lay.img_rows(inp["img_ids"], sl), lay.txt_rows(inp["txt_ids"], sl)
    img = bf(lay.img_rows(torch.cat((inp["x"], inp["cond"]), -1), sl))
    x0, cond = bf(lay.img_rows(inp["x"], sl)), bf(lay.img_rows(inp["cond"], sl))
    tg = solver_time_grid(4, N, 0.0, 1, True, 1)
    st = m.engine().stream

    def prepare(hh, s):
        hh.prepare(txt, y, g, False, ii, ti, 3, lay.kv_len(sl), lay.kv_gap(sl), stream=s)

    def run(hh, s):
        out, x = torch.empty(1, N, 64, dtype=torch.bfloat16, device=DEV), x0.clone()
        hh.forward(img, torch.tensor([0.7]), False, out, stream=s)
        hh.sample_euler(x, cond, tg, True, s)
        return out, x

    try:
        with torch.cuda.stream(st):
            s = st.cuda_stream
            prepare(h, s)
            a1, x1 = run(h, s)                                                   # scale 1: has run, has captured its step
            h.set_lora_scale(1.0)                                                # unchanged: nothing is stale
            out = torch.empty_like(a1)
            h.forward(img, torch.tensor([0.7]), False, out, stream=s)
            h.set_lora_scale(0.5)
            assert L.vc_flux_forward(h.h, img.data_ptr(), (C.c_float * 1)(0.7), 0, out.data_ptr(), s) == -3 and b"vc_flux_prepare again" in L.vc_last_error()
            with pytest.raises(hip.VclozeHipError, match="lora scale changed"):
                h.sample_begin(x0.clone(), cond, tg, True, s)
            prepare(h, s)
            a2, x2 = run(h, s)
            h.sample_begin(x0.clone(), cond, tg, True, s)
            assert L.vc_flux_set_lora_scale(h.h, 0.25) == -3 and b"scale" in L.vc_last_error()      # inside a trajectory
            h.sample_steps(3, s)
            x3 = torch.empty_like(x0)
            h.sample_end(x3, s)
        torch.cuda.synchronize()
        assert torch.equal(out, a1) and torch.equal(x3, x2) and not torch.equal(a1, a2) and not torch.equal(x1, x2)
        fresh = _model(scale=0.5)
        fh = fresh.handle()
        with torch.cuda.stream(st):
            prepare(fh, st.cuda_stream)
            b2, y2 = run(fh, st.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(a2, b2) and torch.equal(x2, y2)
    finally:
        h.set_lora_scale(1.0)


# ------------------------------------------------------------------------------------------ 6. what the twin cannot do
def _same_plans(m, row_counts):
    """every Linear of the un-merged plan (base, lora_A, lora_B), asked of the host-only launch planner at each pair of row counts:
    the same tile, the same main loop, no cut along M or K"""
    from tests.helpers import gemm_plan_answer
    from visualcloze_amd import hip
    L = hip.lib()

    def plan(M, N, K, epi):
        a = hip.GemmArgs()
        a.nprob, a.epi = 1, epi
        p = a.p[0]
        p.A = p.W = p.C = p.res = p.gate = 0x1000
        p.lda, p.ldw, p.ldc, p.ldres = K, K, N, N
        p.M, p.N, p.K, p.rows_per_batch = M, N, K, M
        ans = gemm_plan_answer(L, a, m.engine().tile_cfg)
        return ans[:5] + ans[6:]

    shapes = set()
    for r in m.engine().W.ref.values():
        shapes.add((tuple(r.w.shape), hip.EPI_BIAS))
        if r.A is not None:
            shapes.add((tuple(r.A.shape), hip.EPI_BIAS))
            shapes.add((tuple(r.B.shape), hip.EPI_GATE_RES))
    return all(plan(a, N, K, epi) == plan(b, N, K, epi) for (N, K), epi in shapes for a, b in row_counts)


def _unmerged_linear_budget(x, W, b, A, Bm, bB, s):
    """(ref64, budget) of out = bf16(y + bf16(bf16(h B^T + b_B) * s)), y = bf16(x W^T + b), h = bf16(x A^T), element by element:
    y and h carry the budget of a VC_EPI_BIAS GEMM (tests/budget.py gemm_case); the third GEMM is its VC_EPI_GATE_RES case with
    gate = s and residual y, whose inputs' own budgets - y's with gain 1, h's through |B| |s| - join its f32 terms."""
    from tests import budget as Bu
    y64, my, fy = Bu.gemm_case(x, W, b, 0)
    by = Bu.budget(y64, 1, my, fy)
    h64, mh, fh = Bu.gemm_case(x, A, None, 0)
    bh = Bu.budget(h64, 1, mh, fh)
    gate = torch.full((W.shape[0],), float(s), dtype=torch.float64)
    ref, mags, f32 = Bu.gemm_case(h64, Bm, bB, 2, res=y64, gate=gate)
    extra = by + abs(float(s)) * (bh @ Bm.to(torch.float64).abs().t())
    return ref, Bu.budget(ref, 3, mags, f32 + extra)


def test_batch_against_per_sample(ref_model):
    """B = 2 with unequal kv_len, un-merged, through the handle.  Where the tile plan of a GEMM differs with M, a batch and its
    samples run alone differ in the order of f32 sums.  Held element by element to the fp64 budget of tests/budget.py where one
    exists: the residual streams after img_in / txt_in (taps), each an un-merged Linear of the inputs alone - the batch's rows and
    each sample's own.  Behind them differences would travel through every block, where no per-element fp64 budget is defined
    (tests/budget.py budgets single kernels).  The bound there is derived for THIS geometry instead: the launch planner gives every
    Linear of the plan the same tile, main loop and no cut at the batch's row counts and at one sample's (`_same_plans`, asked of
    the planner here), the attention variant chosen by size is the same for B = 1 and B = 2, and every kernel of the plan computes
    a row from that row's operands alone (a GEMM tile sums over K in one order whatever else the tile holds; attention works per
    sample, head and query block; the norms and passes per row; gates and modulation rows are indexed per sample).  So nothing
    may depend on the batch: every tap and the output of each sample in the batch equal its own run BIT FOR BIT - which a wrong
    per-sample gate row, modulation row, kv_len or row offset does not survive."""
    from tests.procedural import tiny_inputs
    m = _plan(ref_model, "handle")
    assert m.max_batch() >= 2
    inp = tiny_inputs(B=2, seed=7)
    inp["img_mask"][1, -12:] = 0
    t = torch.tensor([0.9, 0.25])
    both = _taps(m, inp, t)
    one = lambda b: {k: (v[b:b + 1].clone() if torch.is_tensor(v) else v) for k, v in inp.items()}  # noqa: E731
    singles = [_taps(m, one(b), t[b:b + 1]) for b in range(2)]
    R = m.engine().W.ref
    f64 = lambda a: None if a is None else a.detach().cpu().to(torch.float64)  # noqa: E731
    for name, key, src in (("img_in", "img_in", torch.cat((inp["x"], inp["cond"]), -1)), ("txt_in", "txt_in", inp["txt"])):
        r = R[key]
        for b in range(2):
            x = src[b].to(torch.bfloat16).to(torch.float64)
            ref, bud = _unmerged_linear_budget(x, f64(r.w), f64(r.b), f64(r.A), f64(r.B), f64(r.bB), 1.0)
            for what, got in (("batch", both[name][b]), ("alone", singles[b][name][0])):
                ratio = ((got.cpu().to(torch.float64) - ref).abs() / bud).max().item()
                print(f"\n[{name} sample {b} {what}] worst |err| / budget = {ratio:.3f}")
                assert ratio <= 1.0, (name, b, what, ratio)
    from visualcloze_amd import hip
    N, T = inp["x"].shape[1], inp["txt"].shape[1]
    assert _same_plans(m, [(N, 2 * N), (T, 2 * T), (T + N, 2 * (T + N)), (1, 2)])
    n_cu, H = m.engine().n_cu, m.params.num_heads
    assert m.engine().attn_variant is None and hip.attention_variant_by_size(1, T + N, H, n_cu) == hip.attention_variant_by_size(2, T + N, H, n_cu)
    for b in range(2):
        assert torch.isfinite(both["out"][b].float()).all()
        for name in both:
            got, want = both[name][b], singles[b][name][0]
            assert torch.equal(got, want), f"{name} sample {b}: {(got != want).float().mean().item():.4f} of the elements differ, rel-L2 {rel_l2(got, want):.3e}"
    assert not torch.equal(both["out"][0], both["out"][1]) and not torch.equal(both["double.0.img"][0], both["double.0.img"][1])


def test_euler_trajectory_equals_the_twins_bitwise(ref_model):
    from tests.procedural import tiny_inputs
    m = ref_model
    inp = _gap(tiny_inputs(B=1))
    x = inp["x"].to(DEV, torch.bfloat16)
    fn = _fn("euler", 4)                                                          # 3 steps
    a = fn(x, _plan(m, "handle").forward, _kw(inp))
    b = fn(x, _plan(m, "python").forward, _kw(inp))
    torch.cuda.synchronize()
    assert a.shape == (4, 1) + tuple(x.shape[1:]) and torch.isfinite(a.float()).all()
    for i in range(4):
        assert torch.equal(a[i], b[i]), f"state {i}: rel-L2 {rel_l2(a[i], b[i]):.3e}"
    assert not torch.equal(a[0], a[-1])


def test_unmerged_euler_step_keeps_its_captured_nodes(ref_model, merged_model):
    """The captured Euler step in lora_mode 1 at B 2, T 16, N 24 (depth 2 + 2): 121 nodes in ONE graph, against 39 of the merged plan -
    the count recorded on the engine while it was one file, before resolve() / lora_of / mods (flux_weights.hip) and lora_linear /
    gemm() (flux_engine.hip) were put into separate units.  Every Linear with a pair is three GEMMs and, where its epilogue is not a plain
    bias, a pass behind them: a change of this number is a change of the captured graph."""
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=2)
    x = inp["x"].to(DEV, torch.bfloat16)
    assert (x.shape[0], inp["txt"].shape[1], x.shape[1]) == (2, 16, 24)
    nodes = {}
    for name, m in (("unmerged", _plan(ref_model, "handle")), ("merged", merged_model)):
        _fn("euler", 5, return_trajectory=False)(x, m.forward, _kw(inp))
        torch.cuda.synchronize()
        h = m.handle()
        assert h is not None and h.lora_mode == (name == "unmerged")
        nodes[name] = h.step_nodes()
    assert nodes == {"unmerged": (121, 0, 0), "merged": (39, 0, 0)}


def test_f32_state_rk4_and_true_cfg(ref_model):
    """a 2-step rk4 trajectory on an f32 state, and a true-CFG pair (B = 2, another text-mask length per half): fused through the
    handle against `_sample_foreign` over the same handle's forward - bit for bit, the bound tests/test_solvers_gpu.py and
    tests/test_cfg_gpu.py hold the merged mode to (test_fused_equals_eager_bitwise*)."""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import transport
    m = _plan(ref_model, "handle")
    inp = tiny_inputs(B=1)
    x = inp["x"].to(DEV, torch.float32)
    assert transport._fusable(m, x, "rk4")
    fn = _fn("rk4", 3)
    fused = fn(x, m.forward, _kw(inp))
    eager = fn(x, lambda xin, **k: m.forward(xin, **k).to(torch.bfloat16), _kw(inp))
    torch.cuda.synchronize()
    assert fused.dtype == torch.float32 and fused.shape == (3, 1) + tuple(x.shape[1:])
    for i in range(3):
        assert torch.equal(fused[i], eager[i]), f"rk4 state {i}: rel-L2 {rel_l2(fused[i], eager[i]):.3e}"
    assert not torch.equal(fused[-1].to(torch.bfloat16).float(), fused[-1])      # stepped IN f32
    inp2 = tiny_inputs(B=2, seed=7)
    inp2["txt_mask"][1, -5:] = 0                                                 # the negative prompt is shorter: unequal kv_gap
    x2 = inp2["x"].to(DEV, torch.bfloat16)
    kw = _kw(inp2, cfg_scale=3.5)
    assert transport._cfg_fusable(m, x2, "euler", {k: v for k, v in kw.items() if k != "cfg_scale"})
    fn = _fn("euler", 3)
    fused = fn(x2, m.forward_with_cfg, kw)
    eager = fn(x2, lambda xin, **k: m.forward_with_cfg(xin, **k).to(torch.bfloat16), kw)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(fused[i], eager[i]), f"cfg state {i}: rel-L2 {rel_l2(fused[i], eager[i]):.3e}"
    assert not torch.equal(fused[-1][:1], fused[-1][1:])


# ------------------------------------------------------------------------------------------ 7. full width, the reference itself
def test_full_width_unmerged_taps_vs_the_reference_bf16_run():
    """1 + 1 blocks at hidden 3072 / 24 heads / LoRA r256 / L = 3968: block_taps through the handle in un-merged mode against the
    reference's OWN bf16 autocast run (tests/golden/fullwidth_reference.npz, the *_bf16 arrays; bf16 guidance), at the bound
    tests/test_fullsize_gpu.py::test_full_width_blocks_vs_the_reference_itself holds the twin to: rel-L2 < 3e-2 for Flux.forward
    and every sampled block output."""
    from tests.procedural import procedural_param
    from visualcloze_amd.model import FLUX_DEV_FILL, FluxLoraWrapper, FluxParams
    gold = os.path.join(REPO, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_fullwidth_traj", os.path.join(gold, "make_fullwidth_traj.py"))
    FT = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FT)
    fx = np.load(os.path.join(gold, "fullwidth_reference.npz"))
    inp = FT.inputs("cfg2")
    assert float(fx["x_sum"]) == inp["x"].double().sum().item()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(DEV):
            m = FluxLoraWrapper(lora_rank=256, lora_scale=1.0, params=FluxParams(**{**FLUX_DEV_FILL, "depth": 1, "depth_single_blocks": 1}))
    finally:
        torch.set_default_dtype(old)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(procedural_param(k, v.shape, device=DEV, dtype=torch.float32))
    m = m.eval()
    m.lora_mode, m.ref_plan = "ref", "handle"
    got = _taps(m, inp, torch.tensor(fx["t"]), torch.bfloat16)
    assert m.handle() is not None and m.handle().lora_mode == 1
    rs, cs = int(fx["row_stride"]), int(fx["col_stride"])
    bf = lambda k: torch.tensor(fx[k].view(np.int16)).view(torch.bfloat16).float()  # noqa: E731
    errs = {"flux": rel_l2(got["out"], bf("flux_bf16").reshape(got["out"].shape)),
            "double_img": rel_l2(got["double.0.img"][0, ::rs, ::cs], bf("double_img_bf16")),
            "double_txt": rel_l2(got["double.0.txt"][0, ::rs, ::cs], bf("double_txt_bf16")),
            "single": rel_l2(got["single.0"][0, ::rs, ::cs], bf("single_bf16"))}
    print("\n[1+1 blocks at full width, cfg2, handle lora_mode 1] vs the REFERENCE's own bf16 run: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v < 3e-2 for v in errs.values()), errs


# ------------------------------------------------------------------------------------------ 8. errors
def test_errors_name_the_argument_and_launch_nothing(ref_model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import solver_time_grid
    m = _plan(ref_model, "handle")
    h = m.handle()
    L = hip.lib()
    p = m.params
    inp = tiny_inputs(B=1)
    kw = _kw(inp)
    st = m.engine().stream
    with torch.cuda.stream(st):
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 2, stream=st.cuda_stream)
    torch.cuda.synchronize()
    dst = torch.full((inp["x"].shape[1], p.hidden_size), 7.0, dtype=torch.bfloat16, device=DEV)

    def refused(rc, code, word):
        msg = L.vc_last_error()
        assert rc == code and msg and word in msg, (rc, msg)

    refused(L.vc_flux_set_tap(h.h, b"double.0.image", dst.data_ptr()), -1, b"name")
    refused(L.vc_flux_set_tap(h.h, b"nope", dst.data_ptr()), -1, b"name")
    refused(L.vc_flux_set_tap(h.h, f"double.{p.depth}.img".encode(), dst.data_ptr()), -1, b"double blocks")
    refused(L.vc_flux_set_tap(h.h, f"single.{p.depth_single_blocks}".encode(), dst.data_ptr()), -1, b"single blocks")
    rows, cols = C.c_int64(0), C.c_int32(0)
    refused(L.vc_flux_tap_shape(h.h, b"double.9.txt", C.byref(rows), C.byref(cols)), -1, b"name")
    R = m.engine().W.ref["img_in"]
    D, K = R.w.shape
    a48 = torch.zeros(48, K, dtype=torch.bfloat16, device=DEV)
    b48 = torch.zeros(D, 48, dtype=torch.bfloat16, device=DEV)
    refused(L.vc_flux_bind_lora(h.h, b"img_in", a48.data_ptr(), K, b48.data_ptr(), 48, None, D, K, 48), -1, b"rank")
    refused(L.vc_flux_bind_lora(h.h, b"img_in", R.A.data_ptr(), K, R.B.data_ptr(), 64, None, D, K - 64, 64), -1, b"in_features")
    refused(L.vc_flux_bind_lora(h.h, b"img_in", R.A.data_ptr(), K, R.B.data_ptr(), 64, None, D + 8, K, 64), -1, b"out_features")
    refused(L.vc_flux_bind_lora(h.h, b"no_such.linear", R.A.data_ptr(), K, R.B.data_ptr(), 64, None, D, K, 64), -3, b"name")
    # a mode switch in the middle of a trajectory
    x = inp["x"].to(DEV, torch.bfloat16).clone()
    tg = solver_time_grid(3, x.shape[1], 0.0, 1, True, 1)
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.sample_begin(x, kw["cond"], tg, True, s)
        h.sample_steps(1, s)
        refused(L.vc_flux_set_option(h.h, b"lora_mode", 0), -3, b"lora_mode")
        h.sample_steps(1, s)
        out = torch.empty_like(x)
        h.sample_end(out, s)
    torch.cuda.synchronize()
    assert torch.equal(dst, torch.full_like(dst, 7.0)) and not h._taps           # nothing was bound, nothing written
    want = _fn("euler", 3, return_trajectory=False)(x, m.forward, kw)            # the refused calls left the handle as it was
    assert torch.equal(out, want[-1])
