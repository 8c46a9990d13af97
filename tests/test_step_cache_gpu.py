"""-m gpu: the opt-in first-block step cache of the fused Euler loop (vc_flux_set_step_cache).

The rule is restated HERE (`restate`), independently of csrc/flux_engine.hip: the literal torch expressions for r, P, R, the metric
and the decision, around `engine.FluxEngine`'s per-block methods (imported, never edited) on the tiny model of the solver tests.

  1. the three kernels against torch: r, sub, add bit for bit; the two sums against an fp64 sum;
  2. never reusing == the uncached handle trajectory, bit for bit;
  3. always reusing: the pattern "compute, k reuses, compute, ..." and the final latent against the restatement;
  4. data-dependent decisions equal the restatement's at EVERY step;
  5. determinism and state hygiene;  6. batch;  7. the Python surface.

Bound of test 3 (measured, not invented): dev0 = the deviation of the UNCACHED handle trajectory from the restatement with its cache
off, same inputs; the cached run is allowed 2 x dev0 (each reused step adds two bf16 roundings, R and h1 + R).  The restatement runs
the library's own kernels in the handle's launch order, so dev0 may well be 0 - the cached run must then be bit-equal too.  Both
figures are printed and go to the file VC_PARITY_LOG names (profiles/r10a_step_cache_parity.log).

The seed of test 4 was not checked against the CPU oracle beforehand; instead the test prints and asserts the margin its threshold
keeps from every metric of the restatement's thresholded run (see there)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 8                      # Euler steps of every trajectory here


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()[0]


def _cache(threshold, k=1):
    from visualcloze_amd.transport import StepCache
    return StepCache(threshold, k)


def _inputs(B=1, seed=1, copies=0):
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=1 if copies else B, seed=seed)
    if copies:
        inp = {k: v.repeat(copies, *([1] * (v.dim() - 1))) for k, v in inp.items()}
    return {k: (v.to(DEV, torch.bfloat16) if k in ("x", "cond", "txt", "y") else v.to(DEV)) for k, v in inp.items()}


def _grid(inp):
    from visualcloze_amd.transport import solver_time_grid
    return solver_time_grid(S + 1, inp["x"].shape[1], 0.0, 1, True, 1)


def run_handle(m, inp, cache):
    """one trajectory through vc_flux_sample_ode -> (trajectory [S, B, N, C], stats, workspace bytes)"""
    from visualcloze_amd import hip
    h = m.handle()
    h.set_step_cache(cache)
    B, T, N = inp["x"].shape[0], inp["txt"].shape[1], inp["x"].shape[1]
    st = m.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(inp["txt"], inp["y"], inp["guidance"], False, inp["img_ids"], inp["txt_ids"], S, stream=s)
        x = inp["x"].clone()
        traj = torch.empty((S,) + tuple(x.shape), dtype=torch.bfloat16, device=DEV)
        h.sample_ode("euler", x, inp["cond"], _grid(inp), True, s, trajectory=traj)
    torch.cuda.synchronize()
    assert torch.equal(traj[-1], x)
    return traj, h.step_cache_stats(S), hip.lib().vc_flux_workspace_bytes(h.h, B, T, N, S)


def restate(m, inp, threshold=0.0, k=0):
    """THE RULE, restated.  threshold <= 0 or k == 0: off.  Returns (trajectory, decisions, metrics, per-sample metrics)."""
    from visualcloze_amd import hip
    from visualcloze_amd.transport import model_times
    eng = m.engine()
    x = inp["x"]
    B, N, C = x.shape
    T = inp["txt"].shape[1]
    t32 = _grid(inp).to(torch.float32)
    ws = eng.workspace(T, N, S, B)
    eng.prepare_sample(ws, inp["txt"], inp["y"], inp["guidance"], False, inp["img_ids"], inp["txt_ids"], model_times(t32, x),
                       [T + N] * B)
    ws.DTS.copy_((t32[1:] - t32[:-1]).contiguous())
    ws.STEP.zero_()
    ws.XS.copy_(x.reshape(B * N, C))
    ws.COND.copy_(inp["cond"].reshape(B * N, -1))
    c = eng._ctx(ws, ws.STEP, None)
    L, D = T + N, ws.XI.shape[-1]
    on = threshold > 0 and k != 0
    P = R = None
    run = 0
    traj, decisions, metrics, per_sample = [], [], [], []
    for _ in range(S):
        hip.concat_cols(ws.XS, ws.COND, ws.XIN)
        hip.copy(ws.XT, ws.TXT0)
        eng._lin("img_in", ws.XIN, ws.XI)
        h0 = ws.XI.clone()
        eng.double_block(c, 0)
        h1 = ws.XI.clone()
        r = (h1.float() - h0.float()).to(torch.bfloat16)
        mb = None
        if P is not None:
            num = (r.double() - P.double()).abs().reshape(B, -1).sum(1)
            mb = (num / P.double().abs().reshape(B, -1).sum(1)).tolist()
        mm = math.nan if mb is None else max(mb)
        reuse = on and P is not None and mm < threshold and (k < 0 or run < k)
        if reuse:
            xi = (h1.float() + R.float()).to(torch.bfloat16).reshape(B, N, D)
            ws.X.reshape(B, L, D)[:, T:].copy_(xi)
            run += 1
        else:
            for i in range(1, eng.g.depth):
                eng.double_block(c, i)
            eng.join_streams(c)
            for i in range(eng.g.depth_single_blocks):
                eng.single_block(c, i)
            hE = ws.X.reshape(B, L, D)[:, T:].reshape(B * N, D)
            P, R, run = r, (hE.float() - h1.float()).to(torch.bfloat16), 0
        eng.last_layer(c)
        hip.euler_step(ws.XS, ws.V, ws.DTS, ws.STEP)
        hip.step_advance(ws.STEP)
        torch.cuda.synchronize()
        traj.append(ws.XS.reshape(B, N, C).clone())
        decisions.append("reuse" if reuse else "compute")
        metrics.append(mm)
        per_sample.append(mb)
    return torch.stack(traj), decisions, metrics, per_sample


def sum_tol(inp, m):
    """relative tolerance of the handle's f32 metric against an fp64 one: two sums of n = N * D terms (test 1)"""
    n = inp["x"].shape[1] * m.engine().D
    return 2 * 1.01 * n * 2.0 ** -24


def handle_decisions(stats, threshold, k):
    """the handle reports its metrics and counts, not its decisions one by one: they follow from the rule, given ITS metrics - and
    must reproduce its counts"""
    out, have, run = [], False, 0
    for mm in stats["metrics"]:
        reuse = have and mm < threshold and (k < 0 or run < k)
        out.append("reuse" if reuse else "compute")
        run = run + 1 if reuse else 0
        have = True
    assert (out.count("compute"), out.count("reuse")) == (stats["computed"], stats["reused"])
    return out


# ---------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("B,n", [(1, 24 * 256), (2, 96 * 256), (3, 8), (4, 200 * 1024 + 8)])
def test_kernels_against_torch(B, n):
    """r, sub, add: bit-exact against the literal expressions.  The sums against fp64: every term |f32(r) - f32(P)| carries one f32
    rounding (relative 2^-24) and a sum of n non-negative terms in f32 - in ANY order - carries at most (n - 1) 2^-24 relative error
    to first order (each term passes through at most n - 1 additions, each of relative error 2^-24, and nothing cancels), so
    |got - fp64| <= n 2^-24 fp64; 1.01 x for the second-order terms.  The ratio of two such sums: twice that."""
    from visualcloze_amd import hip
    g = torch.Generator().manual_seed(B * 1000 + n % 997)
    h0, h1, p = [(torch.randn(B, n, generator=g) * 3).to(DEV, torch.bfloat16) for _ in range(3)]
    if B == 2:
        p[1] *= 0.01                                                    # the second sample has the larger ratio by far
    r, sums, metric = hip.residual_change(h0, h1, p)
    torch.cuda.synchronize()
    want_r = (h1.float() - h0.float()).to(torch.bfloat16)
    assert torch.equal(r, want_r)
    s0 = (want_r.double() - p.double()).abs().sum(1)
    s1 = p.double().abs().sum(1)
    tol = 1.01 * n * 2.0 ** -24
    got = sums.double()
    print(f"\nresidual_change B={B} n={n}: rel err of the sums {((got[:, 0] - s0).abs() / s0).max().item():.2e} / "
          f"{((got[:, 1] - s1).abs() / s1).max().item():.2e} (tolerance {tol:.2e})")
    assert ((got[:, 0] - s0).abs() <= tol * s0).all() and ((got[:, 1] - s1).abs() <= tol * s1).all()
    want_m = (s0 / s1).max().item()
    assert abs(metric.item() - want_m) <= 2 * tol * want_m + 2.0 ** -24 * want_m
    assert metric.item() == (sums[:, 0] / sums[:, 1]).max().item()          # the max of the f32 ratios, exactly
    r2, sums2, metric2 = hip.residual_change(h0, h1, p)                      # fixed reduction order: the same bits again
    assert torch.equal(sums, sums2) and torch.equal(metric, metric2)
    # sub / add on contiguous samples and on strided ones (the image rows of a joint stream: rows T.. of every sample)
    a, b = h0, h1
    assert torch.equal(hip.residual_sub(a, b), (a.float() - b.float()).to(torch.bfloat16))
    assert torch.equal(hip.residual_add(a, b), (a.float() + b.float()).to(torch.bfloat16))
    joint = (torch.randn(B, n + 64, generator=g) * 3).to(DEV, torch.bfloat16)
    before = joint.clone()
    view = joint[:, 64:]
    assert torch.equal(hip.residual_sub(view, b), (view.float() - b.float()).to(torch.bfloat16))
    hip.residual_add(a, b, out=view)
    torch.cuda.synchronize()
    assert torch.equal(joint[:, 64:], (a.float() + b.float()).to(torch.bfloat16)) and torch.equal(joint[:, :64], before[:, :64])


@pytest.mark.parametrize("n", [8, 257 * 8, (256 * 256 + 3) * 8], ids=["1 chunk", "257 chunks", "256 * 256 + 3 chunks"])
def test_sums_have_the_bits_of_the_stated_order(n):
    """Both sums of vc_residual_change against reduction.ordered_sum, f32 bit for bit: one chunk, a second block that is nearly
    empty, a second round of the capped grid.  B = 3: pass 2 runs its tree three times over the same LDS.  The addends of a 16-byte
    chunk, in order: |f32(r) - f32(P)| (and |f32(P)|) of its eight elements, r = bf16(h1 - h0).  The fp64 budget of
    test_kernels_against_torch stands beside the bit comparison."""
    from visualcloze_amd import hip
    from visualcloze_amd.reduction import ordered_sum
    B = 3
    g = torch.Generator().manual_seed(77 + n % 997)
    h0, h1, p = [(torch.randn(B, n, generator=g) * 3).to(DEV, torch.bfloat16) for _ in range(3)]
    p[2] *= 0.01
    r, sums, metric = hip.residual_change(h0, h1, p)
    torch.cuda.synchronize()
    want_r = (h1.float() - h0.float()).to(torch.bfloat16)
    assert torch.equal(r, want_r)
    rf, pf = want_r.float().cpu(), p.float().cpu()
    t0, t1 = (rf - pf).abs().reshape(B, n // 8, 8), pf.abs().reshape(B, n // 8, 8)
    want = torch.stack([torch.stack([ordered_sum(t[b], max_blocks=hip.RESIDUAL_CHANGE_MAX_BLOCKS) for t in (t0, t1)]) for b in range(B)])
    s64 = torch.stack([t0.double().sum((1, 2)), t1.double().sum((1, 2))], 1)
    tol = 1.01 * n * 2.0 ** -24
    rel = ((sums.double().cpu() - s64).abs() / s64).max().item()
    print(f"\nresidual_change B={B} n={n}: sums {sums.tolist()} mirror {want.tolist()}, rel err against fp64 {rel:.2e} (tolerance {tol:.2e})")
    assert rel <= tol
    assert torch.equal(sums.cpu(), want)
    assert metric.item() == (sums[:, 0] / sums[:, 1]).max().item()          # the max of the f32 ratios, exactly


def test_kernel_argument_errors():
    from visualcloze_amd import hip
    a = torch.zeros(2, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(hip.VclozeHipError, match="multiple"):
        hip.residual_add(a, a.clone())
    with pytest.raises(hip.VclozeHipError, match="multiple of 8"):
        hip.residual_change(a, a.clone(), a.clone())
    with pytest.raises(hip.VclozeHipError):
        hip.residual_sub(a.float(), a)


# ---------------------------------------------------------------------------------------------- 2. never reusing
def test_never_reusing_is_the_uncached_trajectory_bitwise(model):
    inp = _inputs()
    base, st0, _ = run_handle(model, inp, None)
    assert (st0["computed"], st0["reused"]) == (S, 0) and all(math.isnan(v) for v in st0["metrics"])
    probe, st, _ = run_handle(model, inp, _cache(1e-30))
    finite = st["metrics"][1:]
    assert all(math.isfinite(v) and v > 0 for v in finite) and math.isnan(st["metrics"][0])
    tiny = min(finite) * 0.5                                           # below every recorded metric
    got, st, _ = run_handle(model, inp, _cache(tiny, 3))
    assert torch.equal(got, base)
    assert (st["computed"], st["reused"]) == (S, 0) and len(st["metrics"]) == S
    assert math.isnan(st["metrics"][0]) and all(math.isfinite(v) for v in st["metrics"][1:])
    run_handle(model, inp, None)


# ---------------------------------------------------------------------------------------------- 3. always reusing
@pytest.mark.parametrize("k", [1, 2, 3])
def test_always_reusing_pattern_and_latent(model, k):
    from tests.helpers import parity_log
    inp = _inputs()
    want_off, _, _, _ = restate(model, inp)
    base, _, _ = run_handle(model, inp, None)
    dev0 = rel_l2(base[-1], want_off[-1])
    want, dec, _, _ = restate(model, inp, math.inf, k)
    got, st, _ = run_handle(model, inp, _cache(math.inf, k))
    pattern = [("compute" if i % (k + 1) == 0 else "reuse") for i in range(S)]
    assert dec == pattern and handle_decisions(st, math.inf, k) == pattern
    assert (st["computed"], st["reused"]) == (pattern.count("compute"), pattern.count("reuse"))
    dev = rel_l2(got[-1], want[-1])
    parity_log(f"[tiny, step cache, threshold inf, max_consecutive {k}] final latent vs the restatement: {dev:.3e}; the uncached "
               f"handle vs the restatement with the cache off: {dev0:.3e} (bound 2 x that = {2 * dev0:.3e}); cached vs uncached "
               f"latent: {rel_l2(got[-1], base[-1]):.3e}")
    assert not torch.equal(got[-1], base[-1])                           # the cache does change the result
    assert dev <= 2 * dev0
    run_handle(model, inp, None)


# ---------------------------------------------------------------------------------------------- 4. data-dependent decisions
def _gap_threshold(metrics):
    v = sorted(x for x in metrics if math.isfinite(x))
    gaps = [(v[i + 1] - v[i], i) for i in range(len(v) - 1)]
    g, i = max(gaps)
    return 0.5 * (v[i] + v[i + 1]), g


def test_data_dependent_decisions_equal_the_restatement(model):
    from tests.helpers import parity_log
    inp = _inputs()
    _, _, never, _ = restate(model, inp)                                # the restatement's own metrics, nothing reused
    thr, gap = _gap_threshold(never)
    want_off = restate(model, inp)[0]
    dev0 = rel_l2(run_handle(model, inp, None)[0][-1], want_off[-1])
    want, dec, ms, _ = restate(model, inp, thr, 2)
    got, st, _ = run_handle(model, inp, _cache(thr, 2))
    margin = min(abs(v - thr) / thr for v in ms if math.isfinite(v))
    parity_log(f"[tiny, step cache, decisions] threshold {thr:.4e} (largest gap {gap:.3e} of {['%.4e' % v for v in never[1:]]}); "
               f"restated run: {dec}, metrics {['%.4e' % v for v in ms[1:]]}, smallest relative margin to the threshold {margin:.2e}")
    # the handle's f32 metric is within 2 x 1.01 n 2^-24 of this fp64 one (test 1; n = N * D): a margin ten times that makes the
    # comparison meaningful for every step
    tol = sum_tol(inp, model)
    assert margin > 10 * tol
    assert "reuse" in dec and dec.count("compute") > 1
    assert handle_decisions(st, thr, 2) == dec                          # every step
    dev = rel_l2(got[-1], want[-1])
    parity_log(f"[tiny, step cache, decisions] final latent vs the restatement: {dev:.3e} (bound 2 x {dev0:.3e}, as in test 3)")
    assert dev <= 2 * dev0
    run_handle(model, inp, None)


# ---------------------------------------------------------------------------------------------- 5. determinism, hygiene
def test_determinism_and_state_hygiene(model):
    from tests.helpers import tiny_model
    inp, other = _inputs(), _inputs(seed=5)
    c = _cache(math.inf, 2)
    a, sa, bytes_on = run_handle(model, inp, c)
    b, sb, _ = run_handle(model, inp, c)
    assert torch.equal(a, b)
    assert sa["metrics"][1:] == sb["metrics"][1:] and (sa["computed"], sa["reused"]) == (sb["computed"], sb["reused"])
    # a second trajectory does not see the first one's P / R: after another sample ran, the same bits again
    run_handle(model, other, c)
    b2, sb2, _ = run_handle(model, inp, c)
    assert torch.equal(a, b2) and math.isnan(sb2["metrics"][0]) and sb2["metrics"][1:] == sa["metrics"][1:]
    # cache off again == a handle that never had it on, workspace size included
    off, st_off, bytes_off = run_handle(model, inp, None)
    fresh = tiny_model()[0]
    want, _, bytes_fresh = run_handle(fresh, inp, None)
    assert torch.equal(off, want) and bytes_off == bytes_fresh and (st_off["computed"], st_off["reused"]) == (S, 0)
    N, D = inp["x"].shape[1], model.engine().D
    assert bytes_on - bytes_off >= 3 * N * D * 2 and bytes_on - bytes_off < 3 * N * D * 2 + 16384
    # through the sampler: the cached graphs and the plain one live side by side on the handle
    assert torch.equal(run_handle(model, inp, c)[0], a) and torch.equal(run_handle(model, inp, None)[0], off)


def test_refusals_on_the_handle(model):
    from visualcloze_amd import hip
    inp = _inputs()
    h = model.handle()
    st = model.engine().stream
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.set_step_cache(_cache(0.1))
        h.prepare(inp["txt"], inp["y"], inp["guidance"], False, inp["img_ids"], inp["txt_ids"], 2 * S, stream=s)
        with pytest.raises(hip.VclozeHipError, match="VC_SOLVER_EULER only"):
            h.sample_ode("midpoint", inp["x"].clone(), inp["cond"], _grid(inp), True, s)
        h.set_step_cache(None)
        h.prepare(inp["txt"], inp["y"], inp["guidance"], False, inp["img_ids"], inp["txt_ids"], S, stream=s)
        hip._check(hip.lib().vc_flux_set_step_cache(h.h, 0.1, 1), "set")       # on AFTER prepare: the workspace lacks P / R
        with pytest.raises(hip.VclozeHipError, match="prepare again"):
            h.sample_ode("euler", inp["x"].clone(), inp["cond"], _grid(inp), True, s)
        hip._check(hip.lib().vc_flux_set_step_cache(h.h, 0.0, 0), "set")
        h.sample_ode("euler", inp["x"].clone(), inp["cond"], _grid(inp), True, s)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. batch
def test_batch_metric_is_the_larger_and_copies_decide_as_one(model):
    inp2 = _inputs(B=2, seed=7)
    _, _, ms, per = restate(model, inp2)
    _, st, _ = run_handle(model, inp2, _cache(1e-30))
    tol = sum_tol(inp2, model)
    told_apart = 0
    for i in range(1, S):
        assert abs(st["metrics"][i] - max(per[i])) <= tol * max(per[i]), (i, st["metrics"][i], per[i])
        told_apart += abs(st["metrics"][i] - min(per[i])) > 4 * tol * max(per[i])      # ... and it is NOT the smaller one
    assert told_apart >= 1, per          # two different samples: in some step their values are far enough apart to tell
    # two copies of one sample decide as the sample alone does
    one, two = _inputs(), _inputs(copies=2)
    _, _, never, _ = restate(model, one)
    thr, _ = _gap_threshold(never)
    t1, s1, _ = run_handle(model, one, _cache(thr, 2))
    t2, s2, _ = run_handle(model, two, _cache(thr, 2))
    assert handle_decisions(s1, thr, 2) == handle_decisions(s2, thr, 2) and s1["reused"] > 0
    assert torch.isfinite(t1.float()).all() and torch.isfinite(t2.float()).all()
    run_handle(model, one, None)


# ---------------------------------------------------------------------------------------------- 7. the Python surface
def test_python_surface(model):
    from tests.procedural import tiny_inputs
    from visualcloze_amd import pipeline
    from visualcloze_amd.transport import Sampler, StepCache, create_transport
    inp = tiny_inputs(B=1)
    txt, y = inp["txt"].to(DEV, torch.bfloat16), inp["y"].to(DEV, torch.bfloat16)
    noise = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16) for _ in range(2)]
    lat = [torch.randn(1, 16, 8, 24, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16) for _ in range(2)]
    masks = [torch.ones(1, 1, 64, 192, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    plain = pipeline.denoise_grid(model, noise, lat, masks, txt, y, cfg=30.0, steps=6)
    model.last_step_cache_stats = None
    rows = pipeline.denoise_grid(model, noise, lat, masks, txt, y, cfg=30.0, steps=6, step_cache=StepCache(math.inf, 1))
    st = model.last_step_cache_stats
    assert len(st) == 1 and (st[0]["computed"], st[0]["reused"]) == (3, 2) and len(st[0]["metrics"]) == 5
    assert all(torch.isfinite(r.float()).all() for r in rows) and any(not torch.equal(a, b) for a, b in zip(rows, plain))
    again = pipeline.denoise_grid(model, noise, lat, masks, txt, y, cfg=30.0, steps=6)      # the keyword's default is off
    assert all(torch.equal(a, b) for a, b in zip(again, plain))
    up = pipeline.sdedit_upsample(model, noise[0], lat[0], lat[1], txt, y, cfg=30.0, steps=5, strength=0.4,
                                  step_cache=StepCache(math.inf, 2))
    st = model.last_step_cache_stats
    assert torch.isfinite(up.float()).all() and (st[0]["computed"], st[0]["reused"]) == (2, 2)
    # the sampler keeps the stats too; refusals on the Flux path are ValueErrors, never a silent full evaluation
    s = Sampler(create_transport())
    kw = {k: v for k, v in _inputs().items() if k != "x"}
    x = _inputs()["x"]
    s.sample_ode(sampling_method="euler", num_steps=4, do_shift=True, time_shifting_factor=1, step_cache=StepCache(math.inf))(
        x, model.forward, kw)
    assert (s.last_step_cache_stats[0]["computed"], s.last_step_cache_stats[0]["reused"]) == (2, 1)
    model.use_handle = False
    try:
        with pytest.raises(ValueError, match="C handle"):
            s.sample_ode(sampling_method="euler", num_steps=4, step_cache=StepCache(0.1))(x, model.forward, kw)
    finally:
        model.use_handle = True
    with pytest.raises(ValueError, match="stepped eagerly"):
        s.sample_ode(sampling_method="euler", num_steps=4, step_cache=StepCache(0.1))(x.to(torch.float16), model.forward, kw)
