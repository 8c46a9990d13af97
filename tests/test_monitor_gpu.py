"""The numerics monitor on the GPU (include/vcloze_hip.h: vc_tensor_stats, vc_flux_set_monitor, vc_flux_monitor_report).

Op level: vc_tensor_stats against an fp64 restatement in numpy - the two counts and max |x| bit for bit, sum x^2 inside a budget
that follows from the number of f32 additions of the order the header states (`_adds`), never from what the kernel returned.
Handle level (tiny procedural model: hidden 256, 2 heads, 2 + 2 blocks, T = 64, N = 96, B = 2): the monitor changes no bit of a
trajectory, its log agrees with statistics taken in torch from taps, the model's output and the trajectory, and the report names the
site where a NaN / inf first appeared.  No kernel is made to fault: the non-finite values flow through ordinary arithmetic."""
import math

import numpy as np
import pytest
import torch

from tests.budget import EPS24, assert_within_budget

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("max_abs", "sum_sq", "nonfinite", "count")


# ------------------------------------------------------------------------------------------ references
def _adds(rows: int, cols: int, f32: bool) -> int:
    """f32 roundings on the way to sum_sq in the order of the header: a thread's chain - ceil(units / (nblk * 256)) units of E
    elements, one addition each (and, for f32 data, one rounding of each product: bf16 squares are exact in f32) - then the 8 levels of
    the block's tree and the 8 levels of the tree over the block sums."""
    E = 4 if f32 else 8
    units = rows * ((cols + E - 1) // E)
    nblk = min((units + 255) // 256, 256)
    chain = -(-units // (nblk * 256)) * E
    return chain * (2 if f32 else 1) + 16


def _ref(x: torch.Tensor):
    """fp64 statistics per sample of a [B, rows, cols] tensor (any strides)"""
    a = x.detach().cpu().to(torch.float64).reshape(x.shape[0], -1).numpy()
    fin = np.isfinite(a)
    z = np.where(fin, a, 0.0)
    return dict(max_abs=np.abs(z).max(axis=1), sum_sq=(z * z).sum(axis=1), nonfinite=(~fin).sum(axis=1), count=np.full(a.shape[0], a.shape[1]))


def _check(rec, x, what, adds=None):
    """rec: structured records [B] of x's samples.  Counts and max_abs exact, sum_sq within adds * 2^-24 * sum x^2 of the fp64 sum."""
    want = _ref(x)
    B, R, Cc = x.shape
    assert np.array_equal(rec["nonfinite"], want["nonfinite"].astype(np.uint32)), (what, rec["nonfinite"], want["nonfinite"])
    assert np.array_equal(rec["count"], want["count"].astype(np.uint32)), (what, rec["count"])
    assert np.array_equal(rec["max_abs"].view(np.uint32), want["max_abs"].astype(np.float32).view(np.uint32)), (what, rec["max_abs"], want["max_abs"])
    adds = _adds(R, Cc, x.dtype == torch.float32) if adds is None else adds
    ref = torch.from_numpy(want["sum_sq"])
    return assert_within_budget(torch.from_numpy(rec["sum_sq"].astype(np.float64)), ref, roundings=0, f32_terms=adds * EPS24 * ref, what=what)


def _values(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 3.0).to(dtype)


def _stats(x, **kw):
    from visualcloze_amd import hip
    out = hip.tensor_stats(x, **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------ op level
def _cases():
    """(name, tensor on the device).  Sample roles: random values with NaN / +-inf at the first and last element and on both sides of
    the boundaries between threads, blocks and rounds of the grid, a finite value larger than everything else next to an inf; an
    all-non-finite sample; an all-zero sample."""
    inf, nan = float("inf"), float("nan")
    out = []

    def special(x, E):
        flat = x[0].reshape(-1)                      # a view where x[0] is contiguous; strided cases set by index below
        n = flat.numel()
        for i, v in ((0, nan), (n - 1, -inf), (256 * E - 1, inf), (256 * E, nan), (65536 * E - 1, -inf), (65536 * E, inf)):
            if 0 < i < n - 1 or i in (0, n - 1):
                flat[i] = v
        if n > 40:
            flat[20], flat[21] = inf, 3.0e4          # the largest finite value sits next to an inf

    x = _values((1, 1, 8), torch.bfloat16, 1)
    x[0, 0, 0], x[0, 0, 7], x[0, 0, 3] = nan, inf, -77.0
    out.append(("1x1x8", x.to(DEV)))
    for dt, name in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        x = _values((2, 3, 64), dt, 2)
        special(x, 8 if dt == torch.bfloat16 else 4)
        x[1] = 0.0                                   # an all-zero sample
        out.append((f"2x3x64 {name}", x.to(DEV)))
    x = _values((2, 3, 64), torch.bfloat16, 3)
    x[1, :, 0::3], x[1, :, 1::3], x[1, :, 2::3] = nan, inf, -inf      # an all-non-finite sample
    out.append(("2x3x64 all-nonfinite", x.to(DEV)))
    # the strided stream: 37 rows of 256 columns inside rows of 320, behind 5 leading rows of each sample's 48
    buf = _values((2, 48, 320), torch.bfloat16, 4)
    buf[:, :5], buf[:, 42:], buf[:, :, 256:] = nan, nan, inf          # everything outside the view is non-finite
    v = buf[:, 5:42, :256]
    v[0, 0, 0], v[0, 36, 255], v[1, 17, 100], v[1, 17, 101] = nan, -inf, inf, -2.5e4
    out.append(("strided 2x37x256 ld 320", buf.to(DEV)[:, 5:42, :256]))
    # the element-wise path: 13 columns from a base 2 bytes off
    flat = torch.zeros(1 + 2 * 5 * 13, dtype=torch.bfloat16)
    flat[0] = nan
    w = flat[1:].view(2, 5, 13)
    w.copy_(_values((2, 5, 13), torch.bfloat16, 5))
    w[0, 0, 0], w[0, 4, 12], w[1, 2, 12], w[1, 3, 0] = inf, nan, -inf, 9.0e3
    out.append(("2x5x13 misaligned", flat.to(DEV)[1:].view(2, 5, 13)))
    # more than one block, VC_MONITOR_MAX_BLOCKS partials and two rounds of the grid per thread
    x = _values((2, 4096, 256), torch.bfloat16, 6)
    special(x, 8)
    out.append(("2x4096x256", x.to(DEV)))
    x = _values((1, 700, 100), torch.float32, 7)                      # f32, several blocks, not a power of two
    special(x, 4)
    out.append(("1x700x100 f32", x.to(DEV)))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_tensor_stats_against_fp64(cases):
    from visualcloze_amd import hip
    for name, x in cases:
        rec = hip.stats_to_numpy(_stats(x))
        assert rec.shape == (x.shape[0],)
        worst = _check(rec, x, name)
        print(f"tensor_stats {name}: sum_sq at {worst:.3f} of its budget ({_adds(x.shape[1], x.shape[2], x.dtype == torch.float32)} roundings)")
    names = [n for n, _ in cases]
    assert any(int(_ref(x)["nonfinite"][1]) == x[1].numel() for n, x in cases if x.shape[0] > 1)        # the all-non-finite sample is there
    assert "2x4096x256" in names


def test_budget_rejects_a_sum_beyond_it(cases):
    """the mutant: a sum_sq moved by twice its budget does not pass the check that the kernel's passes"""
    from visualcloze_amd import hip
    name, x = cases[-2]
    rec = hip.stats_to_numpy(_stats(x)).copy()
    _check(rec, x, name)
    ref = _ref(x)["sum_sq"][0]
    rec["sum_sq"][0] = np.float32(ref * (1.0 + 2.0 * _adds(x.shape[1], x.shape[2], False) * EPS24))
    assert rec["sum_sq"][0] != np.float32(ref)
    with pytest.raises(AssertionError, match="over budget"):
        _check(rec, x, name)


def test_two_runs_and_both_load_paths_give_the_same_bits(cases):
    for name, x in cases:
        a, b = _stats(x), _stats(x)
        assert torch.equal(a, b), name
    # the same values through 16-byte loads and element by element (a base 2 bytes off)
    x = cases[-2][1][:, :64]
    flat = torch.zeros(1 + x.numel(), dtype=x.dtype, device=DEV)
    y = flat[1:].view(x.shape)
    y.copy_(x)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 2
    assert torch.equal(_stats(x.contiguous()), _stats(y))


def _ordered_sum_sq(x: torch.Tensor) -> torch.Tensor:
    """sum_sq [B] of a [B, rows, cols] tensor in the order the header states, through the host mirror: the f32 squares of each row
    cut into units of E, a non-finite element's square replaced by zero (it is skipped; x + 0 = x for these non-negative terms)"""
    from visualcloze_amd.reduction import ordered_sum
    B, rows, cols = x.shape
    E = 4 if x.dtype == torch.float32 else 8
    upr = (cols + E - 1) // E
    v = x.detach().cpu().to(torch.float32)
    sq = torch.where(torch.isfinite(v), v * v, torch.zeros(()))
    terms = torch.zeros(B, rows, upr * E, dtype=torch.float32)
    terms[:, :, :cols] = sq
    return torch.stack([ordered_sum(terms[b].reshape(rows * upr, E), max_blocks=256) for b in range(B)])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_sum_sq_has_the_bits_of_the_stated_order(dtype):
    """vc_tensor_stats.sum_sq against reduction.ordered_sum, f32 bit for bit, B = 3 with different data per sample: a partial single
    block, a second block that is nearly empty, a second round of the capped grid (one 16-byte unit per row), short units on the
    element path (6 columns of rows 11 apart), and non-finite elements, which the sum skips."""
    E = 4 if dtype == torch.float32 else 8
    inf, nan = float("inf"), float("nan")
    planted = _values((3, 1, 257 * E), dtype, 34)
    planted[0, 0, 0], planted[0, 0, 5], planted[1, 0, 256 * E], planted[2, 0, 257 * E - 1], planted[2, 0, 300] = nan, inf, -inf, nan, inf
    cases = [("9 units", _values((3, 1, 9 * E), dtype, 31).to(DEV)),
             ("257 units", _values((3, 1, 257 * E), dtype, 32).to(DEV)),
             ("256 * 256 + 8 units", _values((3, 256 * 256 + 8, E), dtype, 33).to(DEV)),
             ("cols 6 of ld 11", _values((3, 300, 11), dtype, 35).to(DEV)[:, :, :6]),
             ("257 units, non-finite planted", planted.to(DEV))]
    from visualcloze_amd import hip
    for name, x in cases:
        rec = hip.stats_to_numpy(_stats(x))
        got, want = torch.from_numpy(rec["sum_sq"].astype(np.float32)), _ordered_sum_sq(x)
        worst = _check(rec, x, name)
        print(f"tensor_stats {name} {dtype}: sum_sq {got.tolist()} mirror {want.tolist()}, {worst:.3f} of the fp64 budget")
        assert torch.equal(got, want), (name, got, want)
    assert int(hip.stats_to_numpy(_stats(cases[-1][1]))["nonfinite"].sum()) == 5


def test_row_ptr_writes_its_row_and_nothing_else(cases):
    from visualcloze_amd import hip
    name, x = cases[1]
    B, cap = x.shape[0], 3
    want = _stats(x)
    for row in (0, 1, 2, 3, -1, 1 << 20):            # 3 == capacity and everything outside writes nothing at all
        log = torch.full((cap * B * 16,), 0xAB, dtype=torch.uint8, device=DEV)
        ptr = torch.tensor([row], dtype=torch.int32, device=DEV)
        _stats(x, out=log, row_ptr=ptr, capacity=cap)
        rows = log.view(cap, B * 16)
        for r in range(cap):
            if r == row:
                assert torch.equal(rows[r], want), (row, r)
            else:
                assert bool((rows[r] == 0xAB).all()), (row, r)
    assert hip.stats_to_numpy(want)["count"].tolist() == [192, 192]


# ------------------------------------------------------------------------------------------ handle level
T, B = 64, 2


def _model():
    from tests.helpers import tiny_model
    return tiny_model()[0]


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def inputs():
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=B, rows_hw=((8, 24), (8, 24)), T=T, seed=21)
    assert inp["x"].shape[1] == 96
    return inp


def _kw(inp):
    return dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                cond=inp["cond"].to(DEV, torch.bfloat16), guidance=inp["guidance"].to(DEV))


def _grid(points, N):
    from visualcloze_amd.transport import solver_time_grid
    return solver_time_grid(points, N, 0.0, 1, True, 1)


def _run(m, inp, method, points, level, dtype=torch.bfloat16, capacity=None, cond=None, taps=None, step_cache=None):
    """one trajectory on the model's C handle, driven directly: (final state, trajectory, monitor log or None, report or None)"""
    from visualcloze_amd import hip
    h, kw = m.handle(), _kw(inp)
    S, E = points - 1, hip.solver_evals(method)
    t = _grid(points, inp["x"].shape[1])
    st = m.engine().stream
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.set_step_cache(step_cache)
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], S * E, stream=s)
        h.set_monitor(level, S * E if capacity is None else capacity)
        bufs = {}
        try:
            for n in (taps or []):
                bufs[n] = torch.empty(*h.tap_shape(n), dtype=torch.bfloat16, device=DEV)
                h.set_tap(n, bufs[n])
            x = inp["x"].to(DEV, dtype).clone()
            traj = torch.empty((S,) + tuple(x.shape), dtype=dtype, device=DEV)
            h.sample_ode(method, x, kw["cond"] if cond is None else cond, t, dtype == torch.bfloat16, s, trajectory=traj)
            log = h.monitor_log(s) if level else None
            bad = h.monitor_report(s) if level else None
        finally:
            for n in bufs:
                h.set_tap(n, None)
            h.set_monitor(0)
            h.set_step_cache(None)
    torch.cuda.synchronize()
    return x, traj, log, bad, bufs


def _rec(log, site, ev):
    """the records [B] of one site and evaluation as a structured array"""
    from visualcloze_amd import hip
    out = np.zeros(log[site]["count"].shape[1], dtype=hip.STAT_DTYPE)
    for f in FIELDS:
        out[f] = log[site][f][ev]
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("method,points", [("euler", 4), ("rk4", 3)])
def test_monitor_changes_no_bit_of_a_trajectory(inputs, method, points, dtype):
    """a handle that never heard of the monitor, the same handle at level 2, and with the monitor off again: one trajectory, bit for
    bit, and (vc_flux_step_nodes) the captured step of the off plan has the node count of the never-set one - with level 2 on, two
    kernel nodes more per site."""
    m = _model()
    x0, t0, log0, _, _ = _run(m, inputs, method, points, 0, dtype)
    h = m.handle()
    assert log0 is None and h._monitor is None
    never = h.step_nodes()
    x2, t2, log, bad, _ = _run(m, inputs, method, points, 2, dtype)
    on = h.step_nodes()
    x3, t3, _, _, _ = _run(m, inputs, method, points, 0, dtype)
    assert torch.equal(x0, x2) and torch.equal(t0, t2) and torch.equal(x0, x3) and torch.equal(t0, t3)
    assert never[0] > 20 and never[1:] == (0, 0) and h.step_nodes() == never
    assert on == (never[0] + 2 * len(log), 0, 0) and len(log) == 10
    assert bad is None and all(int(v["nonfinite"].sum()) == 0 for v in log.values())
    evals = (points - 1) * (4 if method == "rk4" else 1)
    assert all(v["count"].shape == (evals, B) for v in log.values())
    # "x" is the state behind the solver's update, read in the state's own dtype: after the last evaluation of step i it is traj[i]
    E = evals // (points - 1)
    for i in range(points - 1):
        _check(_rec(log, "x", i * E + E - 1), t0[i], f"x after step {i}")


def test_level_2_log_against_taps_of_a_second_handle(model, inputs):
    """the last evaluation of a trajectory (its taps stay in the buffers) and one vc_flux_forward"""
    m2 = _model()
    names = m2.handle().tap_names()
    _, _, log, bad, _ = _run(model, inputs, "euler", 4, 2)
    _, _, _, _, taps = _run(m2, inputs, "euler", 4, 0, taps=names)
    assert bad is None and sorted(log) == sorted(names + ["v", "x"])
    D = 256
    for n in names:
        _check(_rec(log, n, 2), taps[n].reshape(B, -1, D), f"trajectory {n}")
    # one forward: row 0 of a zeroed log, "x" stays zeroed
    img = torch.cat((inputs["x"], inputs["cond"]), -1).to(DEV, torch.bfloat16)
    kw = {k: v for k, v in _kw(inputs).items() if k != "cond"}
    tt = torch.tensor([0.7, 0.3], device=DEV)
    model.monitor = 2
    try:
        out = model(img, timesteps=tt, **kw)
    finally:
        model.monitor = 0
    torch.cuda.synchronize()
    flog = model.last_monitor_log[0]
    ref = m2.block_taps(img, timesteps=tt, **kw)
    for n in names:
        assert flog[n]["count"].shape == (1, B)
        _check(_rec(flog, n, 0), ref[n].reshape(B, -1, D), f"forward {n}")
    _check(_rec(flog, "v", 0), out, "forward v")
    assert torch.equal(out, ref["out"]) and int(flog["x"]["count"].sum()) == 0


def test_v_and_x_rows_of_every_evaluation(model, inputs):
    """"v" against velocities recomputed with vc_flux_forward from the returned trajectory, "x" against the trajectory itself"""
    from visualcloze_amd.transport import model_times
    x_end, traj, log, bad, _ = _run(model, inputs, "euler", 4, 1)
    assert bad is None and sorted(log) == ["v", "x"]
    x0 = inputs["x"].to(DEV, torch.bfloat16)
    ts = model_times(_grid(4, 96), x0)
    kw = {k: v for k, v in _kw(inputs).items() if k != "cond"}
    cond = inputs["cond"].to(DEV, torch.bfloat16)
    for i in range(3):
        state = x0 if i == 0 else traj[i - 1]
        v = model(torch.cat((state, cond), -1), timesteps=ts[i].expand(B).to(DEV), **kw)
        torch.cuda.synchronize()
        _check(_rec(log, "v", i), v, f"v of evaluation {i}")
        _check(_rec(log, "x", i), traj[i], f"x of evaluation {i}")
    assert torch.equal(traj[2], x_end)


def test_a_nan_in_one_samples_cond_is_found_at_img_in(model, inputs):
    cond = inputs["cond"].to(DEV, torch.bfloat16).clone()
    cond[1, 5, 3] = float("nan")
    _, _, log, bad, _ = _run(model, inputs, "euler", 3, 2, cond=cond)
    assert bad == (0, "img_in", 1)
    assert int(log["img_in"]["nonfinite"][0, 1]) > 0
    # sample 0 never meets sample 1's rows before the streams are joined, and the text stream is clean until the first joint attention
    for site in ("img_in", "txt_in"):
        assert int(log[site]["nonfinite"][:, 0].sum()) == 0, site
    assert int(log["txt_in"]["nonfinite"].sum()) == 0
    assert int(log["v"]["nonfinite"][0, 1]) > 0 and int(log["x"]["nonfinite"][0, 1]) > 0


def test_an_inf_bias_in_single_block_0_is_found_at_single_0(inputs):
    m = _model()
    with torch.no_grad():
        m.single_blocks[0].linear2.bias[7] = float("inf")          # a bf16 inf: plain arithmetic, inf or NaN from there on
    _, _, log, bad, _ = _run(m, inputs, "euler", 3, 2)
    assert bad is not None and bad[:2] == (0, "single.0")
    for site in ("img_in", "txt_in", "double.0.img", "double.0.txt", "double.1.img", "double.1.txt"):
        assert int(log[site]["nonfinite"][0].sum()) == 0, site
    assert int(log["single.0"]["nonfinite"][0].min()) > 0 and int(log["v"]["nonfinite"][0].min()) > 0


def test_report_after_a_prepare_with_another_batch(model, inputs):
    """the report of a finished trajectory reads its rows with the B they were logged with, whatever was prepared since; a new
    forward / trajectory at another B is refused until the monitor is set again"""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    h = model.handle()
    cond = inputs["cond"].to(DEV, torch.bfloat16).clone()
    cond[1, 5, 3] = float("nan")
    one = _kw(tiny_inputs(B=1, rows_hw=((8, 24), (8, 24)), T=T, seed=22))
    t = _grid(3, 96)
    kw = _kw(inputs)
    st = model.engine().stream
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 2, stream=s)
        try:
            h.set_monitor(2, 2)                       # a log of exactly 2 evaluations x 10 sites x 2 samples
            x = inputs["x"].to(DEV, torch.bfloat16).clone()
            h.sample_ode("euler", x, cond, t, True, s)
            assert h.monitor_report(s) == (0, "img_in", 1)
            h.prepare(one["txt"], one["y"], one["guidance"], False, one["img_ids"], one["txt_ids"], 2, stream=s)      # B = 1
            assert h.monitor_report(s) == (0, "img_in", 1) and h._monitor_evals == 2
            with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*sized for B = 2, the prepared B is 1"):
                h.sample_begin(x[:1].contiguous(), one["cond"], t, True, s)
            # and the other way round: logged at B = 1, a larger batch prepared behind it
            h.set_monitor(2, 2)
            x1 = x[:1].contiguous()
            h.sample_ode("euler", x1, one["cond"], t, True, s)
            assert h.monitor_report(s) is None
            h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 2, stream=s)          # B = 2
            assert h.monitor_report(s) is None and h._monitor_evals == 2
            log = h.monitor_log(s)
            assert log["single.1"]["count"].shape == (2, 1) and (log["single.1"]["count"] == (T + 96) * 256).all()
        finally:
            h.set_monitor(0)
    torch.cuda.synchronize()


def test_refusals(model, inputs):
    from visualcloze_amd import hip
    h, kw = model.handle(), _kw(inputs)
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*capacity_evals = 2"):          # 3 evaluations into a log of 2: VC_ERR_ARG
        _run(model, inputs, "euler", 4, 1, capacity=2)
    with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*capacity_evals = 4"):          # rk4: 2 steps are 8 evaluations
        _run(model, inputs, "rk4", 3, 1, capacity=4)
    t = _grid(4, 96)
    st = model.engine().stream
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(kw["txt"], kw["y"], kw["guidance"], False, kw["img_ids"], kw["txt_ids"], 7, stream=s)
        x = inputs["x"].to(DEV, torch.float32)
        try:
            h.set_monitor(1, 7)
            with pytest.raises(hip.VclozeHipError, match=r"\(-1\).*monitor is on"):       # dopri5: VC_ERR_ARG
                h.sample_dopri5(x.clone(), kw["cond"], t, False, s)
            h.sample_begin(x.to(torch.bfloat16), kw["cond"], t, True, s)
            h.sample_steps(1, s)
            with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*cannot change"):       # mid-trajectory: VC_ERR_STATE
                h.set_monitor(2, 7)
            with pytest.raises(hip.VclozeHipError, match=r"\(-3\).*cannot change"):
                h.set_monitor(0)
            h.sample_steps(2, s)
            h.sample_end(torch.empty(B, 96, 64, dtype=torch.bfloat16, device=DEV), s)
            assert h.monitor_report(s) is None and h._monitor_evals == 3
        finally:
            h.set_monitor(0)
    torch.cuda.synchronize()


def test_a_reused_evaluation_leaves_the_skipped_blocks_rows_zeroed(model, inputs):
    from visualcloze_amd.transport import StepCache
    _, _, log, bad, _ = _run(model, inputs, "euler", 4, 2, step_cache=StepCache(math.inf, -1))
    stats = model.handle().step_cache_stats(3)
    assert (stats["computed"], stats["reused"]) == (1, 2) and bad is None
    ran = ("img_in", "txt_in", "double.0.img", "double.0.txt", "v", "x")
    for site, v in log.items():
        assert (v["count"][0] > 0).all(), site                         # the first evaluation computes every block
        for ev in (1, 2):
            if site in ran:
                assert (v["count"][ev] > 0).all(), (site, ev)
            else:
                assert not any(v[f][ev].any() for f in FIELDS), (site, ev)


def test_python_switches(model, inputs):
    from visualcloze_amd.transport import Sampler, create_transport
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=3, do_shift=True, time_shifting_factor=1)
    x = inputs["x"].to(DEV, torch.bfloat16)
    kw = _kw(inputs)
    model.monitor, model.use_handle = 2, False
    try:
        with pytest.raises(ValueError, match="monitor needs the C handle"):      # the Python-ordered plan: never silently ignored
            fn(x, model.forward, kw)
        model.use_handle = True
        clean = fn(x, model.forward, kw)
        assert model.last_monitor_report is None and len(model.last_monitor_log) == 1
        assert model.last_monitor_log[0]["single.1"]["count"].shape == (2, B)
        model.monitor = 0
        assert torch.equal(clean, fn(x, model.forward, kw))
        model.monitor = 2
        bad = dict(kw)
        bad["cond"] = kw["cond"].clone()
        bad["cond"][1, 5, 3] = float("nan")
        fn(x, model.forward, bad)                                                # not strict: the report alone
        assert model.last_monitor_report == (0, 0, "img_in", 1)
        model.monitor_strict = True
        with pytest.raises(FloatingPointError, match=r"evaluation 0, site 'img_in', sample 1"):
            fn(x, model.forward, bad)
    finally:
        model.monitor, model.monitor_strict, model.use_handle = 0, False, True
    assert model.handle()._monitor is None
