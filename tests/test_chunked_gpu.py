"""-m gpu: a batch larger than one chunk (MAX_BATCH = 4) through every entry point of the Flux front end.

One call over the whole batch must equal, bit for bit, the same entry point called once per chunk of samples: B = 5 runs as the
chunks [0:4] and [4:5], a true-CFG batch of 6 as the pairs [0, 1, 3, 4] and [2, 5].  Tiny procedural model, default grid (N = 24),
T = 16; samples 0 and 3 have holes in both masks, the text of sample 4 is right-padded."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNKS = (slice(0, 4), slice(4, 5))
CFG_CHUNKS = ([0, 1, 3, 4], [2, 5])
PER_SAMPLE = ("txt", "txt_ids", "txt_mask", "y", "img_ids", "img_mask", "cond", "guidance")


@pytest.fixture(scope="module")
def model():
    from tests.helpers import tiny_model
    return tiny_model()[0]


def _inputs(B):
    """(x [B, N, 64] f32 on the host, model_kwargs on the device)"""
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=B, T=16)
    for j in (0, 3):                                   # (a true-CFG batch of 6 pairs 0 with 3: the same image mask)
        inp["txt_mask"][j, [2, 9, 10]] = 0
        inp["img_mask"][j, [0, 5, 11, 12, 23]] = 0
    inp["txt_mask"][3, 13:] = 0                        # another text length within the pair
    inp["txt_mask"][4, 11:] = 0
    inp["guidance"] = torch.tensor([30.0, 10.0, 3.5, 1.0, 20.0, 7.0])[:B]
    kw = {k: inp[k].to(DEV, torch.bfloat16) if k in ("txt", "y", "cond") else inp[k].to(DEV) for k in PER_SAMPLE}
    return inp["x"], kw


def _rows(kw, sl):
    return {k: (v[sl] if k in PER_SAMPLE else v) for k, v in kw.items()}


def _sampler():
    from visualcloze_amd.transport import Sampler, create_transport
    return Sampler(create_transport())


def _euler(**over):
    opts = dict(sampling_method="euler", num_steps=3, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    opts.update(over)
    return _sampler().sample_ode(**opts)


def _assert_chunkwise(whole, part, chunks=CHUNKS, dim=0):
    """whole: the result over the batch; part(sl): the result over the samples sl alone"""
    torch.cuda.synchronize()
    assert torch.isfinite(whole.float()).all()
    for sl in chunks:
        got = whole[:, sl] if dim else whole[sl]
        want = part(sl)
        torch.cuda.synchronize()
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(got, want), f"samples {sl}: {(got != want).float().mean().item():.4f} of the elements differ"


def _forward_args(x, kw, ts, sl=slice(None)):
    k = _rows(kw, sl)
    img = torch.cat((x.to(DEV, torch.bfloat16), kw["cond"]), -1)[sl]
    return dict(img=img, img_ids=k["img_ids"], txt=k["txt"], txt_ids=k["txt_ids"], timesteps=ts[sl], y=k["y"], txt_mask=k["txt_mask"],
                img_mask=k["img_mask"], guidance=k["guidance"])


TIMESTEPS = torch.tensor([0.9, 0.7, 0.5, 0.3, 0.1])


def test_forward_with_per_sample_timesteps(model):
    x, kw = _inputs(5)
    ts = TIMESTEPS.to(DEV)
    whole = model.forward(**_forward_args(x, kw, ts))
    _assert_chunkwise(whole, lambda sl: model.forward(**_forward_args(x, kw, ts, sl)))
    assert not torch.equal(whole[0], whole[1])


def test_block_taps(model):
    x, kw = _inputs(5)
    ts = TIMESTEPS.to(DEV)
    whole = model.block_taps(**_forward_args(x, kw, ts))
    parts = [model.block_taps(**_forward_args(x, kw, ts, sl)) for sl in CHUNKS]
    assert "out" in whole and "txt_in" in whole and any(n.startswith("single.") for n in whole)
    assert all(set(p) == set(whole) for p in parts)
    for n, t in whole.items():
        _assert_chunkwise(t, lambda sl: parts[CHUNKS.index(sl)][n])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_euler_trajectory(model, dtype):
    x, kw = _inputs(5)
    x = x.to(DEV, dtype)
    fn = _euler()
    whole = fn(x, model.forward, kw)
    assert whole.shape == (3, 5) + x.shape[1:] and whole.dtype == dtype
    _assert_chunkwise(whole, lambda sl: fn(x[sl], model.forward, _rows(kw, sl)), dim=1)


def test_rk4(model):
    x, kw = _inputs(5)
    x = x.to(DEV, torch.bfloat16)
    fn = _euler(sampling_method="rk4", num_steps=2, return_trajectory=False)
    whole = fn(x, model.forward, kw)
    assert whole.shape == (1, 5) + x.shape[1:]
    _assert_chunkwise(whole, lambda sl: fn(x[sl], model.forward, _rows(kw, sl)), dim=1)


def test_adaptive(model):
    """one step size per chunk: chunk-wise equality is exact"""
    x, kw = _inputs(5)
    x = x.to(DEV, torch.bfloat16)
    sampler = _sampler()
    fn = sampler.sample_ode_adaptive(num_steps=2, rtol=1e-2, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    whole = fn(x, model.forward, kw)
    log = sampler.last_adaptive_log
    assert len(log) == 2 and all(entry["attempts"] for entry in log)
    assert whole.shape == (2, 5) + x.shape[1:]
    _assert_chunkwise(whole, lambda sl: fn(x[sl], model.forward, _rows(kw, sl)), dim=1)


def test_true_cfg_pairs(model):
    x, kw = _inputs(6)
    assert torch.equal(kw["img_mask"][:3], kw["img_mask"][3:])
    x = x.to(DEV, torch.bfloat16)
    kw["cfg_scale"] = 3.5
    fn = _euler()
    whole = fn(x, model.forward_with_cfg, kw)
    assert whole.shape == (3, 6) + x.shape[1:]
    _assert_chunkwise(whole, lambda sl: fn(x[sl], model.forward_with_cfg, _rows(kw, sl)), chunks=CFG_CHUNKS, dim=1)


def test_python_ordered_twin(model):
    x, kw = _inputs(5)
    ts = TIMESTEPS.to(DEV)
    xb = x.to(DEV, torch.bfloat16)
    fn = _euler()
    with_handle = fn(xb, model.forward, kw)
    model.use_handle = False
    try:
        assert model.handle() is None
        whole = model.forward(**_forward_args(x, kw, ts))
        _assert_chunkwise(whole, lambda sl: model.forward(**_forward_args(x, kw, ts, sl)))
        traj = fn(xb, model.forward, kw)
        _assert_chunkwise(traj, lambda sl: fn(xb[sl], model.forward, _rows(kw, sl)), dim=1)
    finally:
        model.use_handle = True
    assert torch.equal(traj, with_handle)


def test_monitor_logs_one_entry_per_chunk(model):
    x, kw = _inputs(5)
    x = x.to(DEV, torch.bfloat16)
    fn = _euler()
    plain = fn(x, model.forward, kw)
    model.monitor = 1
    try:
        watched = fn(x, model.forward, kw)
        torch.cuda.synchronize()
        assert len(model.last_monitor_log) == 2
        assert model.last_monitor_report is None
    finally:
        model.monitor = 0
    assert torch.equal(watched, plain)


def test_step_cache_stats_one_entry_per_chunk(model):
    from visualcloze_amd.transport import StepCache
    x, kw = _inputs(5)
    x = x.to(DEV, torch.bfloat16)
    sampler = _sampler()
    fn = sampler.sample_ode(sampling_method="euler", num_steps=4, do_shift=True, time_shifting_factor=1,
                            step_cache=StepCache(threshold=math.inf, max_consecutive=1))
    out = fn(x, model.forward, kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert len(model.last_step_cache_stats) == 2
    assert sampler.last_step_cache_stats is model.last_step_cache_stats
