"""model.ChunkPlan on the CPU: how one call's batch becomes chunks of `FluxHandle.prepare` arguments and kernel-order rows.
CPU tensors, torch.device("cpu") and a fake handle that records what `prepare` was given."""
import pytest
import torch

from tests.procedural import TINY
from visualcloze_amd import hip
from visualcloze_amd.model import ChunkPlan, FluxParams
from visualcloze_amd.transport import cfg_chunks

CPU = torch.device("cpu")
PARAMS = FluxParams(**TINY)
T, N, CTX, VEC = 6, 8, 5, 3


class FakeHandle:
    def __init__(self):
        self.calls = []

    def prepare(self, txt, y, guidance, guidance_is_bf16, img_ids, txt_ids, max_steps, kv_len=None, kv_gap=None, stream=None):
        self.calls.append(dict(txt=txt, y=y, guidance=guidance, guidance_is_bf16=guidance_is_bf16, img_ids=img_ids, txt_ids=txt_ids,
                               max_steps=max_steps, kv_len=kv_len, kv_gap=kv_gap, stream=stream))


def _tensors(B):
    """every row of every tensor holds its own number 8 * sample + row (exact in bf16): a moved row is seen"""
    rows = lambda n, c: (torch.arange(B)[:, None, None] * 8 + torch.arange(n)[None, :, None] + torch.zeros(c)).float()  # noqa: E731
    return dict(txt=rows(T, CTX), y=torch.arange(B)[:, None] + torch.zeros(VEC), guidance=torch.arange(B) + 1.0,
                img_ids=rows(N, 3) + 0.5, txt_ids=rows(T, 3) + 0.25)


def _plan(B, max_batch=4, pairs=False, txt_mask=None, img_mask=None, params=PARAMS, channels=None, **over):
    t = dict(_tensors(B), **over)
    return ChunkPlan(B, N, t["txt"], t["y"], t["guidance"], t["img_ids"], t["txt_ids"], txt_mask, img_mask, params, CPU, max_batch,
                     pairs=pairs, channels=channels), t


def _prepared(plan, sl, max_evals=3, stream=17):
    h = FakeHandle()
    h.prepare(*plan.prepare_args(sl, max_evals), stream=stream)
    (call,) = h.calls
    assert call["max_steps"] == max_evals and call["stream"] == stream
    return call


# ---------------------------------------------------------------------------------------------- chunks
def test_plain_chunking():
    plan, _ = _plan(5)
    assert plan.chunks == [slice(0, 4), slice(4, 5)]
    assert [plan.size(sl) for sl in plan.chunks] == [4, 1]
    assert _plan(1)[0].chunks == [slice(0, 1)]
    assert _plan(8)[0].chunks == [slice(0, 4), slice(4, 8)]
    assert [plan.size(sl) for sl in _plan(3, max_batch=1)[0].chunks] == [1, 1, 1]


def test_pair_chunking():
    plan, _ = _plan(6, pairs=True)
    assert plan.chunks == cfg_chunks(6, 4) == [[0, 1, 3, 4], [2, 5]]
    assert [plan.size(sl) for sl in plan.chunks] == [4, 2]
    with pytest.raises(ValueError, match="true CFG needs an even batch"):
        _plan(5, pairs=True)


# ---------------------------------------------------------------------------------------------- masks
def test_no_masks():
    plan, t = _plan(5)
    for sl in plan.chunks:
        call = _prepared(plan, sl)
        bs = plan.size(sl)
        assert call["kv_len"] == [T + N] * bs and call["kv_gap"] is None
        assert call["txt"].dtype == torch.bfloat16 and torch.equal(call["txt"].float(), t["txt"][sl])
        assert call["y"].dtype == torch.bfloat16 and torch.equal(call["y"].float(), t["y"][sl])
        assert torch.equal(call["img_ids"], t["img_ids"][sl]) and torch.equal(call["txt_ids"], t["txt_ids"][sl])
        assert torch.equal(call["guidance"], t["guidance"][sl]) and call["guidance_is_bf16"] is False


def test_handed_over_ids_and_guidance_are_views_of_the_callers_storage():
    """handle._HostCopies keys on the memory: no copy may come between the caller's tensor and `prepare`"""
    plan, t = _plan(5)
    call = _prepared(plan, plan.chunks[1])
    for k in ("img_ids", "txt_ids", "guidance"):
        assert call[k].untyped_storage().data_ptr() == t[k].untyped_storage().data_ptr(), k
        assert call[k].storage_offset() == t[k][4:5].storage_offset()


def test_right_padded_masks_are_the_identity_row_order():
    tm, im = torch.ones(2, T, dtype=torch.int32), torch.ones(2, N, dtype=torch.int32)
    tm[0, 4:] = 0
    im[1, 5:] = 0
    plan, t = _plan(2, txt_mask=tm, img_mask=im)
    call = _prepared(plan, slice(0, 2))
    assert torch.equal(call["txt"].float(), t["txt"]) and torch.equal(call["txt_ids"], t["txt_ids"])
    assert torch.equal(call["img_ids"], t["img_ids"])
    assert call["kv_len"] == [T + N, T + 5] and call["kv_gap"] == [(4, T), (0, 0)]
    x = torch.randn(2, N, 4)
    assert torch.equal(plan.img_rows(x, slice(0, 2), torch.float32), x)


def test_holes_in_both_streams_and_a_sample_without_text():
    tm, im = torch.ones(3, T, dtype=torch.int32), torch.ones(3, N, dtype=torch.int32)
    tm[0, [1, 4]] = 0
    im[0, [0, 3, 6]] = 0
    tm[2] = 0                                          # no text at all
    plan, t = _plan(3, txt_mask=tm, img_mask=im)
    call = _prepared(plan, slice(0, 3))
    order_t, order_i = [0, 2, 3, 5, 1, 4], [1, 2, 4, 5, 7, 0, 3, 6]     # valid first, stable
    assert torch.equal(call["txt"][0].float(), t["txt"][0][order_t])
    assert torch.equal(call["txt_ids"][0], t["txt_ids"][0][order_t])
    assert torch.equal(call["img_ids"][0], t["img_ids"][0][order_i])
    assert torch.equal(call["txt"][1:].float(), t["txt"][1:]) and torch.equal(call["img_ids"][1:], t["img_ids"][1:])
    assert call["kv_len"] == [T + 5, T + N, T + N]
    assert call["kv_gap"] == [(4, T), (0, 0), (0, T)]
    only = _prepared(plan, [2])                        # an index list, the sample without text alone
    assert only["kv_len"] == [T + N] and only["kv_gap"] == [(0, T)]
    assert _prepared(plan, slice(1, 2))["kv_gap"] is None


# ---------------------------------------------------------------------------------------------- rows there and back
@pytest.mark.parametrize("sl", [slice(0, 4), slice(4, 6), [0, 1, 3, 4], [2, 5]], ids=str)
def test_scatter_returns_the_callers_rows(sl):
    g = torch.Generator().manual_seed(3)
    tm, im = (torch.rand(6, T, generator=g) > 0.4).int(), (torch.rand(6, N, generator=g) > 0.4).int()
    assert not tm.all() and not im.all()
    plan, _ = _plan(6, txt_mask=tm, img_mask=im)
    x, tx = torch.randn(6, N, 4, generator=g), torch.randn(6, T, 4, generator=g)
    rows = plan.img_rows(x, sl, torch.float32)
    assert rows.is_contiguous() and not torch.equal(rows, x[sl])
    assert torch.equal(plan.img_back(rows, sl), x[sl])
    assert torch.equal(plan.txt_back(plan.lay.txt_rows(tx, sl), sl), tx[sl])
    joint = torch.cat((plan.lay.txt_rows(tx, sl), rows), dim=1)          # a single-stream tap: text rows, then image rows
    assert torch.equal(plan.joint_back(joint, sl), torch.cat((tx[sl], x[sl]), dim=1))
    assert plan.img_rows(x, sl, torch.bfloat16).dtype == torch.bfloat16


def test_state_rows_are_a_copy_when_asked():
    plan, _ = _plan(2)
    x = torch.randn(2, N, 4)
    assert plan.img_rows(x, slice(0, 2), torch.float32).data_ptr() == x.data_ptr()
    xs = plan.img_rows(x, slice(0, 2), torch.float32, copy=True)
    assert xs.data_ptr() != x.data_ptr() and torch.equal(xs, x)


# ---------------------------------------------------------------------------------------------- guidance and validation
def test_guidance():
    plan, _ = _plan(5, guidance=torch.full((1,), 30.0))
    assert [_prepared(plan, sl)["guidance"].tolist() for sl in plan.chunks] == [[30.0] * 4, [30.0]]
    plan, _ = _plan(5, guidance=torch.full((5,), 3.5, dtype=torch.bfloat16))
    assert _prepared(plan, plan.chunks[0])["guidance_is_bf16"] is True
    with pytest.raises(ValueError, match="expected 1 or 5 per-sample values, got 3"):
        _plan(5, guidance=torch.ones(3))
    with pytest.raises(ValueError, match="Didn't get guidance strength for guidance distilled model."):
        _plan(5, guidance=None)
    no_embed = FluxParams(**dict(TINY, guidance_embed=False))
    plan, _ = _plan(5, guidance=None, params=no_embed)
    call = _prepared(plan, plan.chunks[0])
    assert call["guidance"] is None and call["guidance_is_bf16"] is False


def test_state_and_cond_channels():
    _plan(2, channels=(64, 320))
    with pytest.raises(hip.VclozeHipError, match=r"x \(64\) \|\| cond \(300\) does not match in_channels 384"):
        _plan(2, channels=(64, 300))


def test_twin_arguments_are_the_same_tensors():
    tm, im = torch.ones(2, T, dtype=torch.int32), torch.ones(2, N, dtype=torch.int32)
    tm[1, 2:] = 0
    plan, _ = _plan(2, txt_mask=tm, img_mask=im)
    sl = slice(0, 2)
    ts = torch.ones(1, 2)
    args, kwargs = plan.twin_prepare_args(sl, ts)
    want = plan.prepare_args(sl, 1)
    assert len(args) == 8 and args[6] is ts and args[7] == want[7] == [T + N, T + N]
    assert kwargs == dict(kv_gap=want[8]) and want[8] == [(0, 0), (2, T)]
    for a, b in zip(args[:6], want[:6]):
        assert (a is b) or torch.equal(a, b)
