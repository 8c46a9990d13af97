"""tests/poison.py on CPU tensors: how each number format reads the three byte patterns, that every patched name fills, that
strided and zero-size requests work, that the counter counts and that the originals are back after the block - also when the block
raises."""
import math

import pytest
import torch

from tests.poison import PATTERNS, any_byte, holds, poison_fixture, poisoned_empty

ORIGINALS = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


def _originals_back():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty) == ORIGINALS


def test_the_three_patterns_as_each_format_reads_them():
    assert PATTERNS == (0x00, 0xFF, 0x7F)
    with poisoned_empty(0x00) as p:
        for dt in (torch.bfloat16, torch.float32, torch.int32, torch.uint8):
            t = torch.empty(5, 3, dtype=dt)
            assert bool((t == 0).all()) and holds(t, 0x00)
    with poisoned_empty(0xFF) as p:
        b, f, i = torch.empty(7, dtype=torch.bfloat16), torch.empty(7, dtype=torch.float32), torch.empty(7, dtype=torch.int32)
        assert bool((b.view(torch.int16) == -1).all()) and bool(torch.isnan(b).all())             # 0xFFFF: a NaN
        assert bool((f.view(torch.int32) == -1).all()) and bool(torch.isnan(f).all())             # 0xFFFFFFFF: a NaN
        assert bool((i == -1).all())
        assert p.count == 3
    with poisoned_empty(0x7F) as p:
        b, f, i = torch.empty(7, dtype=torch.bfloat16), torch.empty(7, dtype=torch.float32), torch.empty(7, dtype=torch.int32)
        assert bool((b.view(torch.int16) == 0x7F7F).all()) and bool(torch.isfinite(b).all())
        assert bool((f.view(torch.int32) == 0x7F7F7F7F).all()) and bool(torch.isfinite(f).all())
        assert math.isclose(float(b[0]), 3.39e38, rel_tol=5e-3) and math.isclose(float(f[0]), 3.39e38, rel_tol=5e-3)
        assert bool((i == 2139062143).all())
        assert p.count == 3
    assert _originals_back()


def test_every_patched_name_fills_and_counts():
    src = torch.zeros(4, 6, dtype=torch.float32)
    with poisoned_empty(0x7F) as p:
        assert p.count == 0
        a = torch.empty(3, 4)
        b = torch.empty((2, 5), dtype=torch.int64)
        c = torch.empty_like(src)
        d = src.new_empty((9,))
        e = src.new_empty(2, 2, dtype=torch.uint8)
        assert p.count == 5
        for t in (a, b, c, d, e):
            assert holds(t, 0x7F)
        assert c.shape == src.shape and c.dtype == src.dtype and d.dtype == src.dtype and e.dtype == torch.uint8
        assert bool((src == 0).all())                                   # the tensor asked about is not the tensor filled
        out = torch.zeros(3)
        torch.empty(3, out=out)                                         # the caller's own tensor stays the caller's
        assert p.count == 5 and bool((out == 0).all())
    assert _originals_back()
    assert torch.zeros(3).sum() == 0


def test_strided_and_zero_size_requests():
    with poisoned_empty(0xFF) as p:
        z = torch.empty(0, dtype=torch.bfloat16)
        z2 = torch.empty(4, 0, 3)
        assert z.numel() == 0 and z2.shape == (4, 0, 3) and p.count == 2
        cl = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        assert cl.stride() == (60, 1, 15, 3) and holds(cl, 0xFF)
        base = torch.zeros(6, 8)[:, ::2]                                # a strided tensor: empty_like keeps or packs, both filled
        like = torch.empty_like(base)
        assert like.shape == base.shape and bool(torch.isnan(like).all())
        tr = torch.empty_like(torch.zeros(5, 7).t())                    # preserve_format: the transposed strides
        assert tr.shape == (7, 5) and bool(torch.isnan(tr).all())
        view = torch.empty(32, dtype=torch.uint8)[5:21]                 # the bytes around a view are the pattern too
        assert holds(view, 0xFF) and any_byte(view, 0xFF)
        assert p.count == 6
    assert not any_byte(torch.zeros(64, dtype=torch.uint8), 0xFF)


def test_the_patch_is_undone_when_the_block_raises_and_with_pytests_own_monkeypatch(monkeypatch):
    with pytest.raises(RuntimeError, match="inside"):
        with poisoned_empty(0xFF):
            assert torch.empty is not ORIGINALS[0]
            raise RuntimeError("inside")
    assert _originals_back()
    with poisoned_empty(0x7F, monkeypatch) as p:
        assert torch.empty is not ORIGINALS[0] and holds(torch.empty(3), 0x7F) and p.count == 1
    assert _originals_back()
    with pytest.raises(ValueError, match="not a byte"):
        with poisoned_empty(256):
            pass
    assert _originals_back()


poisoned_ff = poison_fixture(0xFF)


def test_the_fixture_factory(poisoned_ff):
    assert bool(torch.isnan(torch.empty(4)).all()) and poisoned_ff.count == 1 and poisoned_ff.byte == 0xFF


def test_after_the_fixture_the_originals_are_back():
    assert _originals_back()
