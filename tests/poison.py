"""Poisoned allocations: `poisoned_empty(byte)` replaces torch.empty, torch.empty_like and Tensor.new_empty by functions that
allocate as before and then fill every byte of the new tensor's storage with `byte` - through a uint8 view of the storage, so any
dtype, any strides, a zero-size request, the device or the CPU.  What the library is handed by `torch.empty` then holds what a C
caller's hipMalloc may hold: anything.  A helper, not a conftest: a test opens the block around the code whose buffers it wants
poisoned (a fresh model and handle built INSIDE the block have their workspace, arena and argument slots poisoned) and reads
`.count`, the allocations filled, to show the block did not pass vacuously.  On exit the originals are back.

The patterns and how the kernels' number formats read them:
    0x00   bf16 0            f32 0                        int32 0            the baseline
    0xFF   bf16 0xFFFF, NaN  f32 0xFFFFFFFF, NaN          int32 -1
    0x7F   bf16 0x7F7F = 3.39e38, finite   f32 0x7F7F7F7F = 3.39e38, finite   int32 2139062143
torch.zeros / torch.full / torch.tensor and allocations made inside torch's own C++ are not touched."""
import contextlib

import pytest
import torch

PATTERNS = (0x00, 0xFF, 0x7F)


class Poison:
    """the state of one block: the byte and the number of allocations filled so far"""

    def __init__(self, byte: int):
        if not 0 <= int(byte) <= 0xFF:
            raise ValueError(f"poisoned_empty: byte = {byte!r} is not a byte")
        self.byte = int(byte)
        self.count = 0
        self._empty = torch.empty       # the original: fill() runs while the name is patched

    def fill(self, t):
        """every byte of t's storage <- the pattern (a fresh tensor owns its storage: nothing else lives there)"""
        if not isinstance(t, torch.Tensor) or t.is_sparse or t.device.type == "meta":
            return t
        st = t.untyped_storage()
        if st.nbytes():
            self._empty(0, dtype=torch.uint8, device=t.device).set_(st).fill_(self.byte)
        self.count += 1
        return t


def holds(t: torch.Tensor, byte: int) -> bool:
    """every byte of the (contiguous) tensor t is `byte`"""
    return bool((t.contiguous().view(-1).view(torch.uint8) == byte).all())


def any_byte(t: torch.Tensor, byte: int, run: int = 16) -> bool:
    """somewhere in the (contiguous) tensor t `run` aligned consecutive bytes are all `byte`"""
    b = t.contiguous().view(-1).view(torch.uint8)
    b = b[:b.numel() // run * run].view(-1, run)
    return bool((b == byte).all(dim=1).any())


@contextlib.contextmanager
def poisoned_empty(byte: int, monkeypatch=None):
    """with poisoned_empty(0xFF) as p: ... ; p.count allocations were filled.  `monkeypatch`: pytest's fixture, or None for a
    MonkeyPatch of the block's own; either way the three names are the originals again when the block ends."""
    p = Poison(byte)
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    mp = pytest.MonkeyPatch() if monkeypatch is None else None
    with (mp.context() if mp is not None else monkeypatch.context()) as m:
        # (out=: the caller's own tensor is filled by whoever asked for it, not here)
        m.setattr(torch, "empty", lambda *a, **k: empty(*a, **k) if k.get("out") is not None else p.fill(empty(*a, **k)))
        m.setattr(torch, "empty_like", lambda *a, **k: p.fill(empty_like(*a, **k)))
        m.setattr(torch.Tensor, "new_empty", lambda self, *a, **k: p.fill(new_empty(self, *a, **k)))
        yield p


def poison_fixture(byte: int):
    """a pytest fixture that runs its test inside poisoned_empty(byte) and hands it the Poison"""
    @pytest.fixture
    def _poisoned(monkeypatch):
        with poisoned_empty(byte, monkeypatch) as p:
            yield p
    return _poisoned
