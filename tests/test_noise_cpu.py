"""CPU: the noise stream of include/vcloze_hip.h ("noise source") restated on the host (tests/noise_ref.py) - known answers,
moments, the error budget with its mutants - and the host-only surface of vc_randn / vc_randn_tokens: exported, declared, bound,
argument errors before any device work, `pipeline.NoiseStream` bookkeeping.

The budget (tests/budget.py's constants; no figure here comes from a device):
    bf16 output   |got - ref64| <= HALF * ulp_bf16(STORE) + (1/64) * ulp_bf16(r)
    f32 output    |got - ref64| <= (1/64) * ulp_bf16(r)
(1/64) ulp_bf16 is the project's allowance for f32 arithmetic and intrinsics between two roundings; it is taken at the Box-Muller
radius r because the error of cos / sin is absolute and r scales it.  ulp_bf16(r) > 2^-8 r, so the allowance is at least
2^-14 r, where ln, sqrt, cos / sin and the product, a few f32 ulps each, add up to about 2^-21 r.  EVERY element is checked."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import noise_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC_ERR_ARG = -1
P = 0x10000000          # a 16-byte aligned stand-in for a device pointer; never dereferenced
N = 1 << 16
SEED = 1234


@pytest.fixture(scope="module", autouse=True)
def contract():
    """what these tests restate is the header's text: without the entry points there is no contract to hold anything to"""
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    assert re.search(r"\bint vc_randn\s*\(", hdr) and "Philox4x32-10" in hdr, "include/vcloze_hip.h declares no noise source"


@pytest.fixture(scope="module")
def L():
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


@pytest.fixture(scope="module")
def draw():
    """the 2^16 positions at seed 1234: words [N/4, 4], fp64 normals and radii (computed once, never written)"""
    x = R.blocks_np(SEED, np.arange(N // 4, dtype=np.uint64))
    z, r = R.normals_from_words64(x)
    for a in (x, z, r):
        a.setflags(write=False)
    return x, z, r


KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter, key, out", KNOWN)
def test_philox_known_answers(counter, key, out):
    assert R.philox4x32_10(counter, key) == out


def test_vectorised_restatement_equals_the_integer_one():
    for seed in (0, SEED, (1 << 64) - 1, 0x9E3779B97F4A7C15):
        for b in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 62) - 1):
            assert tuple(int(v) for v in R.blocks_np(seed, np.asarray([b], dtype=np.uint64))[0]) == R.block(seed, b)
    # positions: offset + i, element p & 3 of block p >> 2, across the carry of the block counter into its second word
    for offset, n in ((0, 9), (3, 6), ((1 << 34) - 3, 7), ((1 << 64) - 5, 5)):
        assert [int(v) for v in R.words(SEED, offset, n)] == [R.word(SEED, offset + i) for i in range(n)]
    # the header's first known answer is block 0 of seed 0
    assert R.block(0, 0) == KNOWN[0][2]


def test_moments_of_2_16_positions(draw):
    _, z, _ = draw
    z = z.reshape(-1)
    mean, std, m4, big = float(z.mean()), float(z.std()), float((z ** 4).mean()), float(np.abs(z).max())
    print(f"mean {mean:.4f} std {std:.4f} fourth moment {m4:.3f} max|z| {big:.3f}")
    assert abs(mean) < 0.02
    assert abs(std - 1.0) < 0.01
    assert abs(m4 - 3.0) < 0.1
    assert big <= 5.78
    assert R.R_MAX < 5.78


def test_f32_emulation_meets_the_budget_on_every_element(draw):
    x, z, r = draw
    got = R.normals_from_words_f32(x)
    wf = R.worst(got, z, R.budget_f32(z, r))
    wb = R.worst(R.to_bf16(got), z, R.budget_bf16(z, r))
    print(f"worst |err| / budget over {N} elements: f32 {wf:.4f}, bf16 {wb:.4f}")
    assert wf <= 1.0 and wb <= 1.0


EDGE = np.asarray([[0x00000000, 0x00000000, 0xffffffff, 0x40000000],     # u1 = 2^-24: r = sqrt(48 ln 2); u1 = 1: r = 0
                   [0x000000ff, 0x80000000, 0xffffff00, 0xc0000000]], dtype=np.uint32)


def _edge_ok(mutant: str) -> bool:
    """the formula's two ends, exactly: the largest r is finite, u1 = 1 gives 0, and the pair order is (cos, sin)"""
    got = R.normals_from_words_f32(EDGE, mutant)
    z, r = R.normals_from_words64(EDGE)
    if not np.isfinite(got).all() or R.worst(got, z, R.budget_f32(z, r)) > 1.0:
        return False
    return abs(float(got[0, 0]) - R.R_MAX) < 1e-5 and got[0, 2] == 0 and got[0, 3] == 0 and abs(float(got[1, 0]) + R.R_MAX) < 1e-5


def test_formula_edges():
    z, r = R.normals_from_words64(EDGE)
    assert abs(r[0, 0] - R.R_MAX) < 1e-12 and r[0, 2] == 0.0 and float(np.abs(z).max()) <= R.R_MAX
    assert _edge_ok("")


@pytest.mark.parametrize("mutant", ["u1_no_plus_one", "sincos_swapped", "pairs_swapped"])
def test_mutants_break_the_budget_or_the_exact_tests(draw, mutant):
    x, z, r = draw
    got = R.normals_from_words_f32(x, mutant)
    wf = R.worst(got, z, R.budget_f32(z, r))
    wb = R.worst(R.to_bf16(got), z, R.budget_bf16(z, r))
    edge = _edge_ok(mutant)
    print(f"{mutant}: f32 x{wf:.3g}, bf16 x{wb:.3g}, edges {'pass' if edge else 'fail'}")
    assert wf > 1.0 or not edge
    assert wb > 1.0 or not edge
    if mutant != "u1_no_plus_one":       # (that one moves u1 by 2^-24 / u1: it shows where u1 is small, and exactly at u1 = 0)
        assert wf > 1.0 and wb > 1.0


# ---------------------------------------------------------------- the C ABI, host side only
def test_entry_points_are_declared_exported_and_bound_without_an_abi_bump(L):
    from visualcloze_amd import hip
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    assert re.search(r"#define VC_ABI_VERSION 11\b", hdr) and hip.ABI_VERSION == 11 and L.vc_abi_version() == 11
    for name, nargs in (("vc_randn", 6), ("vc_randn_tokens", 9)):
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in hip.SYMBOLS and len(hip.SYMBOLS[name][1]) == nargs and hasattr(C.CDLL(hip.LIB_PATH), name)
    assert [int(re.search(r"#define VC_RNG_%s (\d+)" % n, hdr).group(1)) for n in ("BF16", "F32", "U32")] == \
        [hip.RNG_BF16, hip.RNG_F32, hip.RNG_U32]
    for text in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "6627e8d5 e169c58d bc57ac4c 9b00dbd8",
                 "408f276d 41c83b0e a20bc7c6 6d5451fd", "d16cfe09 94fdcceb 5001e420 24126ea1"):
        assert text in hdr                     # the stream's contract is the header's text
    assert callable(hip.randn) and callable(hip.randn_tokens)


@pytest.mark.parametrize("kw, word", [
    (dict(out=None), "null"),
    (dict(n=0), "n >= 1"),
    (dict(n=-5), "n >= 1"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(offset=(1 << 64) - 3, n=4), "wraps"),
    (dict(offset=(1 << 64) - 1, n=2), "wraps"),
    (dict(out=P + 1, dtype=0), "aligned"),
    (dict(out=P + 2, dtype=1), "aligned"),
    (dict(out=P + 2, dtype=2), "aligned"),
])
def test_randn_argument_errors_come_back_before_any_device_work(L, kw, word):
    a = dict(out=P, dtype=0, n=16, seed=1, offset=0)
    a.update(kw)
    assert L.vc_randn(a["out"], a["dtype"], a["n"], a["seed"], a["offset"], None) == VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert msg.startswith("randn:") and word in msg, msg


@pytest.mark.parametrize("kw, word", [
    (dict(tokens=None), "null"),
    (dict(C=0), "even"),
    (dict(C=15), "even"),
    (dict(h=3), "even"),
    (dict(w=5), "even"),
    (dict(h=0), "even"),
    (dict(w=-2), "even"),
    (dict(ld=68), "multiples of 8"),
    (dict(col0=4), "multiples of 8"),
    (dict(ld=64, col0=8), "col0 + 4C <= ld"),
    (dict(tokens=P + 8), "16-byte"),
    (dict(offset=(1 << 64) - 16 * 4 * 6 + 1), "wraps"),
    (dict(C=1 << 30, h=1 << 30, w=1 << 30, ld=1 << 40), "wraps"),
])
def test_randn_tokens_argument_errors_come_back_before_any_device_work(L, kw, word):
    a = dict(tokens=P, C=16, h=4, w=6, ld=64, col0=0, seed=1, offset=0)
    a.update(kw)
    assert L.vc_randn_tokens(a["tokens"], a["C"], a["h"], a["w"], a["ld"], a["col0"], a["seed"], a["offset"], None) == VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert msg.startswith("randn_tokens:") and word in msg, msg


def test_the_last_stream_position_is_a_legal_one(L):
    """offset + n may reach 2^64 (the last position is 2^64 - 1): only the null pointer is left to object to"""
    assert L.vc_randn(None, 0, 4, 1, (1 << 64) - 4, None) == VC_ERR_ARG and b"null" in L.vc_last_error()


# ---------------------------------------------------------------- pipeline.NoiseStream
def test_noise_stream_offset_bookkeeping(monkeypatch):
    from visualcloze_amd import hip, pipeline
    calls = []

    def fake(shape, seed, offset=0, dtype=torch.bfloat16, device=None, out=None, stream=None):
        calls.append((tuple(shape), seed, offset, dtype))
        return torch.zeros(shape, dtype=dtype)
    monkeypatch.setattr(hip, "randn", fake)
    s = pipeline.NoiseStream(77)
    assert s.seed == 77 and s.offset == 0
    a = s.randn([1, 16, 4, 8])
    b = s.randn((3, 5), torch.float32)
    assert a.shape == (1, 16, 4, 8) and a.dtype == torch.bfloat16 and b.dtype == torch.float32
    assert s.offset == 512 + 15
    s.offset = 1 << 34
    s.randn([7])
    assert s.offset == (1 << 34) + 7
    assert calls == [((1, 16, 4, 8), 77, 0, torch.bfloat16), ((3, 5), 77, 512, torch.float32), ((7,), 77, 1 << 34, torch.bfloat16)]
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            s.offset = bad
    s.offset = (1 << 64) - 4
    with pytest.raises(ValueError):
        s.randn([5])                       # would leave the stream; nothing was drawn, nothing moved
    assert s.offset == (1 << 64) - 4 and len(calls) == 3
    s.randn([4])                           # ... the last four positions are fine
    assert s.offset == 1 << 64             # exhausted: any further draw is refused
    with pytest.raises(ValueError):
        s.randn([0])
    assert pipeline.NoiseStream(5, offset=9).offset == 9


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_host_program_compiles_and_links_as_c99(L, tmp_path):
    """tests/c_abi/noise_demo.c names nothing but the C ABI and the HIP runtime (it runs in tests/test_noise_gpu.py)"""
    from visualcloze_amd import hip
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(hip.LIB_PATH)
    exe = str(tmp_path / "noise_demo")
    r = subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(rocm, "include"),
                        os.path.join(REPO, "tests", "c_abi", "noise_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip",
                        "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(exe) > 0
