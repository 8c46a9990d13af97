"""Host restatement of the library's noise stream (include/vcloze_hip.h, "noise source"; csrc/rng.hip), from the header's text alone.

    philox4x32_10(counter, key)      integer Python, one block: the known answers of the header are checked against THIS
    words(seed, offset, n)           the raw words x[p & 3] of positions offset .. offset + n (numpy uint32; VC_RNG_U32)
    normals64(seed, offset, n)       (z, r): the fp64 value of every element and the Box-Muller radius it was scaled by
    normals_from_words_f32(x)        a numpy-f32 emulation of the formula on given blocks of words (what a device computes)
    budget_bf16 / budget_f32         the per-element error budget of a bf16 / f32 draw against normals64

The vectorised functions do the same integer arithmetic in numpy uint64 (a 32 x 32 bit product fits); tests/test_noise_cpu.py
holds them to the integer-Python block function word for word.
"""
import math

import numpy as np
import torch

from tests import budget as B

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
R_MAX = math.sqrt(48.0 * math.log(2.0))          # u1 = 2^-24


def philox4x32_10(counter, key):
    """counter (c0, c1, c2, c3), key (k0, k1): Python ints -> (x0, x1, x2, x3)"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def block(seed: int, b: int):
    """the four words of stream block b of `seed` (integer Python)"""
    return philox4x32_10((b & MASK32, b >> 32, 0, 0), (seed & MASK32, seed >> 32))


def word(seed: int, p: int) -> int:
    return block(seed, p >> 2)[p & 3]


def blocks_np(seed: int, b: np.ndarray) -> np.ndarray:
    """b: uint64 block numbers [m] -> uint32 words [m, 4]"""
    b = np.asarray(b, dtype=np.uint64)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    c0, c1 = b & m32, b >> s32
    c2, c3 = np.zeros_like(b), np.zeros_like(b)
    k0, k1 = seed & MASK32, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _span(offset: int, n: int):
    """block numbers covering positions offset .. offset + n, and the slice of their 4 m words that the positions are"""
    assert n >= 1 and 0 <= offset and offset + n <= 1 << 64
    b0, b1 = offset >> 2, (offset + n - 1) >> 2
    b = np.uint64(b0) + np.arange(b1 - b0 + 1, dtype=np.uint64)
    lo = offset & 3
    return b, slice(lo, lo + n)


def words(seed: int, offset: int, n: int) -> np.ndarray:
    b, sl = _span(offset, n)
    return blocks_np(seed, b).reshape(-1)[sl]


def normals_from_words64(x: np.ndarray):
    """x: uint32 [m, 4] -> (z [m, 4], r [m, 4]) in fp64; u1, u2 are exact"""
    x = np.asarray(x, dtype=np.uint32).astype(np.uint64)
    u1 = ((x[:, 0::2] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (x[:, 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(x.shape, dtype=np.float64)
    z[:, 0::2], z[:, 1::2] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return z, np.repeat(r, 2, axis=1)


def normals64(seed: int, offset: int, n: int):
    b, sl = _span(offset, n)
    z, r = normals_from_words64(blocks_np(seed, b))
    return z.reshape(-1)[sl], r.reshape(-1)[sl]


def normals_from_words_f32(x: np.ndarray, mutant: str = "") -> np.ndarray:
    """The formula in numpy float32, every operation rounded to f32: x uint32 [m, 4] -> z float32 [m, 4].
    mutant: "" (the formula), or one of the three wrong ones the tests must catch -
      "u1_no_plus_one"   u1 = (x0 >> 8) * 2^-24, which can be 0
      "sincos_swapped"   z0 = r sin, z1 = r cos
      "pairs_swapped"    (z2, z3, z0, z1)"""
    assert mutant in ("", "u1_no_plus_one", "sincos_swapped", "pairs_swapped")
    x = np.asarray(x, dtype=np.uint32)
    one = np.uint32(0 if mutant == "u1_no_plus_one" else 1)
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        u1 = ((x[:, 0::2] >> np.uint32(8)) + one).astype(f) * f(2.0 ** -24)
        u2 = (x[:, 1::2] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
        r = np.sqrt(f(-2.0) * np.log(u1)).astype(f)
        th = f(2.0 * math.pi) * u2
        c, s = (r * np.cos(th)).astype(f), (r * np.sin(th)).astype(f)
    if mutant == "sincos_swapped":
        c, s = s, c
    z = np.empty(x.shape, dtype=f)
    z[:, 0::2], z[:, 1::2] = c, s
    if mutant == "pairs_swapped":
        z = z[:, [2, 3, 0, 1]]
    return z


def to_bf16(z32: np.ndarray) -> torch.Tensor:
    """float32 -> bf16, round to nearest even (torch's .to(bfloat16))"""
    return torch.from_numpy(np.ascontiguousarray(z32, dtype=np.float32)).to(torch.bfloat16)


# ---------------------------------------------------------------- the error budget (tests/budget.py's constants)
def _t64(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a, dtype=np.float64))


def f32_term(r64) -> torch.Tensor:
    """(1/64) ulp_bf16(r): the project's allowance for f32 arithmetic and intrinsics between two roundings (HALF - 1/2 of
    tests/budget.py), taken at r because the error of cos / sin is absolute: it is scaled by r, not by |z|"""
    return (B.HALF - 0.5) * B.ulp_bf16(_t64(r64))


def budget_bf16(z64, r64) -> torch.Tensor:
    """|got - ref64| <= HALF * ulp_bf16(STORE) + (1/64) * ulp_bf16(r)"""
    return B.budget(_t64(z64), roundings=1, mags=[B.STORE], f32_terms=f32_term(r64))


def budget_f32(z64, r64) -> torch.Tensor:
    """|got - ref64| <= (1/64) * ulp_bf16(r)"""
    return B.budget(_t64(z64), roundings=0, f32_terms=f32_term(r64))


def worst(got, z64, bud) -> float:
    """max |got - ref64| / budget over ALL elements, inf for a non-finite result"""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64).reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - _t64(z64).reshape(-1)).abs() / bud.reshape(-1)).max())


def fnv64(data: bytes) -> int:
    """64-bit FNV-1a of a byte string (what tests/c_abi/noise_demo.c prints)"""
    h = 0xCBF29CE484222325
    for v in data:
        h = ((h ^ v) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
