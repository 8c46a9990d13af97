"""A float64 numpy restatement of the IMAGE COMPARE rule of include/vcloze_hip.h, written from the header text (not from
image_metrics.hip), and the error budget of the library's F32 arithmetic against it.  A helper, not a test.

The rule: two images of geometry C x H x W, 8-bit [H, W, C] (L = 255) or F32 [C, H, W] (L = 1).  sse = sum (a - b)^2, max_abs,
n_diff; psnr_db = 10 log10(L^2 n / sse), +inf at sse == 0; the mean over all VALID 11 x 11 windows (no padding) of
    ssim = ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2))
with the separable Gaussian window sigma = 1.5 whose eleven weights, exp(-(k - 5)^2 / 4.5) normalised in double, are rounded to
F32 once, and C1 = F32((0.01 L)^2), C2 = F32((0.03 L)^2).  The restatement uses those F32 VALUES (they are part of the rule) and
rounds nothing else.

THE BUDGET (u = 2^-24, the unit round-off of F32; first order, times 1 + 1e-3 for the products of two errors, which are below
100 u of the first-order terms).  The header's order of operations gives, per window:
  a value of plane p passes w[k] * p (1 rounding) and at most 10 additions in the horizontal pass, the same in the vertical pass:
  22 roundings, 23 with the product a * a, b * b or a * b in front:
      e(mu_a) = 22 u E|a|          e(e_aa) = 23 u E[a^2]          e(e_ab) = 23 u E|a b|          (E: the window's weighted mean)
  ma2 = mu_a * mu_a:  e = 2 |mu_a| e(mu_a) + u ma2;   mab = mu_a * mu_b:  e = |mu_a| e(mu_b) + |mu_b| e(mu_a) + u |mab|
  va = e_aa - ma2:    e = e(e_aa) + e(ma2) + u (|va| + e(e_aa) + e(ma2));   vb, cab likewise
  n1 = (mab + mab) + C1:  the doubling is exact;  e = 2 e(mab) + u |n1|;      n2 = (cab + cab) + C2:  e = 2 e(cab) + u |n2|
  d1 = (ma2 + mb2) + C1:  e = e(ma2) + e(mb2) + u (ma2 + mb2) + u |d1|;       d2 = (va + vb) + C2:  likewise
  num = n1 * n2:  e = |n2| e(n1) + |n1| e(n2) + u |num|;   den likewise;   ssim = num / den:  e = e(num) / |den| + |ssim| e(den) / |den| + u |ssim|
and for the mean: a thread adds its 4 windows (3 roundings: the first lands on 0), the tile's tree has 8 levels, the fold of the
tiles is in double (2^-53: nothing) and the mean is rounded to F32 once: 12 roundings on the path of a window,
      e(ssim_mean) = mean(e(ssim)) + 12 u mean|ssim|
The F32 sse: d = a - b (1 rounding), d * d (1; the square doubles d's), a thread adds at most 7 owned pixels (6 roundings), the
tree 8, the double fold none, the rounding to F32 one:  e(sse) = (3 + 6 + 8 + 1) u sse = 18 u sse.  max_abs: one subtraction, u max_abs."""
import numpy as np

U = 2.0 ** -24
TAPS = 11
TILE = 32
SECOND_ORDER = 1.0 + 1e-3


def weights() -> np.ndarray:
    """the eleven one-dimensional weights, float32"""
    k = np.arange(TAPS, dtype=np.float64) - 5.0
    g = np.exp(-(k * k) / 4.5)
    return (g / g.sum()).astype(np.float32)


def constants(L: float):
    return float(np.float32((0.01 * L) ** 2)), float(np.float32((0.03 * L) ** 2))


def to_chw(img) -> tuple:
    """(float64 [C, H, W], L) of a uint8 [H, W, C] or a float32 [C, H, W] array"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float64), 255.0
    assert img.dtype == np.float32, img.dtype
    return img.astype(np.float64), 1.0


def window_mean(p: np.ndarray) -> np.ndarray:
    """[C, H, W] -> [C, H - 10, W - 10]: the Gaussian window over the valid positions, horizontal pass first"""
    w = weights().astype(np.float64)
    Wv = p.shape[2] - (TAPS - 1)
    h = sum(w[k] * p[:, :, k:k + Wv] for k in range(TAPS))
    Hv = p.shape[1] - (TAPS - 1)
    return sum(w[j] * h[:, j:j + Hv, :] for j in range(TAPS))


def ssim_terms(a: np.ndarray, b: np.ndarray, L: float) -> dict:
    c1, c2 = constants(L)
    mu_a, mu_b = window_mean(a), window_mean(b)
    e_aa, e_bb, e_ab = window_mean(a * a), window_mean(b * b), window_mean(a * b)
    va, vb, cab = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    n1, n2 = 2.0 * mu_a * mu_b + c1, 2.0 * cab + c2
    d1, d2 = mu_a * mu_a + mu_b * mu_b + c1, va + vb + c2
    return dict(mu_a=mu_a, mu_b=mu_b, e_aa=e_aa, e_bb=e_bb, e_ab=e_ab, va=va, vb=vb, cab=cab, n1=n1, n2=n2, d1=d1, d2=d2,
                ssim=(n1 * n2) / (d1 * d2))


def ssim_budget(a: np.ndarray, b: np.ndarray, L: float, t: dict) -> float:
    """e(ssim_mean) of the module docstring, from the fp64 terms `t` of ssim_terms"""
    e_mua, e_mub = 22 * U * window_mean(np.abs(a)), 22 * U * window_mean(np.abs(b))
    e_eaa, e_ebb, e_eab = 23 * U * t["e_aa"], 23 * U * t["e_bb"], 23 * U * window_mean(np.abs(a * b))
    ma, mb = np.abs(t["mu_a"]), np.abs(t["mu_b"])
    ma2, mb2, mab = ma * ma, mb * mb, ma * mb
    e_ma2, e_mb2, e_mab = 2 * ma * e_mua + U * ma2, 2 * mb * e_mub + U * mb2, ma * e_mub + mb * e_mua + U * mab
    sub = lambda v, e1, e2: e1 + e2 + U * (np.abs(v) + e1 + e2)  # noqa: E731
    e_va, e_vb, e_cab = sub(t["va"], e_eaa, e_ma2), sub(t["vb"], e_ebb, e_mb2), sub(t["cab"], e_eab, e_mab)
    e_n1 = 2 * e_mab + U * np.abs(t["n1"])
    e_n2 = 2 * e_cab + U * np.abs(t["n2"])
    e_d1 = e_ma2 + e_mb2 + U * (ma2 + mb2) + U * np.abs(t["d1"])
    e_d2 = e_va + e_vb + U * np.abs(t["va"] + t["vb"]) + U * np.abs(t["d2"])
    num, den = t["n1"] * t["n2"], t["d1"] * t["d2"]
    e_num = np.abs(t["n2"]) * e_n1 + np.abs(t["n1"]) * e_n2 + U * np.abs(num)
    e_den = np.abs(t["d2"]) * e_d1 + np.abs(t["d1"]) * e_d2 + U * np.abs(den)
    s = np.abs(t["ssim"])
    e_ssim = e_num / np.abs(den) + s * e_den / np.abs(den) + U * s
    return float(SECOND_ORDER * (e_ssim.mean() + 12 * U * s.mean()))


def compare(a, b) -> dict:
    """the rule on two uint8 [H, W, C] or two float32 [C, H, W] arrays, in float64 (integers for the 8-bit form), with the budgets"""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.ndim == 3
    fa, L = to_chw(a)
    fb, _ = to_chw(b)
    C, H, W = fa.shape
    assert H >= TAPS and W >= TAPS
    if a.dtype == np.uint8:
        d = a.astype(np.int64) - b.astype(np.int64)
        sse, max_abs = int((d * d).sum()), int(np.abs(d).max())
    else:
        d = fa - fb
        sse, max_abs = float((d * d).sum()), float(np.abs(d).max())
    n = C * H * W
    t = ssim_terms(fa, fb, L)
    return {"n": n, "n_windows": C * (H - 10) * (W - 10), "sse": sse, "max_abs": max_abs, "n_diff": int((a != b).sum()),
            "mse": sse / n, "psnr_db": float("inf") if sse == 0 else 10.0 * np.log10(L * L * n / sse),
            "ssim": float(t["ssim"].mean()), "ssim_budget": ssim_budget(fa, fb, L, t),
            "sse_budget": 0.0 if a.dtype == np.uint8 else SECOND_ORDER * 18 * U * sse, "max_abs_budget": 0.0 if a.dtype == np.uint8 else U * max_abs}


def tiles(extent: int) -> int:
    return -(-(extent - 10) // TILE)


def scratch_bytes(C: int, H: int, W: int) -> int:
    """P * VC_IMG_RECORD_BYTES, P = C * TY * TX"""
    return C * tiles(H) * tiles(W) * 32
