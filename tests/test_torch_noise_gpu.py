"""GPU: the torch noise stream (include/vcloze_hip.h, THE TORCH STREAM; csrc/rng_torch.hip) against torch itself.  torch.randn with a
seeded device generator is the arbiter: every comparison with it is BIT FOR BIT on integer views, 0 differing elements allowed.

  1. hip.randn_torch (F32, bf16) == torch.randn(n, generator=G) (.to(bfloat16)); a sequence of draws follows G.get_offset()
  2. the layout alone: VC_RNG_U32 words & 0x7fffffff == torch.empty(n, int32).random_(generator=G).  random_ of a 32-bit integer type
     (DistributionTemplates.h, random_kernel: distribution_nullary_kernel<scalar_t, uint32_t, uint4> over hiprand4, then
     uniform_int = word % 2^31) takes ONE word per element through the same grid-stride kernel as normal_ does, so it shows the
     (thread, lane, round) -> element map without the transform
  3. explicit sm_count / threads_per_sm: the device's own give the same bits as 0 / 0; a smaller cap gives the words of a numpy
     restatement of the contract built on tests/noise_ref.py's Philox constants
  4. vc_randn_torch_tokens == the bf16 draw + vc_pack_latent
  5. pipeline.generate_grid(seed=s) == generate_grid(rng=TorchNoiseStream(s)) and the same for upsample_images
  6. use_grid_handle=True with a TorchNoiseStream == without the handle; noise_offset_out == the stream's offset
  7. tests/c_abi/torch_noise_demo.c == the ctypes calls

Sizes: 1, 3, 4, 5 (inside one Philox block's worth of threads), 1023 / 1024 / 1025 (around four blocks of 256 threads), 221184 (the
start state of a 1024 x 3456 grid), 256 cap and 256 cap + 1 (either side of the device's grid cap: from there on a thread owns more
than one lane) and 4 * 256 cap + 1 (a second round of the grid-stride loop), cap from the device's properties."""
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import noise_ref as R
from tests.test_grid_handle_gpu import AE, CFG, CL, DEV, ROWS, STEPS, data, hip, mods, same  # noqa: F401  (fixtures of the tiny grid)

pytestmark = pytest.mark.gpu
SEEDS = [0, 1, (1 << 32) + 5, (1 << 63) + 1]
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 221184, "cap", "cap+1", "4cap+1"]


@pytest.fixture(scope="module")
def caps(hip):
    p = torch.cuda.get_device_properties(torch.device(DEV))
    return p.multi_processor_count, p.max_threads_per_multi_processor


def size_of(n, caps) -> int:
    cap = caps[0] * (caps[1] // 256)
    return {"cap": 256 * cap, "cap+1": 256 * cap + 1, "4cap+1": 4 * 256 * cap + 1}.get(n, n)


def gen(seed: int, offset: int = 0) -> torch.Generator:
    g = torch.Generator(DEV).manual_seed(seed)
    if offset:
        g.set_offset(offset)
    return g


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def differing(a: torch.Tensor, b: torch.Tensor) -> int:
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((bits(a) != bits(b)).sum())


# ---------------------------------------------------------------- 1. bit-equality with torch
@pytest.mark.parametrize("n", SIZES)
def test_f32_and_bf16_draws_are_torchs_bit_for_bit(hip, caps, n):
    n = size_of(n, caps)
    for seed in SEEDS:
        want = torch.randn(n, device=DEV, generator=gen(seed))
        got = hip.randn_torch([n], seed, 0, dtype=torch.float32, device=DEV)
        got16 = hip.randn_torch([n], seed, 0, dtype=torch.bfloat16, device=DEV)
        d32, d16 = differing(got, want), differing(got16, want.to(torch.bfloat16))
        print(f"n {n} seed {seed:#x}: {d32} differing f32 elements, {d16} differing bf16 elements")
        assert d32 == 0 and d16 == 0


def test_a_nonzero_offset_and_an_unaligned_base(hip):
    """the generator's offset enters the counter; a base that is not 16-byte aligned takes the element-wise stores"""
    for seed, off, n in ((7, 4, 1000), (7, (1 << 34) - 4, 1029), (9, 12, 221184)):
        want = torch.randn(n, device=DEV, generator=gen(seed, off))
        assert differing(hip.randn_torch([n], seed, off, dtype=torch.float32, device=DEV), want) == 0
        buf = torch.zeros(n + 3, device=DEV)
        hip.randn_torch(None, seed, off, out=buf[1:n + 1])
        assert differing(buf[1:n + 1], want) == 0 and float(buf[0]) == 0 and float(buf[n + 1]) == 0 and float(buf[n + 2]) == 0
        b16 = torch.zeros(n + 3, device=DEV, dtype=torch.bfloat16)
        hip.randn_torch(None, seed, off, out=b16[1:n + 1])
        assert differing(b16[1:n + 1], want.to(torch.bfloat16)) == 0 and float(b16[0]) == 0 and float(b16[n + 1]) == 0


def test_a_sequence_of_draws_follows_the_generators_offset(hip, caps):
    from visualcloze_amd import pipeline
    G = gen(1234)
    s = pipeline.TorchNoiseStream(1234, device=DEV)
    shapes = [(1, 16, 6, 10), (3, 5), (1, 16, 48, 144), (size_of("4cap+1", caps) + 7,)]
    for shape, dtype in zip(shapes, (torch.bfloat16, torch.float32, torch.bfloat16, torch.float32)):
        want = torch.randn(shape, device=DEV, generator=G).to(dtype)
        got = s.randn(shape, dtype)
        assert got.dtype == dtype and differing(got, want) == 0
        assert s.offset == G.get_offset()
    assert s.offset == 4 + 4 + 4 + 8                    # the last draw takes a second round of the grid-stride loop


# ---------------------------------------------------------------- 2. the layout alone
@pytest.mark.parametrize("n", SIZES)
def test_raw_words_are_the_words_torchs_random_takes(hip, caps, n):
    n = size_of(n, caps)
    for seed in SEEDS:
        G = gen(seed)
        want = torch.empty(n, dtype=torch.int32, device=DEV).random_(generator=G)
        got = hip.randn_torch([n], seed, 0, dtype=torch.int32, device=DEV)
        assert int(((got & 0x7fffffff) != want).sum()) == 0
        assert G.get_offset() == hip.torch_randn_policy(n)[1]


# ---------------------------------------------------------------- 3. explicit caps
def words_np(seed: int, offset: int, n: int, T: int) -> np.ndarray:
    """the contract restated: element i is word lane of the block with counter (c, thread), c = offset / 4 + round"""
    i = np.arange(n, dtype=np.uint64)
    thread, q = i % np.uint64(T), i // np.uint64(T)
    lane, c = (q & np.uint64(3)).astype(np.int64), np.uint64(offset // 4) + (q >> np.uint64(2))
    m32, s32 = np.uint64(R.MASK32), np.uint64(32)
    c0, c1, c2, c3 = c & m32, c >> s32, thread & m32, thread >> s32
    k0, k1 = seed & R.MASK32, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(R.M0) * c0, np.uint64(R.M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + R.W0) & R.MASK32, (k1 + R.W1) & R.MASK32
    x = np.stack([c0, c1, c2, c3], axis=1)
    return x[np.arange(n), lane].astype(np.uint32)


def test_the_restatement_is_noise_refs_philox():
    for seed, off, n, T in ((5, 8, 9, 256), ((1 << 63) + 1, (1 << 34) - 4, 2100, 512)):
        w = words_np(seed, off, n, T)
        for i in (0, 1, n // 2, n - 1):
            thread, q = i % T, i // T
            c = off // 4 + q // 4
            blk = R.philox4x32_10((c & R.MASK32, c >> 32, thread & R.MASK32, thread >> 32), (seed & R.MASK32, seed >> 32))
            assert int(w[i]) == blk[q % 4]


def u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def test_explicit_caps(hip, caps):
    seed, off, n = (1 << 32) + 5, 16, 2500
    dflt = hip.randn_torch([n], seed, off, dtype=torch.int32, device=DEV)
    own = hip.randn_torch([n], seed, off, dtype=torch.int32, device=DEV, sm_count=caps[0], threads_per_sm=caps[1])
    assert torch.equal(dflt, own)
    assert differing(hip.randn_torch([n], seed, off, dtype=torch.float32, device=DEV),
                     hip.randn_torch([n], seed, off, dtype=torch.float32, device=DEV, sm_count=caps[0], threads_per_sm=caps[1])) == 0
    assert hip.torch_randn_policy(n) == hip.torch_randn_policy(n, *caps) == (10, 4)
    # n = 2500 on this device: ten blocks, T = 2560, every element lane 0 of its own thread
    assert np.array_equal(u32(dflt), words_np(seed, off, n, 2560))
    # a device of one multiprocessor and 256 threads: T = 256, three rounds - the same words only where thread, lane and round agree
    small = hip.randn_torch([n], seed, off, dtype=torch.int32, device=DEV, sm_count=1, threads_per_sm=256)
    assert hip.torch_randn_policy(n, 1, 256) == (1, 12)
    assert np.array_equal(u32(small), words_np(seed, off, n, 256))
    assert torch.equal(small[:256], dflt[:256]) and int((small[256:] == dflt[256:]).sum()) == 0
    # 511 threads per multiprocessor still make one block of 256; two multiprocessors two
    assert torch.equal(hip.randn_torch([n], seed, off, dtype=torch.int32, device=DEV, sm_count=1, threads_per_sm=511), small)
    two = hip.randn_torch([n], seed, off, dtype=torch.int32, device=DEV, sm_count=2, threads_per_sm=256)
    assert np.array_equal(u32(two), words_np(seed, off, n, 512))
    # the normals follow the same map: element i of the small device is a lane the default draw never computes, except the first 256
    f_small = hip.randn_torch([n], seed, off, dtype=torch.float32, device=DEV, sm_count=1, threads_per_sm=256)
    f_dflt = hip.randn_torch([n], seed, off, dtype=torch.float32, device=DEV)
    assert differing(f_small[:256], f_dflt[:256]) == 0 and differing(f_small, f_dflt) > 2000


# ---------------------------------------------------------------- 4. the tokens form
@pytest.mark.parametrize("shape", [(16, 6, 10), (16, 48, 144)])
def test_tokens_form_is_the_draw_packed(hip, shape):
    Cz, h, w = shape
    seed, off = (1 << 63) + 1, 8
    for kw in (dict(), dict(sm_count=1, threads_per_sm=256)):          # the second: every lane and several rounds
        lat = hip.randn_torch([Cz, h, w], seed, off, dtype=torch.bfloat16, device=DEV, **kw)
        want = torch.zeros((h // 2) * (w // 2), 4 * Cz + 64, dtype=torch.bfloat16, device=DEV)
        hip.pack_latent(lat, want, col0=32)
        got = torch.zeros_like(want)
        hip.randn_torch_tokens(Cz, h, w, seed, off, tokens=got, col0=32, **kw)
        assert differing(got, want) == 0 and float(got[:, 32:32 + 4 * Cz].float().std()) > 0.5
    want_t = torch.randn(shape, device=DEV, generator=gen(seed, off)).to(torch.bfloat16)
    assert differing(hip.randn_torch([Cz, h, w], seed, off, dtype=torch.bfloat16, device=DEV), want_t) == 0


# ---------------------------------------------------------------- 5. the pipeline: seed= and TorchNoiseStream are one path
SEED = 11


@pytest.fixture(scope="module")
def enc_noise():
    """the encoder's DiagonalGaussian draws, supplied: the reference takes them from torch's GLOBAL generator, which no seed fixes"""
    g = torch.Generator(DEV).manual_seed(99)
    return [torch.randn(1, 16, H // 8, W // 8, device=DEV, generator=g).to(torch.bfloat16) for H, W in ROWS]


@pytest.fixture(scope="module")
def by_seed(mods, data, enc_noise):
    from visualcloze_amd import pipeline
    out = pipeline.generate_grid(*mods, data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, cfg=CFG, steps=STEPS,
                                 encode_noise=enc_noise)
    torch.cuda.synchronize()
    return out


def test_generate_grid_by_seed_equals_generate_grid_by_torch_noise_stream(mods, data, enc_noise, by_seed):
    from visualcloze_amd import pipeline
    rng = pipeline.TorchNoiseStream(SEED, device=DEV)
    got = pipeline.generate_grid(*mods, data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], 12345, cfg=CFG, steps=STEPS,
                                 encode_noise=enc_noise, rng=rng)
    torch.cuda.synchronize()
    assert len(got) == len(by_seed) == 2 and all(same(a, b) and float(a.std()) > 0 for a, b in zip(got, by_seed))
    assert rng.offset == 8                               # two start-noise draws, one round each; the encoder draws were supplied
    own = pipeline.generate_grid(*mods, data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, cfg=CFG, steps=STEPS,
                                 encode_noise=enc_noise, rng=pipeline.NoiseStream(SEED))
    assert not torch.equal(own[1], by_seed[1])           # the library's own stream is another one


def _pils(data, K):
    from visualcloze_amd import pipeline
    return [pipeline.to_uint8_image(((c.float() + 1) / 2).clamp(0, 1)) for c in data["cells"][:K]]


def test_upsample_images_by_generator_equals_by_torch_noise_stream(mods, data):
    from visualcloze_amd import pipeline
    pils = _pils(data, 2)
    g = torch.Generator(DEV).manual_seed(98)
    en = [tuple(torch.randn(16, 4, 4, device=DEV, generator=g).to(torch.bfloat16) for _ in range(2)) for _ in range(2)]
    G = gen(SEED, 8)                                     # where the generator stands behind the grid stage above
    want = pipeline.upsample_images(*mods, pils, (32, 32), data["t5_ids"], data["clip_ids"], G, cfg=CFG, steps=3, strength=0.4, encode_noise=en)
    rng = pipeline.TorchNoiseStream(SEED, device=DEV, offset=8)
    got = pipeline.upsample_images(*mods, pils, (32, 32), data["t5_ids"], data["clip_ids"], rng, cfg=CFG, steps=3, strength=0.4, encode_noise=en)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2 and all(same(a, b) and float(a.std()) > 0 for a, b in zip(got, want))
    assert rng.offset == G.get_offset() == 16


# ---------------------------------------------------------------- 6. the grid handle
def test_grid_handle_with_the_torch_stream_is_bit_identical_to_the_pipeline(mods, data):
    """every draw from the stream - the encoder's included, in NoiseStream's order - with and without the handle"""
    from visualcloze_amd import pipeline
    from visualcloze_amd.handle import GridHandle
    args = (data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED)
    off, on = pipeline.TorchNoiseStream(SEED, device=DEV, offset=4), pipeline.TorchNoiseStream(SEED, device=DEV, offset=4)
    want = pipeline.generate_grid(*mods, *args, cfg=CFG, steps=STEPS, rng=off)
    got = pipeline.generate_grid(*mods, *args, cfg=CFG, steps=STEPS, rng=on, use_grid_handle=True)
    torch.cuda.synchronize()
    assert all(same(a, b) and float(a.std()) > 0 for a, b in zip(got, want)) and len(got) == 2
    assert on.offset == off.offset == 4 + 4 * 4          # per row the encode draw and the start noise, one round each
    # the handle itself: noise_offset_out is the stream's offset; back on the library's own stream it is NoiseStream's twin again
    gh = GridHandle(*mods)
    gh.set_noise("torch")
    direct, after = gh.generate(*args[:4], SEED, 4, cfg=CFG, steps=STEPS)
    assert after == off.offset and all(same(a, b) for a, b in zip(direct, want))
    with pytest.raises(Exception, match="multiple of 4"):
        gh.generate(*args[:4], SEED, 6, cfg=CFG, steps=STEPS)
    gh.set_noise("own")
    own = pipeline.NoiseStream(SEED, offset=5)
    want_own = pipeline.generate_grid(*mods, *args, cfg=CFG, steps=STEPS, rng=own)
    direct_own, after_own = gh.generate(*args[:4], SEED, 5, cfg=CFG, steps=STEPS)
    assert after_own == own.offset and all(same(a, b) for a, b in zip(direct_own, want_own))
    assert not torch.equal(direct_own[1], direct[1])


def test_grid_handle_sdedit_with_the_torch_stream(mods, data):
    from visualcloze_amd import pipeline
    pils = _pils(data, 2)
    off, on = pipeline.TorchNoiseStream(SEED, device=DEV, offset=16), pipeline.TorchNoiseStream(SEED, device=DEV, offset=16)
    kw = dict(cfg=CFG, steps=3, strength=0.4)
    want = pipeline.upsample_images(*mods, pils, (32, 32), data["t5_ids"], data["clip_ids"], off, **kw)
    got = pipeline.upsample_images(*mods, pils, (32, 32), data["t5_ids"], data["clip_ids"], on, use_grid_handle=True, **kw)
    torch.cuda.synchronize()
    assert len(got) == 2 and all(same(a, b) and float(a.std()) > 0 for a, b in zip(got, want))
    assert on.offset == off.offset == 16 + 2 * 3 * 4     # per target: encode(image), encode(blank), the start noise
    # and those draws are torch's: one target by a torch generator that stands behind the two encoder draws, which are supplied
    s = pipeline.TorchNoiseStream(SEED, device=DEV, offset=16)
    en = [(s.randn([16, 4, 4]), s.randn([16, 4, 4]))]
    by_gen = pipeline.upsample_images(*mods, pils[:1], (32, 32), data["t5_ids"], data["clip_ids"], gen(SEED, s.offset), encode_noise=en, **kw)
    by_handle = pipeline.upsample_images(*mods, pils[:1], (32, 32), data["t5_ids"], data["clip_ids"],
                                         pipeline.TorchNoiseStream(SEED, device=DEV, offset=16), use_grid_handle=True, **kw)
    assert same(by_gen[0], by_handle[0])


def test_sde_refuses_the_torch_stream(mods, data):
    from visualcloze_amd import pipeline
    with pytest.raises(ValueError, match="TorchNoiseStream"):
        pipeline.generate_grid(*mods, data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, cfg=CFG, steps=STEPS,
                               rng=pipeline.TorchNoiseStream(SEED, device=DEV), sde=dict(diffusion_form="linear"))


# ---------------------------------------------------------------- 7. the C demo
@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_demo_prints_the_words_of_the_ctypes_calls(hip, tmp_path):
    from tests.torch_noise_demo_build import build_torch_noise_demo
    exe = build_torch_noise_demo(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seed, off0, n1, n2 = 0x8000000000000001, 8, 13, 1030                       # the #defines of torch_noise_demo.c
    (g1, a1), (g2, a2) = hip.torch_randn_policy(n1), hip.torch_randn_policy(n2)
    w = hip.randn_torch([n1], seed, off0, dtype=torch.int32, device=DEV)
    f = hip.randn_torch([n1], seed, off0, dtype=torch.float32, device=DEV)
    b = hip.randn_torch([n2], seed, off0 + a1, dtype=torch.bfloat16, device=DEV)
    hexs = lambda a, k: " ".join(f"{int(v):0{k}x}" for v in a)  # noqa: E731
    want = [f"policy {n1} {g1} {a1}", f"policy {n2} {g2} {a2}", "u32 " + hexs(u32(w), 8), "f32 " + hexs(f.cpu().numpy().view(np.uint32), 8),
            "bf16 " + hexs(b.cpu().view(torch.int16).numpy().view(np.uint16), 4), f"offset {off0 + a1 + a2}"]
    assert r.stdout.strip().splitlines() == want
    assert (g1, a1, g2, a2) == (1, 4, 5, 4)
    # and those are torch's own numbers
    G = gen(seed, off0)
    assert differing(f, torch.randn(n1, device=DEV, generator=G)) == 0
    assert differing(b, torch.randn(n2, device=DEV, generator=G).to(torch.bfloat16)) == 0 and G.get_offset() == off0 + a1 + a2
