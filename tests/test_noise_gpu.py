"""-m gpu: the library's noise source (csrc/rng.hip: vc_randn, vc_randn_tokens) against the host restatement of its contract
(tests/noise_ref.py, written from the text of include/vcloze_hip.h) and `pipeline.NoiseStream` through `generate_grid`.

Exact where the contract is exact - the raw Philox words, the independence of a draw from its split into calls, from the base
address and from the layout written - and within the per-element budget of tests/test_noise_cpu.py (its docstring has the
derivation; nothing in it was fitted to a device) where f32 arithmetic comes in:
    bf16   |got - ref64| <= HALF * ulp_bf16(STORE) + (1/64) * ulp_bf16(r)
    f32    |got - ref64| <= (1/64) * ulp_bf16(r)
Shapes are the smallest at which the kernel takes each of its paths: a head before the first 16-byte boundary, 16-byte chunks, a
tail, the element-wise form for a phase that allows no chunks, more than one workgroup, and one draw just above a full pass of
the capped grid (the grid-stride loop)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import noise_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
DEV = "cuda:0"
GUARD = 16
SENTINEL = {torch.int32: 0x5A5A5A5A, torch.float32: 1.5, torch.bfloat16: 1.5}


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip
    hip.require_gpu()
    return hip


def guarded(hip, n, seed, offset, dtype, shift=0):
    """a draw of n elements into a buffer whose base lies `shift` elements behind a 256-byte boundary, with GUARD sentinel
    elements either side that must come back untouched"""
    buf = torch.full((shift + 2 * GUARD + n,), SENTINEL[dtype], dtype=dtype, device=DEV)
    assert buf.data_ptr() % 256 == 0
    out = buf[shift + GUARD: shift + GUARD + n]
    hip.randn(None, seed, offset, out=out)
    torch.cuda.synchronize()
    buf = buf.cpu()
    side = torch.cat((buf[:shift + GUARD], buf[shift + GUARD + n:]))
    assert bool((side == SENTINEL[dtype]).all()), f"wrote outside its {n} elements (shift {shift}, offset {offset})"
    return buf[shift + GUARD: shift + GUARD + n].clone()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def ref_words(seed, offset, n):
    return torch.from_numpy(R.words(seed, offset, n).view(np.int32).copy())


def test_u32_words_equal_the_restatement_bit_for_bit(hip):
    seed = 0xC0FFEE1234567
    for n in (1, 3, 4, 5, 7, 8, 9, 255, 2049):
        for offset in (0, 1, 2, 3, 5, (1 << 32) - 2, (1 << 34) + 1):
            got = guarded(hip, n, seed, offset, torch.int32)
            assert torch.equal(got, ref_words(seed, offset, n)), (n, offset)
    # the counter's carry into its second word happens at position 2^34: a draw across it, both phases
    for offset in ((1 << 34) - 8, (1 << 34) - 5):
        assert torch.equal(guarded(hip, 21, seed, offset, torch.int32), ref_words(seed, offset, 21)), offset
    # the last positions of the stream
    assert torch.equal(guarded(hip, 8, seed, (1 << 64) - 8, torch.int32), ref_words(seed, (1 << 64) - 8, 8))


def test_u32_one_draw_just_above_a_full_grid_pass(hip):
    n = hip.RNG_MAX_BLOCKS * 256 * 4 + 5             # every thread stores one 16-byte chunk, the first few a second work item
    for seed, offset in ((77, 0), ((1 << 63) + 9, 6)):        # 16-byte chunks; the element-wise form (phase 2)
        got = hip.randn([n], seed, offset, dtype=torch.int32, device=DEV).cpu()
        assert torch.equal(got, ref_words(seed, offset, n)), (seed, offset)


@pytest.mark.parametrize("dtype", [torch.int32, torch.float32, torch.bfloat16])
def test_any_base_aligned_to_the_element_gives_the_same_values(hip, dtype):
    seed = 991
    for n, offset in ((1, 0), (7, 0), (8, 3), (29, 0), (29, 1), (77, 6), (600, 0)):
        want = guarded(hip, n, seed, offset, dtype, 0)
        if dtype == torch.int32:
            assert torch.equal(want, ref_words(seed, offset, n))
        for shift in range(1, 8):
            assert torch.equal(bits(guarded(hip, n, seed, offset, dtype, shift)), bits(want)), (n, offset, shift)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_draw_does_not_depend_on_its_split_into_calls(hip, dtype):
    seed = (1 << 40) + 12345
    for offset in (0, 3, (1 << 34) - 1001):
        whole = hip.randn([4099], seed, offset, dtype=dtype, device=DEV)
        parts, at = [], offset
        for n in (1, 2, 1000, 3096):
            parts.append(hip.randn([n], seed, at, dtype=dtype, device=DEV))
            at += n
        assert at == offset + 4099
        assert torch.equal(bits(torch.cat(parts)), bits(whole)), offset       # f32 compared as its bit pattern


@pytest.mark.parametrize("seed", [1234, (1 << 32) + 0xABCDEF])
def test_normals_within_the_budget_on_every_element(hip, seed):
    n = 1 << 16
    z, r = R.normals64(seed, 0, n)
    got32 = hip.randn([n], seed, 0, dtype=torch.float32, device=DEV).cpu()
    got16 = hip.randn([n], seed, 0, dtype=torch.bfloat16, device=DEV).cpu()
    wf, wb = R.worst(got32, z, R.budget_f32(z, r)), R.worst(got16, z, R.budget_bf16(z, r))
    print(f"seed {seed}: worst |err| / budget over {n} elements: f32 {wf:.4f}, bf16 {wb:.4f}")
    assert wf <= 1.0, wf
    assert wb <= 1.0, wb
    # the bf16 draw is the f32 draw rounded to nearest even, as torch.randn(...).to(bf16) rounds
    assert torch.equal(bits(got32.to(torch.bfloat16)), bits(got16))
    # ... and the element-wise form (phase 1) computes the very same values
    odd = hip.randn([n - 1], seed, 1, dtype=torch.float32, device=DEV).cpu()
    assert torch.equal(bits(odd), bits(got32[1:]))


@pytest.mark.parametrize("C_, h, w, ld, col0", [(16, 2, 2, 64, 0), (16, 6, 10, 128, 64), (16, 48, 72, 64, 0)])
def test_tokens_form_equals_randn_then_pack_latent(hip, C_, h, w, ld, col0):
    seed = 0x5EED00000001
    rows = (h // 2) * (w // 2)
    for offset in (5, 7, (1 << 33) + 2, 4096):                  # pairs that straddle two blocks (odd), and that do not
        latent = hip.randn([C_, h, w], seed, offset, dtype=torch.bfloat16, device=DEV)
        want = torch.full((rows, ld), 1.5, dtype=torch.bfloat16, device=DEV)
        hip.pack_latent(latent, want, col0)
        got = torch.full((rows, ld), 1.5, dtype=torch.bfloat16, device=DEV)
        hip.randn_tokens(C_, h, w, seed, offset, tokens=got, col0=col0)
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(want)), offset      # the columns outside col0 .. col0 + 4C included: untouched
        # element (c, y, x) sits at stream position offset + (c*h + y)*w + x
        c, y, x = C_ - 1, h - 1, w - 2
        z, _ = R.normals64(seed, offset + (c * h + y) * w + x, 2)
        tok = (y // 2) * (w // 2) + x // 2
        pair = got[tok, col0 + c * 4 + (y & 1) * 2: col0 + c * 4 + (y & 1) * 2 + 2].float().cpu().numpy()
        assert np.abs(pair - z).max() < 2.0 ** -5             # half a bf16 ulp below 8
    new = hip.randn_tokens(C_, h, w, seed, 5, device=DEV)
    assert new.shape == (rows, 4 * C_)


def test_a_replayed_graph_repeats_its_noise(hip):
    """seed and offset are kernel arguments by value: the call is legal under stream capture and every replay draws the same"""
    st = torch.cuda.Stream()
    out = torch.zeros(1000, dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()
    with hip.Graph(st.cuda_stream) as g:
        hip.randn(None, 42, 10, out=out, stream=st.cuda_stream)
    want = hip.randn([1000], 42, 10, device=DEV)
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.launch()
        st.synchronize()
        assert torch.equal(bits(out), bits(want))


# ---------------------------------------------------------------- pipeline.NoiseStream through generate_grid
@pytest.fixture(scope="module")
def tiny_pipeline():
    from tests.helpers import tiny_model
    from tests.procedural import TINY, TINY_T5, procedural_ae_param, procedural_text_param, ptensor, tiny_ids
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m, _ = tiny_model()
    AE = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 1, 1, 1], num_res_blocks=1, z_channels=16,
              scale_factor=0.3611, shift_factor=0.1159)
    CL = dict(vocab_size=128, hidden_size=TINY["vec_in_dim"], intermediate_size=128, num_hidden_layers=1,
              num_attention_heads=1, max_position_embeddings=16, layer_norm_eps=1e-5, eos_token_id=127)
    ae = AutoEncoder(AutoEncoderParams(**AE)); ae.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in ae.state_dict().items()})
    ae = ae.to(DEV).to(torch.bfloat16)
    t5 = T5EncoderModel(T5Config(**TINY_T5)); tsd = {k: procedural_text_param(k, v.shape) for k, v in t5.state_dict().items()}
    tsd["encoder.embed_tokens.weight"] = tsd["shared.weight"]
    t5.load_state_dict(tsd); t5 = t5.to(DEV).to(torch.bfloat16)
    clip = CLIPTextModel(CLIPTextConfig(**CL)); clip.load_state_dict({k: procedural_text_param(k, v.shape) for k, v in clip.state_dict().items()})
    clip = clip.to(DEV).to(torch.bfloat16)
    H, W = 32, 64
    c = lambda t: t.to(DEV, torch.bfloat16)  # noqa: E731
    rows = [c(ptensor((3, H, W), 201 + i, q=7)) for i in range(2)]
    masks = [c(torch.zeros(1, 1, H, W)), c(torch.cat((torch.zeros(1, 1, H, W // 2), torch.ones(1, 1, H, W // 2)), -1))]
    t5_ids, clip_ids = tiny_ids(64, 128, seed=5)[None].to(DEV), tiny_ids(16, 128, seed=6, eos=127, eos_at=7)[None].to(DEV)
    return (m, ae, t5, clip, rows, masks, t5_ids, clip_ids), (H, W)


def test_noise_stream_through_generate_grid(hip, tiny_pipeline, monkeypatch):
    from visualcloze_amd import pipeline
    args, (H, W) = tiny_pipeline
    ae, rows = args[1], args[4]
    seen = []
    inner = pipeline.denoise_grid

    def spy(model, noise_rows, cond_latent_rows, *a, **k):
        seen.append(([t.clone() for t in noise_rows], [t.clone() for t in cond_latent_rows]))
        return inner(model, noise_rows, cond_latent_rows, *a, **k)
    monkeypatch.setattr(pipeline, "denoise_grid", spy)

    def run(seed):
        s = pipeline.NoiseStream(seed)
        out = pipeline.generate_grid(*args, seed=0, cfg=30.0, steps=2, decode_rows=[1], rng=s)[0]
        torch.cuda.synchronize()
        return out, s
    a, sa = run(11)
    b, _ = run(11)
    c, _ = run(12)
    n = 16 * (H // 8) * (W // 8)
    assert sa.offset == 4 * n                                  # two encode draws, two start-noise draws
    assert a.shape == (3, H, W) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)                                   # equal seeds: bit-equal
    assert not torch.equal(a, c)                               # another seed: another image
    # what the sampler saw is hip.randn at the documented offsets, in the reference's order of draws: the DiagonalGaussian draw
    # of each row's encode (visualcloze.py:377), then one start-noise tensor per row (:395-399)
    noise_rows, lat_rows = seen[0]
    for i in range(2):
        enc = hip.randn([1, 16, H // 8, W // 8], 11, i * n, device=DEV)
        assert torch.equal(lat_rows[i], ae.encode(rows[i][None], noise=enc))
        assert torch.equal(bits(noise_rows[i]), bits(hip.randn([1, 16, H // 8, W // 8], 11, (2 + i) * n, device=DEV)))
    assert not torch.equal(seen[0][0][0], seen[2][0][0])
    # an explicit encode_noise keeps those draws off the stream; a torch.Generator or None leaves the path as it was
    s = pipeline.NoiseStream(11)
    enoise = [hip.randn([1, 16, H // 8, W // 8], 11, i * n, device=DEV) for i in range(2)]
    pipeline.generate_grid(*args, seed=0, cfg=30.0, steps=2, decode_rows=[1], rng=s, encode_noise=enoise)
    assert s.offset == 2 * n
    assert torch.equal(bits(seen[-1][0][0]), bits(hip.randn([1, 16, H // 8, W // 8], 11, 0, device=DEV)))
    g1 = pipeline.generate_grid(*args, seed=3, cfg=30.0, steps=2, decode_rows=[1], encode_noise=enoise)[0]
    g2 = pipeline.generate_grid(*args, seed=3, cfg=30.0, steps=2, decode_rows=[1], encode_noise=enoise,
                                rng=torch.Generator(device=DEV).manual_seed(3))[0]
    assert torch.equal(g1, g2)
    want = torch.randn([1, 16, H // 8, W // 8], device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(torch.bfloat16)
    assert torch.equal(bits(seen[-1][0][0]), bits(want))


# ---------------------------------------------------------------- the C99 caller
def build_demo(out_dir) -> str:
    from visualcloze_amd import hip
    exe = os.path.join(str(out_dir), "noise_demo")
    libdir = os.path.dirname(hip.LIB_PATH)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(ROCM, "include"),
           os.path.join(REPO, "tests", "c_abi", "noise_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip", "-L" + os.path.join(ROCM, "lib"),
           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_host_program_draws_the_same_noise_as_the_ctypes_calls(hip, tmp_path):
    exe = build_demo(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.strip().splitlines())
    seed, offset0, Z, H, W, LD, COL0 = 0x0123456789ABCDEF, (1 << 34) - 5, 16, 6, 10, 128, 64       # the #defines of noise_demo.c
    n = Z * H * W
    noise = hip.randn([Z, H, W], seed, offset0, device=DEV)
    tokens = torch.zeros((H // 2) * (W // 2), LD, dtype=torch.bfloat16, device=DEV)
    hip.randn_tokens(Z, H, W, seed, offset0 + n, tokens=tokens, col0=COL0)
    torch.cuda.synchronize()
    raw = lambda t: t.cpu().contiguous().view(torch.int16).numpy().tobytes()  # noqa: E731
    assert got == {"encode_noise": "%016x" % R.fnv64(raw(noise)), "tokens": "%016x" % R.fnv64(raw(tokens))}
    assert got["encode_noise"] != got["tokens"]
