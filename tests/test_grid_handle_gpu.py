"""The grid handle (vc_grid_*, csrc/grid_engine.hip) on the GPU: one grid and the SDEdit upsampling of its cells as ONE C call each.
It composes the entry points `pipeline.generate_grid` / `pipeline.upsample_images` compose, in their order, so every comparison
is BIT FOR BIT against those functions run with rng = NoiseStream(seed) and the three sub-handles on, and needs no tolerance.
Tiny models throughout (tests/helpers.tiny_model, the 8x autoencoder and the text configurations of tests/test_vae_handle_gpu.py /
tests/test_text_handle_gpu.py).  The grid: two rows of 32x64 and 32x48 pixels = latents 4x8 and 4x6, N = 8 + 6 tokens - the
smallest grid with unequal rows, where a wrong row offset, id axis or col0 shows.  SDEdit: K = 1 and 2 targets of 32x32 pixels."""
import ctypes as C

import pytest
import torch

from tests.procedural import TINY, TINY_T5, procedural_ae_param, procedural_text_param, ptensor, tiny_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1
SEED, STEPS, CFG = 11, 4, 30.0
ROWS = [(32, 64), (32, 48)]
AE = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 1, 1, 1], num_res_blocks=1, z_channels=16,
          scale_factor=0.3611, shift_factor=0.1159)                         # 8x down like the FLUX AE
CL = dict(vocab_size=128, hidden_size=TINY["vec_in_dim"], intermediate_size=128, num_hidden_layers=1,
          num_attention_heads=1, max_position_embeddings=16, layer_norm_eps=1e-5, eos_token_id=127)


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def mods(hip):
    """(model, ae, t5, clip) with all three use_handle switches on"""
    from tests.helpers import tiny_model
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m, _ = tiny_model()
    ae = AutoEncoder(AutoEncoderParams(**AE))
    ae.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in ae.state_dict().items()})
    ae = ae.to(DEV).to(torch.bfloat16)
    t5 = T5EncoderModel(T5Config(**TINY_T5))
    tsd = {k: procedural_text_param(k, v.shape) for k, v in t5.state_dict().items()}
    tsd["encoder.embed_tokens.weight"] = tsd["shared.weight"]
    t5.load_state_dict(tsd)
    t5 = t5.to(DEV).to(torch.bfloat16)
    clip = CLIPTextModel(CLIPTextConfig(**CL))
    clip.load_state_dict({k: procedural_text_param(k, v.shape) for k, v in clip.state_dict().items()})
    clip = clip.to(DEV).to(torch.bfloat16)
    ae.use_handle = t5.use_handle = clip.use_handle = True
    assert m.use_handle and m.handle() is not None
    return m, ae, t5, clip


@pytest.fixture(scope="module")
def data():
    c = lambda t: t.to(DEV, torch.bfloat16)  # noqa: E731
    rows = [c(ptensor((3, H, W), 301 + i, q=7)) for i, (H, W) in enumerate(ROWS)]
    masks = [c(torch.zeros(1, 1, *ROWS[0])),
             c(torch.cat((torch.zeros(1, 1, 32, 16), torch.ones(1, 1, 32, 16), torch.zeros(1, 1, 32, 16)), -1))]
    cells = [c(ptensor((3, 32, 32), 311 + i, q=7)) for i in range(2)]
    return dict(rows=rows, masks=masks, cells=cells, t5_ids=tiny_ids(64, 128, seed=5)[None].to(DEV),
                clip_ids=tiny_ids(16, 128, seed=6, eos=127, eos_at=7)[None].to(DEV))


@pytest.fixture(scope="module")
def gh(mods):
    from visualcloze_amd.handle import GridHandle
    return GridHandle(*mods)


@pytest.fixture(scope="module")
def ref(mods, data):
    """pipeline.generate_grid with a NoiseStream and the sub-handles on, per solver: computed once, never changed"""
    from visualcloze_amd import pipeline
    out = {}
    for solver in ("euler", "rk4"):
        rng = pipeline.NoiseStream(SEED, offset=5)
        imgs = pipeline.generate_grid(*mods, data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, cfg=CFG, steps=STEPS,
                                      solver=solver, rng=rng)
        torch.cuda.synchronize()
        out[solver] = (imgs, rng.offset)
    return out


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("solver", ["euler", "rk4"])
def test_generate_is_bit_identical_to_generate_grid(gh, data, ref, solver):
    want, want_off = ref[solver]
    got, off = gh.generate(data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, 5, cfg=CFG, steps=STEPS, solver=solver)
    torch.cuda.synchronize()
    assert off == want_off == 5 + 2 * 16 * 4 * (8 + 6)            # per row: the encode draw and the start noise, 16 x h x w each
    assert len(got) == 2
    for g, w, (H, W) in zip(got, want, ROWS):
        assert g.shape == (3, H, W) and torch.isfinite(g).all() and float(g.std()) > 0
        assert same(g, w)
    assert not torch.equal(ref["euler"][0][1], ref["rk4"][0][1])


def test_decode_row_subset_both_output_forms_and_a_second_call(gh, mods, data, ref):
    from visualcloze_amd import pipeline
    want = ref["euler"][0]
    args = (data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, 5)
    got, _ = gh.generate(*args, cfg=CFG, steps=STEPS, decode_rows=[1])
    assert len(got) == 1 and same(got[0], want[1])
    u8, _ = gh.generate(*args, cfg=CFG, steps=STEPS, uint8=True)
    torch.cuda.synchronize()
    for g, w in zip(u8, want):
        pil = pipeline.to_uint8_image(w)                            # the reference's quantisation of that row
        assert g.dtype == torch.uint8 and g.shape == (pil.height, pil.width, 3)
        assert torch.equal(g.cpu(), torch.from_numpy(__import__("numpy").asarray(pil).copy()))
    # same geometry again: the sub-handles' plan caches serve, nothing is captured, the bits repeat
    counts = (gh.vae.plan_count(), gh.t5.plan_count(), gh.clip.plan_count())
    again, off = gh.generate(*args, cfg=CFG, steps=STEPS)
    torch.cuda.synchronize()
    assert (gh.vae.plan_count(), gh.t5.plan_count(), gh.clip.plan_count()) == counts and counts[0] >= 4 and counts[1] >= 1 and counts[2] >= 1
    assert off == ref["euler"][1] and all(same(a, b) for a, b in zip(again, want))
    # another seed / offset is another image
    other, _ = gh.generate(*args[:4], SEED + 1, 5, cfg=CFG, steps=STEPS)
    assert not torch.equal(other[1], want[1])


@pytest.mark.parametrize("K", [1, 2])
def test_sdedit_is_bit_identical_to_upsample_images(gh, mods, data, K):
    """the pipeline's own path from its encodes onward: its inputs are 8-bit images at the target size, so its resize is a no-op, and
    the handle is fed exactly the pixels it normalises them to"""
    from visualcloze_amd import pipeline
    imgs01 = [((c.float() + 1) / 2).clamp(0, 1) for c in data["cells"][:K]]
    pils = [pipeline.to_uint8_image(i) for i in imgs01]
    rng = pipeline.NoiseStream(SEED, offset=3)
    want = pipeline.upsample_images(*mods, pils, (32, 32), data["t5_ids"], data["clip_ids"], rng, cfg=CFG, steps=3, strength=0.4, solver="euler")
    torch.cuda.synchronize()
    import numpy as np
    px = [((torch.from_numpy(np.asarray(p, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5).to(DEV, torch.bfloat16) for p in pils]
    got, off = gh.sdedit(px, data["t5_ids"], data["clip_ids"], SEED, 3, cfg=CFG, steps=3, strength=0.4)
    torch.cuda.synchronize()
    assert off == rng.offset == 3 + K * 3 * 16 * 4 * 4              # per target: encode(image), encode(blank), start noise
    assert len(got) == len(want) == K
    for g, w in zip(got, want):
        assert g.shape == (3, 32, 32) and float(g.std()) > 0 and same(g, w)
    if K == 2:
        assert not torch.equal(got[0], got[1])
        # the opt-in switch of the pipeline function is the same call
        rng2 = pipeline.NoiseStream(SEED, offset=3)
        on = pipeline.upsample_images(*mods, pils, (32, 32), data["t5_ids"], data["clip_ids"], rng2, cfg=CFG, steps=3, strength=0.4,
                                      use_grid_handle=True)
        assert rng2.offset == off and all(same(a, b) for a, b in zip(on, want))


def test_sdedit_strength_one_returns_the_converted_input(gh, hip, data):
    px = data["cells"][:2]
    got, off = gh.sdedit(px, data["t5_ids"], data["clip_ids"], SEED, 9, steps=3, strength=1.0)
    u8, _ = gh.sdedit(px, data["t5_ids"], data["clip_ids"], SEED, 9, steps=3, strength=1.0, uint8=True)
    torch.cuda.synchronize()
    assert off == 9                                                  # nothing is drawn
    for g, u, p in zip(got, u8, px):
        want = ((p.float() + 1.0) / 2.0).clamp_(0.0, 1.0)
        assert same(g, want) and torch.equal(u, want.mul(255).to(torch.uint8).permute(1, 2, 0).contiguous())


def test_generate_and_upsample_switch_gives_the_same_bits(mods, data):
    """both stages chained: a two-cell last row, one masked cell, target_size = the cell's size (the host resize is the identity)"""
    from visualcloze_amd import pipeline
    rows = [data["rows"][1][:, :, :32].contiguous(), data["rows"][0]]                    # rows of 32x32 and 32x64: the last has two 32x32 cells
    masks = [torch.zeros(1, 1, 32, 32, device=DEV, dtype=torch.bfloat16),
             torch.cat((torch.zeros(1, 1, 32, 32), torch.ones(1, 1, 32, 32)), -1).to(DEV, torch.bfloat16)]
    outs = {}
    for on in (False, True):
        rng = pipeline.NoiseStream(SEED)
        outs[on] = (pipeline.generate_and_upsample(*mods, rows, masks, data["t5_ids"], data["clip_ids"], SEED, grid_w=2, mask_position=[False, True],
                                                   target_size=(32, 32), cfg=CFG, steps=STEPS, upsampling_steps=3, rng=rng, use_grid_handle=on),
                     rng.offset)
        torch.cuda.synchronize()
    assert outs[True][1] == outs[False][1] and len(outs[True][0]) == len(outs[False][0]) == 1
    assert outs[True][0][0].shape == (3, 32, 32) and same(outs[True][0][0], outs[False][0][0]) and float(outs[True][0][0].std()) > 0
    # the switch needs every sub-handle on
    mods[1].use_handle = False
    try:
        with pytest.raises(ValueError, match="use_handle"):
            pipeline.generate_grid(*mods, rows, masks, data["t5_ids"], data["clip_ids"], SEED, rng=pipeline.NoiseStream(1), use_grid_handle=True)
    finally:
        mods[1].use_handle = True


def test_argument_errors_come_back_with_a_message_and_the_handle_still_serves(hip, gh, data, ref):
    L = hip.lib()
    px = [r.contiguous() for r in data["rows"]]
    ms = [m.reshape(m.shape[-2:]).contiguous() for m in data["masks"]]
    import numpy as np
    t5a = np.ascontiguousarray(data["t5_ids"][0].cpu().numpy().astype(np.int32))
    cla = np.ascontiguousarray(data["clip_ids"][0].cpu().numpy().astype(np.int32))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    outs = [torch.full((3, H, W), 7.0, device=DEV) for H, W in ROWS]

    def job(**kw):
        j = hip.GridJob()
        j.rows = 2
        for i, (H, W) in enumerate(ROWS):
            j.height[i], j.width[i], j.pixels[i], j.masks[i], j.decode[i] = H, W, px[i].data_ptr(), ms[i].data_ptr(), 1
        j.t5_ids, j.clip_ids, j.t5_len, j.clip_len = ip(t5a), ip(cla), 64, 16
        j.seed, j.noise_offset, j.guidance, j.n_points, j.method, j.out_form, j.time_shifting_factor = SEED, 5, CFG, STEPS, 0, 0, 1.0
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(j, k)[v[0]] = v[1]
            else:
                setattr(j, k, v)
        return j

    good = job()
    need = C.c_int64(0)
    assert L.vc_grid_workspace_bytes(gh.h, C.byref(good), C.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    ptrs = (C.c_void_p * 2)(*[o.data_ptr() for o in outs])
    st = torch.cuda.Stream()
    s = st.cuda_stream
    torch.cuda.synchronize()
    run = lambda j, h=gh.h, w=base, n=need.value, p=ptrs: L.vc_grid_generate(h, None if j is None else C.byref(j), w, n, p, s)  # noqa: E731
    cases = [(job(width=(1, 40)), b"multiples of 16"), (job(height=(0, 24)), b"multiples of 16"), (job(rows=0), b"rows"),
             (job(rows=17), b"rows"), (job(n_points=1), b"n_points"), (job(method=7), b"method"), (job(out_form=5), b"out_form"),
             (job(n_points=6, max_evals=4), b"max_evals"), (job(method=2, max_evals=4), b"max_evals"),
             (job(pixels=(1, None)), b"null pixels"), (job(masks=(0, None)), b"null mask"), (job(t5_ids=None), b"null"),
             (job(t5_len=60), b"multiple of 64"), (job(noise_offset=2 ** 64 - 8), b"64-bit stream")]
    for j, word in cases:
        assert run(j) == ERR_ARG and word in L.vc_last_error(), (word, L.vc_last_error())
    assert run(None) == ERR_ARG and run(good, h=None) == ERR_ARG and b"null handle" in L.vc_last_error()
    assert run(good, p=None) == ERR_ARG and run(good, w=None) == ERR_ARG and run(good, w=base + 16) == ERR_ARG
    assert run(good, n=need.value - 1) == ERR_ARG and b"too small" in L.vc_last_error()
    assert L.vc_grid_workspace_bytes(gh.h, C.byref(job(rows=0)), C.byref(need)) == ERR_ARG
    sd = hip.GridSdedit()
    assert L.vc_grid_sdedit_workspace_bytes(gh.h, C.byref(sd), C.byref(need)) == ERR_ARG and b"count" in L.vc_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)                 # nothing was launched
    # ... and the handle still generates the reference bits, through the same raw call
    after = C.c_uint64(0)
    good.noise_offset_out = C.pointer(after)
    assert run(good) == 0, L.vc_last_error()
    st.synchronize()
    gh.vae._prepared = gh.t5._prepared = gh.clip._prepared = None     # the raw call prepared the sub-handles in `ws`
    gh.flux.geom = None
    assert after.value == ref["euler"][1] and all(same(o, w) for o, w in zip(outs, ref["euler"][0]))
