"""The autoencoder handle (vc_vae_*, csrc/vae_engine.hip) on the GPU: one C call per decode / encode, one hipGraph launch once
captured.  It issues the kernels `vae.AutoEncoder`'s Python-ordered plan issues, in the same order, so every comparison below is
BIT FOR BIT against that plan - which tests/test_vae_gpu.py holds to the reference's golden vectors - and needs no tolerance.
Tiny autoencoder of tests/golden/vae_golden.npz (tests/procedural.py::TINY_AE, procedural weights), two image sizes: a square
one (4x4 latent, 16 attention tokens) and a non-square one (6x10 latent: height and width differ, neither divides the other, and
its 60 attention tokens exercise the zero pads of the attention operands)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests.procedural import TINY_AE, procedural_ae_param, ptensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SIZES = {"sq": (4, 4), "rect": (6, 10)}          # latent (h, w); the image is 2x (TINY_AE has two levels)
F = 2 ** (len(TINY_AE["ch_mult"]) - 1)
Z = TINY_AE["z_channels"]
ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def ae(hip):
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m = AutoEncoder(AutoEncoderParams(**TINY_AE))
    m.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in m.state_dict().items()})
    return m.to(DEV).to(torch.bfloat16)


@pytest.fixture(scope="module")
def ref(ae):
    """inputs and the Python-ordered plan's results per size, computed once"""
    out = {}
    for i, (name, (h, w)) in enumerate(SIZES.items()):
        z = ptensor((1, Z, h, w), 71 + i, q=5, kmax=96).to(DEV, torch.bfloat16)
        img = ptensor((1, 3, F * h, F * w), 75 + i, q=7, kmax=127).to(DEV, torch.bfloat16)
        noise = ptensor((1, Z, h, w), 79 + i, q=5, kmax=80).to(DEV, torch.bfloat16)
        out[name] = dict(z=z, img=img, noise=noise, decode=ae.decode(z)[0], encode=ae.encode(img, noise=noise)[0],
                         mean=ae.encode(img, sample=False)[0])
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def handle(ae):
    from visualcloze_amd.handle import VaeHandle
    return VaeHandle(ae)


@pytest.mark.parametrize("name", list(SIZES))
def test_decode_is_bit_identical_to_the_python_ordered_plan(ae, handle, ref, name):
    r = ref[name]
    got = handle.decode(r["z"][0])
    torch.cuda.synchronize()
    assert got.shape == r["decode"].shape and torch.isfinite(got.float()).all() and float(got.float().abs().max()) > 0
    assert torch.equal(got, r["decode"])
    # an f32 latent (z / scale + shift is then rounded once, not twice: vc_nchw_to_nhwc) and f32 pixels: the Python-ordered plan on
    # the same f32 latent, widened
    got32 = handle.decode(r["z"][0].float(), pixels_f32=True)
    assert got32.dtype == torch.float32 and torch.equal(got32, ae.decode(r["z"].float())[0].float())


@pytest.mark.parametrize("name", list(SIZES))
def test_encode_with_noise_and_with_null_noise_is_bit_identical(handle, ref, name):
    r = ref[name]
    got = handle.encode(r["img"][0], noise=r["noise"][0])
    mean = handle.encode(r["img"][0], noise=None)
    torch.cuda.synchronize()
    assert torch.equal(got, r["encode"]) and torch.equal(mean, r["mean"])
    assert not torch.equal(got, mean)
    assert torch.equal(handle.encode(r["img"][0].float(), noise=r["noise"][0]), r["encode"])      # f32 pixels round to the same bf16


@pytest.mark.parametrize("name", list(SIZES))
def test_token_forms_equal_pack_and_unpack_around_the_nchw_forms(hip, handle, ref, name):
    r = ref[name]
    h, w = SIZES[name]
    col0, ld = 8, 40                               # 4 * Z = 16 token columns at a non-zero offset inside wider rows
    rows = (h // 2) * (w // 2)
    tokens = ptensor((rows, ld), 91, q=5).to(DEV, torch.bfloat16)
    hip.pack_latent(r["z"][0].contiguous(), tokens, col0=col0)
    got = handle.decode_tokens(tokens, h, w, col0=col0)
    assert torch.equal(got, r["decode"])
    # encode into tokens: the packed latent in columns col0 .. col0 + 16, the other columns untouched
    frame = ptensor((rows, ld), 92, q=5).to(DEV, torch.bfloat16)
    want = frame.clone()
    hip.pack_latent(r["encode"].contiguous(), want, col0=col0)
    got_t = handle.encode(r["img"][0], noise=r["noise"][0], tokens=frame, col0=col0)
    torch.cuda.synchronize()
    assert torch.equal(got_t, want) and not torch.equal(got_t, frame)
    back = torch.empty(Z, h, w, dtype=torch.bfloat16, device=DEV)
    hip.unpack_latent(got_t, back, col0=col0)
    assert torch.equal(back, r["encode"])


def test_plans_are_kept_per_size_and_reused(ae, ref):
    from visualcloze_amd.handle import VaeHandle
    hd = VaeHandle(ae)
    assert hd.plan_count() == 0
    a1 = hd.decode(ref["sq"]["z"][0])
    assert hd.plan_count() == 1
    b = hd.decode(ref["rect"]["z"][0])
    a2 = hd.decode(ref["sq"]["z"][0])
    torch.cuda.synchronize()
    assert hd.plan_count() == 2
    assert torch.equal(a1, a2) and torch.equal(a1, ref["sq"]["decode"]) and torch.equal(b, ref["rect"]["decode"])
    # another latent through the kept plan: the graph reads its argument, not a recording of it
    z2 = ptensor((Z, 4, 4), 97, q=5, kmax=96).to(DEV, torch.bfloat16)
    assert torch.equal(hd.decode(z2), ae.decode(z2[None])[0]) and hd.plan_count() == 2
    # the same for the encoder: capture on one image, replay on another
    img, noise = ref["sq"]["img"], ref["sq"]["noise"]
    assert torch.equal(hd.encode(img[0], noise=noise[0]), ref["sq"]["encode"]) and hd.plan_count() == 3
    img2 = ptensor((1, 3, 8, 8), 98, q=7, kmax=127).to(DEV, torch.bfloat16)
    assert torch.equal(hd.encode(img2[0], noise=noise[0]), ae.encode(img2, noise=noise)[0]) and hd.plan_count() == 3


def test_one_workspace_prepared_again_with_other_halves_gets_plans_of_its_own(hip, ae, ref):
    """The carve-up of a workspace depends on `which` (the decoder's buffers start it when prepared alone and follow the encoder's
    otherwise): a plan captured under one carve-up must not serve another.  One max-sized workspace, fixed argument buffers, one
    stream - what a C caller does."""
    from visualcloze_amd.handle import VaeHandle
    L = hip.lib()
    hd = VaeHandle(ae)
    r = ref["sq"]
    need = hd.workspace_bytes(8, 8, hip.VAE_ENCODER | hip.VAE_DECODER)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    z, img, noise = r["z"][0].clone(), r["img"][0].contiguous(), r["noise"][0].contiguous()      # z is rewritten below: a copy
    px = torch.empty(3, 8, 8, dtype=torch.bfloat16, device=DEV)
    lat = torch.empty(Z, 4, 4, dtype=torch.bfloat16, device=DEV)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    torch.cuda.synchronize()

    def decode():
        px.fill_(float("nan"))
        torch.cuda.synchronize()
        hip._check(L.vc_vae_decode(hd.h, z.data_ptr(), 0, 0, 0, px.data_ptr(), 0, s), "vc_vae_decode")
        st.synchronize()
        return px.clone()

    hip._check(L.vc_vae_prepare(hd.h, 8, 8, hip.VAE_DECODER, base, need, s), "prepare")
    assert torch.equal(decode(), r["decode"]) and hd.plan_count() == 1
    hip._check(L.vc_vae_prepare(hd.h, 8, 8, hip.VAE_ENCODER | hip.VAE_DECODER, base, need, s), "prepare")
    hip._check(L.vc_vae_encode(hd.h, img.data_ptr(), 0, noise.data_ptr(), lat.data_ptr(), 0, 0, 0, s), "vc_vae_encode")
    st.synchronize()
    assert torch.equal(lat, r["encode"]) and hd.plan_count() == 2
    assert torch.equal(decode(), r["decode"]) and hd.plan_count() == 3          # same pointers, another carve-up: a plan of its own
    z.copy_(ptensor((Z, 4, 4), 97, q=5, kmax=96))                              # ... that reads its argument
    want2 = ae.decode(z[None])[0]
    assert torch.equal(decode(), want2) and hd.plan_count() == 3
    hip._check(L.vc_vae_prepare(hd.h, 8, 8, hip.VAE_DECODER, base, need, s), "prepare")
    assert torch.equal(decode(), want2) and hd.plan_count() == 3                # back: the first plan serves again


def test_the_ninth_plan_evicts_the_least_recently_used_one(hip, ae, ref):
    """The list of captured plans holds 8, most recently used first (include/vcloze_hip.h).  One handle, one prepared workspace, one
    stream, the same latent into nine output tensors: nine keys.  The ninth evicts the first, which is then captured again."""
    from visualcloze_amd.handle import VaeHandle
    L = hip.lib()
    hd = VaeHandle(ae)
    r = ref["sq"]
    need = hd.workspace_bytes(8, 8, hip.VAE_DECODER)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    z = r["z"][0].contiguous()
    pxs = [torch.full((3, 8, 8), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(9)]
    st = torch.cuda.Stream()
    s = st.cuda_stream
    torch.cuda.synchronize()
    hip._check(L.vc_vae_prepare(hd.h, 8, 8, hip.VAE_DECODER, base, need, s), "vc_vae_prepare")

    def decode(px):
        hip._check(L.vc_vae_decode(hd.h, z.data_ptr(), 0, 0, 0, px.data_ptr(), 0, s), "vc_vae_decode")
        return hd.plan_count()

    assert [decode(px) for px in pxs] == [1, 2, 3, 4, 5, 6, 7, 8, 8]
    st.synchronize()
    for px in pxs:
        assert torch.equal(px, r["decode"])
    pxs[0].fill_(float("nan"))
    torch.cuda.synchronize()
    assert decode(pxs[0]) == 8                           # its plan was the least recently used one: evicted, captured again
    st.synchronize()
    assert torch.equal(pxs[0], r["decode"])


def test_a_stream_that_is_not_the_current_one_is_ordered(handle, ref):
    r = ref["rect"]
    st = torch.cuda.Stream()
    z = r["z"][0] * 1.0                                   # produced on the current stream just before the call
    got = handle.decode(z, stream=st.cuda_stream)         # ... which runs on `st` and hands back on the current stream
    assert torch.equal(got, r["decode"])
    enc = handle.encode(r["img"][0] * 1.0, noise=r["noise"][0], stream=st.cuda_stream)
    assert torch.equal(enc, r["encode"])


@pytest.mark.parametrize("name", list(SIZES))
def test_null_stream_runs_the_same_plan_uncaptured(handle, ref, name):
    r = ref[name]
    torch.cuda.synchronize()
    n = handle.plan_count()
    got = handle.decode(r["z"][0], stream=None)
    enc = handle.encode(r["img"][0], noise=r["noise"][0], stream=None)
    torch.cuda.synchronize()
    assert handle.plan_count() == n
    assert torch.equal(got, r["decode"]) and torch.equal(enc, r["encode"])


def test_errors_are_reported_before_anything_is_launched(hip, ae, ref):
    from visualcloze_amd.handle import VaeHandle
    L = hip.lib()
    st = hip.cur_stream()
    z = ref["sq"]["z"][0].contiguous()
    px = torch.full((3, 8, 8), float("nan"), dtype=torch.bfloat16, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(px.float()).all())

    hd = VaeHandle(ae)                                              # every weight bound, nothing prepared
    # decode before prepare
    assert L.vc_vae_decode(hd.h, z.data_ptr(), 0, 0, 0, px.data_ptr(), 0, st) == ERR_STATE
    assert b"vc_vae_prepare" in L.vc_last_error() and untouched()
    # a workspace that is too small
    need = hd.workspace_bytes(8, 8)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    assert L.vc_vae_prepare(hd.h, 8, 8, 3, base, need - 1, st) == ERR_ARG and b"too small" in L.vc_last_error()
    assert L.vc_vae_decode(hd.h, z.data_ptr(), 0, 0, 0, px.data_ptr(), 0, st) == ERR_STATE and untouched()
    # prepared for the decoder only: encode is refused, decode runs
    assert L.vc_vae_prepare(hd.h, 8, 8, hip.VAE_DECODER, base, need, st) == 0, L.vc_last_error()
    img = ref["sq"]["img"][0].contiguous()
    lat = torch.full((Z, 4, 4), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert L.vc_vae_encode(hd.h, img.data_ptr(), 0, None, lat.data_ptr(), 0, 0, 0, st) == ERR_STATE and L.vc_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(lat.float()).all())
    # bad forms / token geometry
    assert L.vc_vae_decode(hd.h, z.data_ptr(), 7, 0, 0, px.data_ptr(), 0, st) == ERR_ARG and L.vc_last_error()
    assert L.vc_vae_decode(hd.h, z.data_ptr(), hip.VAE_TOKENS, 36, 8, px.data_ptr(), 0, st) == ERR_ARG and L.vc_last_error()
    assert L.vc_vae_decode(hd.h, None, 0, 0, 0, px.data_ptr(), 0, st) == ERR_ARG and untouched() and hd.plan_count() == 0
    # unknown name, wrong shape
    w = ae.decoder.conv_in.weight
    shape = (C.c_int64 * 4)(*w.shape)
    assert L.vc_vae_bind_weight(hd.h, b"decoder.conv_inn", w.data_ptr(), ae.decoder.conv_in.bias.data_ptr(), 0, shape, 4, st) == ERR_ARG
    assert b"decoder.conv_inn" in L.vc_last_error()
    bad = (C.c_int64 * 4)(w.shape[0], w.shape[1] + 1, 3, 3)
    assert L.vc_vae_bind_weight(hd.h, b"decoder.conv_in", w.data_ptr(), ae.decoder.conv_in.bias.data_ptr(), 0, bad, 4, st) == ERR_ARG
    assert b"decoder.conv_in" in L.vc_last_error()
    # ... and the handle still decodes
    assert L.vc_vae_decode(hd.h, z.data_ptr(), 0, 0, 0, px.data_ptr(), 0, st) == 0, L.vc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(px, ref["sq"]["decode"])

    # decode before bind: a fresh handle with the decoder's first weight missing
    h2 = C.c_void_p()
    assert L.vc_vae_create(C.byref(hd.cfg), C.byref(h2)) == 0
    try:
        px.fill_(float("nan"))
        assert L.vc_vae_prepare(h2, 8, 8, 3, base, need, st) == 0
        assert L.vc_vae_decode(h2, z.data_ptr(), 0, 0, 0, px.data_ptr(), 0, st) == ERR_STATE
        assert b"decoder.conv_in.weight" in L.vc_last_error() and untouched()
        assert L.vc_vae_encode(h2, img.data_ptr(), 0, None, lat.data_ptr(), 0, 0, 0, st) == ERR_STATE
        assert b"encoder.conv_in.weight" in L.vc_last_error() and L.vc_vae_plan_count(h2) == 0
    finally:
        L.vc_vae_destroy(h2)


def write_demo_input(path, hd, ae, z):
    sd = ae.state_dict()
    bits = lambda t: t.detach().to(torch.bfloat16).contiguous().view(torch.int16).cpu().numpy().tobytes()  # noqa: E731
    names = hd.weight_names()
    with open(path, "wb") as f:
        f.write(bytes(hd.cfg))
        f.write(struct.pack("<3i", len(names), z.shape[-2], z.shape[-1]))
        for n in names:
            w, b = sd[n + ".weight"], sd[n + ".bias"]
            f.write(struct.pack("<i", len(n)) + n.encode() + struct.pack("<i", w.dim()) + struct.pack(f"<{w.dim()}q", *w.shape))
            f.write(bits(w))
            f.write(bits(b))
        f.write(bits(z))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_host_program_decodes_and_encodes_bit_identically(hip, ae, handle, ref, tmp_path):
    """tests/c_abi/vae_handle_demo.c: plain C99, no Python in the process - binds the state dict as stored, decodes, encodes."""
    exe = str(tmp_path / "vae_handle_demo")
    libdir = os.path.dirname(hip.LIB_PATH)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(ROCM, "include"),
           os.path.join(REPO, "tests", "c_abi", "vae_handle_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip", "-L" + os.path.join(ROCM, "lib"),
           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    z = ref["rect"]["z"][0]
    write_demo_input(tmp_path / "in.bin", handle, ae, z)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = torch.from_numpy(np.fromfile(tmp_path / "out.bin", dtype=np.int16)).view(torch.bfloat16)
    want_px = ref["rect"]["decode"]
    assert got.numel() == want_px.numel() + z.numel()
    assert torch.equal(got[:want_px.numel()].reshape(want_px.shape), want_px.cpu())
    want_lat = ae.encode(want_px[None], sample=False)[0]
    assert torch.equal(got[want_px.numel():].reshape(z.shape), want_lat.cpu())


def test_opt_in_switch_leaves_generate_grid_unchanged(hip):
    """AutoEncoder.use_handle routes encode / decode of the whole pixel-to-pixel path through the handle: the same pixels."""
    from tests.helpers import tiny_model
    from tests.procedural import TINY, TINY_T5, procedural_text_param, tiny_ids
    from visualcloze_amd import pipeline
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m, _ = tiny_model()
    dev = "cuda"
    AE = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 1, 1, 1], num_res_blocks=1, z_channels=16,
              scale_factor=0.3611, shift_factor=0.1159)                         # 8x down like the FLUX AE
    CL = dict(vocab_size=128, hidden_size=TINY["vec_in_dim"], intermediate_size=128, num_hidden_layers=1,
              num_attention_heads=1, max_position_embeddings=16, layer_norm_eps=1e-5, eos_token_id=127)
    ae = AutoEncoder(AutoEncoderParams(**AE))
    ae.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in ae.state_dict().items()})
    ae = ae.to(dev).to(torch.bfloat16)
    t5 = T5EncoderModel(T5Config(**TINY_T5))
    tsd = {k: procedural_text_param(k, v.shape) for k, v in t5.state_dict().items()}
    tsd["encoder.embed_tokens.weight"] = tsd["shared.weight"]
    t5.load_state_dict(tsd)
    t5 = t5.to(dev).to(torch.bfloat16)
    clip = CLIPTextModel(CLIPTextConfig(**CL))
    clip.load_state_dict({k: procedural_text_param(k, v.shape) for k, v in clip.state_dict().items()})
    clip = clip.to(dev).to(torch.bfloat16)
    H, W = 32, 64
    c = lambda t: t.to(dev, torch.bfloat16)  # noqa: E731
    rows = [c(ptensor((3, H, W), 201 + i, q=7)) for i in range(2)]
    masks = [c(torch.zeros(1, 1, H, W)), c(torch.cat((torch.zeros(1, 1, H, W // 2), torch.ones(1, 1, H, W // 2)), -1))]
    enoise = [c(ptensor((1, 16, H // 8, W // 8), 211 + i, q=5)) for i in range(2)]
    t5_ids, clip_ids = tiny_ids(64, 128, seed=5)[None].to(dev), tiny_ids(16, 128, seed=6, eos=127, eos_at=7)[None].to(dev)

    def run():
        out = pipeline.generate_grid(m, ae, t5, clip, rows, masks, t5_ids, clip_ids, seed=3, cfg=30.0, steps=4, encode_noise=enoise)
        torch.cuda.synchronize()
        return out
    assert ae.use_handle is False
    off = run()
    ae.use_handle = True
    on = run()
    assert ae.handle().plan_count() == 2                            # one encode and one decode plan serve both rows
    assert len(on) == len(off) == 2
    for a, b in zip(on, off):
        assert a.shape == (3, H, W) and torch.equal(a, b)
    assert float(off[1].std()) > 0
