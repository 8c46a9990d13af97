"""The text-encoder handle (vc_text_*, csrc/text_engine.hip) on the GPU: one C call per batch of prompts, one hipGraph launch per
prompt once captured.  It issues the kernels `text.T5EncoderModel` / `text.CLIPTextModel`'s Python-ordered plan issues, with the same
problem structs in the same order, so every comparison against that plan below is BIT FOR BIT and needs no tolerance; the three glue
kernels that replace torch spellings (vc_t5_position_bias, vc_clip_embed, vc_clip_pool) are pure gathers / one rounded sum and are
held to those torch spellings bit for bit too.  The golden cases go through the handle against the bounds tests/test_text_gpu.py
applies to the Python-ordered plan (copied from there)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests.procedural import TINY_CLIP, TINY_T5, procedural_text_param, ptensor, tiny_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
G = np.load(os.path.join(REPO, "tests", "golden", "text_golden.npz"))
ERR_ARG, ERR_STATE = -1, -3
T5_XXL_1 = dict(vocab_size=512, d_model=4096, d_kv=64, d_ff=10240, num_layers=1, num_heads=64,
                relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
CLIP_L_1 = dict(vocab_size=512, hidden_size=768, intermediate_size=3072, num_hidden_layers=1, num_attention_heads=12,
                max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=511)


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


def bf(t):
    return t.to(torch.bfloat16).to(DEV)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def make_t5(cfg):
    from visualcloze_amd.text import T5Config, T5EncoderModel
    m = T5EncoderModel(T5Config(**cfg))
    sd = {k: procedural_text_param(k, v.shape) for k, v in m.state_dict().items()}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    m.load_state_dict(sd)
    return m.to(DEV).to(torch.bfloat16), sd


def make_clip(cfg):
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel
    m = CLIPTextModel(CLIPTextConfig(**cfg))
    sd = {k: procedural_text_param(k, v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    return m.to(DEV).to(torch.bfloat16), sd


@pytest.fixture(scope="module")
def t5(hip):
    return make_t5(TINY_T5)


@pytest.fixture(scope="module")
def clip(hip):
    return make_clip(TINY_CLIP)


def clip_ids(L, seed, eos_at):
    return tiny_ids(L, TINY_CLIP["vocab_size"], seed=seed, eos=TINY_CLIP["eos_token_id"], eos_at=eos_at)


@pytest.fixture(scope="module")
def ref(t5, clip):
    """ids and the Python-ordered plan's results (use_handle False), computed once and left unchanged"""
    out = {}
    for L in (64, 128):
        ids = torch.stack([tiny_ids(L, TINY_T5["vocab_size"], seed=31 + i) for i in range(3)]).to(DEV)
        out["t5", L] = dict(ids=ids, hidden=t5[0](ids).clone())
    for L, at in ((24, 9), (7, 6)):
        ids = torch.stack([clip_ids(L, 41 + i, at - i) for i in range(3)]).to(DEV)
        pooled, hs = clip[0](ids)
        out["clip", L] = dict(ids=ids, hidden=hs.clone(), pooled=pooled.clone())
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def t5_handle(t5):
    from visualcloze_amd.handle import TextHandle
    return TextHandle(t5[0])


@pytest.fixture(scope="module")
def clip_handle(clip):
    from visualcloze_amd.handle import TextHandle
    return TextHandle(clip[0])


# ---------------------------------------------------------------------------------------------------- the three glue kernels
@pytest.mark.parametrize("L,H", [(64, 2), (192, 64), (512, 2)])
def test_position_bias_is_the_torch_gather(hip, L, H):
    """192 is the smallest multiple of 64 beyond max_distance = 128: the saturated bucket is exercised; every table entry is distinct,
    so a wrong bucket or a wrong head cannot hide"""
    from visualcloze_amd.text import t5_relative_buckets
    nb, md = 32, 128
    tab = (torch.arange(nb * H, dtype=torch.int16) + 0x3000).view(torch.bfloat16).reshape(nb, H)      # consecutive bf16 bit patterns
    assert tab.float().unique().numel() == nb * H and torch.isfinite(tab.float()).all()
    tab = tab.to(DEV)
    got = hip.t5_position_bias(tab, L, md)
    want = tab[t5_relative_buckets(L, nb, md).to(DEV)].permute(2, 0, 1).contiguous().view(H * L, L)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("L,Lp,D", [(24, 64, 128), (7, 64, 128), (77, 128, 768)])
def test_clip_embed_is_the_four_step_torch_spelling(hip, L, Lp, D):
    V = 96
    tok, pos = bf(ptensor((V, D), 11, q=6, kmax=96)), bf(ptensor((77, D), 12, q=6, kmax=96))
    ids = tiny_ids(L, V, seed=13).to(DEV, torch.int32)
    # text.py's spelling: embedding of zero-padded ids, a zeroed position buffer with its first L rows copied in, the sum
    idp = torch.zeros(Lp, dtype=torch.int32, device=DEV)
    idp[:L] = ids
    want = torch.empty(Lp, D, dtype=torch.bfloat16, device=DEV)
    hip.embedding(idp, tok, want)
    p = torch.full((Lp, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    p.zero_()
    p[:L] = pos[:L]
    hip.add(want, p, want)
    got = torch.full((Lp, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.clip_embed(ids, tok, pos, got)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got[L:], tok[0].expand(Lp - L, D))
    assert torch.equal(got[:L], tok[ids.long()] + pos[:L])


@pytest.mark.parametrize("case", ["first", "last", "twice", "absent"])
def test_clip_pool_takes_the_first_eos_row(hip, case):
    L, D, eos = 77, 768, 511
    hidden = bf(ptensor((128, D), 14, q=5))
    ids = tiny_ids(L, eos, seed=15)
    where = {"first": [0], "last": [L - 1], "twice": [20, 33], "absent": []}[case]
    for i in where:
        ids[i] = eos
    want_row = where[0] if where else 0
    assert int((ids == eos).int().argmax()) == want_row                     # CLIPTextTransformer.forward's index
    got = hip.clip_pool(ids.to(DEV, torch.int32), hidden, eos)
    torch.cuda.synchronize()
    assert torch.equal(got, hidden[want_row])


# ---------------------------------------------------------------------------------------------------- tiny models through the handle
def test_tiny_t5_two_lengths_through_one_handle(t5, ref):
    from visualcloze_amd.handle import TextHandle
    hd = TextHandle(t5[0])
    assert hd.plan_count() == 0
    for n, L in enumerate((64, 128), 1):
        r = ref["t5", L]
        got, pooled = hd.encode(r["ids"][:1])
        torch.cuda.synchronize()
        assert pooled is None and hd.plan_count() == n
        assert torch.isfinite(got.float()).all() and float(got.float().abs().max()) > 0
        assert torch.equal(got, r["hidden"][:1])
        # another prompt through the kept plan: the graph reads the resident ids, not a recording of them
        got2, _ = hd.encode(r["ids"][1:2])
        assert torch.equal(got2, r["hidden"][1:2]) and not torch.equal(got2, got) and hd.plan_count() == n
    got, _ = hd.encode(ref["t5", 64]["ids"][:1])                            # back to the first length: its plan serves again
    assert torch.equal(got, ref["t5", 64]["hidden"][:1]) and hd.plan_count() == 2


@pytest.mark.parametrize("L", [24, 7])
def test_tiny_clip_hidden_and_pooled_are_bit_identical(clip_handle, ref, L):
    r = ref["clip", L]
    hs, pooled = clip_handle.encode(r["ids"][:1])
    torch.cuda.synchronize()
    assert hs.shape == (1, L, TINY_CLIP["hidden_size"]) and float(hs.float().abs().max()) > 0
    assert torch.equal(hs, r["hidden"][:1]) and torch.equal(pooled, r["pooled"][:1])
    hs2, pooled2 = clip_handle.encode(r["ids"][1:2])
    assert torch.equal(hs2, r["hidden"][1:2]) and torch.equal(pooled2, r["pooled"][1:2]) and not torch.equal(pooled2, pooled)
    only_pooled = clip_handle.encode(r["ids"][:1], want_hidden=False)
    assert only_pooled[0] is None and torch.equal(only_pooled[1], r["pooled"][:1])


@pytest.mark.parametrize("name", ["t5_a", "t5_b"])
def test_t5_golden_cases_through_the_handle(t5, t5_handle, name):
    """the bounds of tests/test_text_gpu.py::test_tiny_t5_matches_transformers_golden_and_oracle"""
    from oracle import text_oracle as TO
    ids = torch.tensor(G[name + "_ids"])
    out = t5_handle.encode(ids[None].to(DEV))[0][0].float().cpu()
    ref32 = torch.tensor(G[name + "_fp32"])
    o16 = TO.t5_encode(t5[1], ids, TINY_T5, "bf16")
    noise = rel_l2(o16, ref32)
    assert rel_l2(out, ref32) <= 3.0 * noise + 2e-3, (rel_l2(out, ref32), noise)
    assert rel_l2(out, o16) <= 2.0 * noise + 2e-3, (rel_l2(out, o16), noise)
    assert torch.equal(out, t5_handle.encode(ids[None].to(DEV))[0][0].float().cpu())


@pytest.mark.parametrize("name", ["clip_a", "clip_b"])
def test_clip_golden_cases_through_the_handle(clip, clip_handle, name):
    """the bounds of tests/test_text_gpu.py::test_tiny_clip_matches_transformers_golden_and_oracle"""
    from oracle import text_oracle as TO
    ids = torch.tensor(G[name + "_ids"])
    hs, pooled = clip_handle.encode(ids[None].to(DEV))
    pooled, hs = pooled[0].float().cpu(), hs[0].float().cpu()
    ref_h, ref_p = torch.tensor(G[name + "_hidden_fp32"]), torch.tensor(G[name + "_pooled_fp32"])
    p16, h16 = TO.clip_text(clip[1], ids, TINY_CLIP, "bf16")
    noise = rel_l2(h16, ref_h)
    assert rel_l2(hs, ref_h) <= 3.0 * noise + 2e-3, (rel_l2(hs, ref_h), noise)
    assert rel_l2(pooled, ref_p) <= 3.0 * rel_l2(p16, ref_p) + 4e-3


# ---------------------------------------------------------------------------------------------------- the product's head geometry
def test_t5_xxl_width_one_layer_is_bit_identical(hip):
    """d_model 4096, 64 heads x 64, d_ff 10240, 128 tokens: the batched-GEMM strides at product width without the product's depth"""
    from visualcloze_amd.handle import TextHandle
    m, _ = make_t5(T5_XXL_1)
    ids = tiny_ids(128, 512, seed=77)[None].to(DEV)
    want = m(ids)
    got, _ = TextHandle(m).encode(ids)
    torch.cuda.synchronize()
    assert got.shape == (1, 128, 4096) and torch.isfinite(got.float()).all() and float(got.float().std()) > 0
    assert torch.equal(got, want)


def test_clip_l_width_one_layer_is_bit_identical(hip):
    """768 wide, 12 heads, 3072, 77 tokens padded to 128 rows"""
    from visualcloze_amd.handle import TextHandle
    m, _ = make_clip(CLIP_L_1)
    ids = tiny_ids(77, 512, seed=78, eos=511, eos_at=20)[None].to(DEV)
    want_p, want_h = m(ids)
    got_h, got_p = TextHandle(m).encode(ids)
    torch.cuda.synchronize()
    assert got_h.shape == (1, 77, 768) and got_p.shape == (1, 768) and float(got_h.float().std()) > 0
    assert torch.equal(got_h, want_h) and torch.equal(got_p, want_p) and torch.equal(got_p[0], got_h[0, 20])


# ---------------------------------------------------------------------------------------------------- batches, streams, plans
def test_three_prompts_in_one_call_equal_three_calls(t5_handle, clip_handle, ref):
    r = ref["t5", 64]
    got, _ = t5_handle.encode(r["ids"])
    assert torch.equal(got, r["hidden"])
    assert torch.equal(got, torch.cat([t5_handle.encode(r["ids"][i:i + 1])[0] for i in range(3)]))
    r = ref["clip", 24]
    hs, pooled = clip_handle.encode(r["ids"])
    assert torch.equal(hs, r["hidden"]) and torch.equal(pooled, r["pooled"])
    one = [clip_handle.encode(r["ids"][i:i + 1]) for i in range(3)]
    assert torch.equal(hs, torch.cat([o[0] for o in one])) and torch.equal(pooled, torch.cat([o[1] for o in one]))


def test_null_stream_runs_the_same_plan_uncaptured(t5_handle, clip_handle, ref):
    torch.cuda.synchronize()
    n_t5, n_clip = t5_handle.plan_count(), clip_handle.plan_count()
    got, _ = t5_handle.encode(ref["t5", 128]["ids"], stream=None)
    hs, pooled = clip_handle.encode(ref["clip", 7]["ids"], stream=None)
    torch.cuda.synchronize()
    assert (t5_handle.plan_count(), clip_handle.plan_count()) == (n_t5, n_clip)
    assert torch.equal(got, ref["t5", 128]["hidden"])
    assert torch.equal(hs, ref["clip", 7]["hidden"]) and torch.equal(pooled, ref["clip", 7]["pooled"])


def test_a_stream_that_is_not_the_current_one_is_ordered(t5_handle, clip_handle, ref):
    st = torch.cuda.Stream()
    ids = ref["t5", 64]["ids"] + 0                       # produced on the current stream just before the call
    got, _ = t5_handle.encode(ids, stream=st.cuda_stream)  # ... which runs on `st` and hands back on the current stream
    assert torch.equal(got, ref["t5", 64]["hidden"])
    hs, pooled = clip_handle.encode(ref["clip", 24]["ids"] + 0, stream=st.cuda_stream)
    assert torch.equal(hs, ref["clip", 24]["hidden"]) and torch.equal(pooled, ref["clip", 24]["pooled"])


def test_plan_count_per_workspace_and_length_and_zero_after_a_rebind(hip, t5, ref):
    from visualcloze_amd.handle import TextHandle
    hd = TextHandle(t5[0])
    a = hd.encode(ref["t5", 64]["ids"])[0]
    assert hd.plan_count() == 1                          # three prompts, one plan
    hd.encode(ref["t5", 128]["ids"][:1])
    assert hd.plan_count() == 2
    hd.encode(ref["t5", 64]["ids"][:1])
    assert hd.plan_count() == 2
    # a re-bind drops the plans; with another bias table the result changes, with the old one it comes back
    key = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    old = t5[0].state_dict()[key]
    hd.bind(key, (old * 0.5).contiguous())
    assert hd.plan_count() == 0
    b = hd.encode(ref["t5", 64]["ids"])[0]
    assert hd.plan_count() == 1 and not torch.equal(a, b)
    hd.bind(key, old)
    assert hd.plan_count() == 0 and torch.equal(hd.encode(ref["t5", 64]["ids"])[0], a) and torch.equal(a, ref["t5", 64]["hidden"])


def test_the_ninth_workspace_evicts_the_least_recently_used_plan(hip, t5, ref):
    """The list of captured plans holds 8, most recently used first (include/vcloze_hip.h).  One handle through the raw ABI, L = 64,
    nine workspaces: the ninth plan evicts the first workspace's, which is then captured again - with the same bits."""
    from visualcloze_amd.handle import TextHandle
    L = hip.lib()
    hd = TextHandle(t5[0])
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    r = ref["t5", 64]
    ids = r["ids"][0].to(torch.int32).contiguous()
    need = hd.workspace_bytes(64)
    wss = [torch.empty(need + 256, dtype=torch.uint8, device=DEV) for _ in range(9)]
    outs = [torch.full((64, TINY_T5["d_model"]), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(10)]
    torch.cuda.synchronize()

    def encode(ws, out):
        base = (ws.data_ptr() + 255) & ~255
        assert L.vc_text_prepare(hd.h, 64, base, need, st) == 0, L.vc_last_error()
        assert L.vc_text_encode(hd.h, ids.data_ptr(), 1, out.data_ptr(), None, st) == 0, L.vc_last_error()
        return L.vc_text_plan_count(hd.h)

    assert [encode(ws, out) for ws, out in zip(wss, outs)] == [1, 2, 3, 4, 5, 6, 7, 8, 8]
    assert encode(wss[0], outs[9]) == 8                  # its plan was the least recently used one: evicted, captured again
    stream.synchronize()
    for out in outs:
        assert torch.equal(out, outs[0])
    assert torch.equal(outs[0], r["hidden"][0])


def test_errors_are_reported_before_anything_is_launched(hip, t5, t5_handle, ref):
    L = hip.lib()
    stream = torch.cuda.Stream()                         # a stream of its own: on the null stream nothing would be captured
    st = stream.cuda_stream
    ids = ref["t5", 64]["ids"][0].to(torch.int32).contiguous()
    out = torch.full((64, TINY_T5["d_model"]), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(out.float()).all())

    h2 = C.c_void_p()
    assert L.vc_text_create(C.byref(t5_handle.cfg), C.byref(h2)) == 0
    try:
        sd = t5[0].state_dict()
        names = t5_handle.weight_names()
        missing = "encoder.block.1.layer.1.DenseReluDense.wo.weight"
        for k in names:
            if k != missing:
                shape = (C.c_int64 * sd[k].dim())(*sd[k].shape)
                assert L.vc_text_bind_tensor(h2, k.encode(), sd[k].data_ptr(), shape, sd[k].dim()) == 0, L.vc_last_error()
        need = t5_handle.workspace_bytes(64)
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        base = (ws.data_ptr() + 255) & ~255
        assert L.vc_text_prepare(h2, 64, base, need, st) == 0, L.vc_last_error()
        assert L.vc_text_encode(h2, ids.data_ptr(), 1, out.data_ptr(), None, st) == ERR_STATE
        assert missing.encode() in L.vc_last_error() and untouched()
        shape = (C.c_int64 * 2)(*sd[missing].shape)
        assert L.vc_text_bind_tensor(h2, missing.encode(), sd[missing].data_ptr(), shape, 2) == 0
        assert L.vc_text_encode(h2, ids.data_ptr(), 1, None, None, st) == ERR_ARG and L.vc_last_error() and untouched()
        assert L.vc_text_encode(h2, ids.data_ptr(), 1, out.data_ptr(), out.data_ptr(), st) == ERR_ARG and untouched()
        assert L.vc_text_plan_count(h2) == 0
        # ... and the handle encodes
        assert L.vc_text_encode(h2, ids.data_ptr(), 1, out.data_ptr(), None, st) == 0, L.vc_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, ref["t5", 64]["hidden"][0]) and L.vc_text_plan_count(h2) == 1
    finally:
        L.vc_text_destroy(h2)


# ---------------------------------------------------------------------------------------------------- a C99 caller
def write_demo_input(path, hd, model, ids):
    sd = model.state_dict()
    bits = lambda t: t.detach().to(torch.bfloat16).contiguous().view(torch.int16).cpu().numpy().tobytes()  # noqa: E731
    names = hd.weight_names()
    with open(path, "wb") as f:
        f.write(bytes(hd.cfg))
        f.write(struct.pack("<3i", len(names), ids.shape[0], ids.shape[1]))
        for n in names:
            w = sd[n]
            f.write(struct.pack("<i", len(n)) + n.encode() + struct.pack("<i", w.dim()) + struct.pack(f"<{w.dim()}q", *w.shape))
            f.write(bits(w))
        f.write(ids.to(torch.int32).contiguous().cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def demo_exe(hip, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("text_demo") / "text_handle_demo")
    libdir = os.path.dirname(hip.LIB_PATH)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(ROCM, "include"),
           os.path.join(REPO, "tests", "c_abi", "text_handle_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip", "-L" + os.path.join(ROCM, "lib"),
           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
@pytest.mark.parametrize("which", ["t5", "clip"])
def test_c_host_program_encodes_bit_identically(demo_exe, t5, clip, t5_handle, clip_handle, ref, tmp_path, which):
    """tests/c_abi/text_handle_demo.c: plain C99, no Python in the process - binds the state dict by pointer, encodes two prompts"""
    model, hd, r = (t5[0], t5_handle, ref["t5", 64]) if which == "t5" else (clip[0], clip_handle, ref["clip", 24])
    ids = r["ids"][:2]
    write_demo_input(tmp_path / "in.bin", hd, model, ids)
    p = subprocess.run(["timeout", "-k", "10", "120", demo_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = torch.from_numpy(np.fromfile(tmp_path / "out.bin", dtype=np.int16)).view(torch.bfloat16)
    want = [r["hidden"][:2].cpu().reshape(-1)] + ([r["pooled"][:2].cpu().reshape(-1)] if which == "clip" else [])
    want = torch.cat(want)
    assert got.numel() == want.numel() and torch.equal(got, want)
    hs, pooled = hd.encode(ids)                                             # the ctypes calls give the same bytes
    assert torch.equal(got[:hs.numel()], hs.cpu().reshape(-1)) and (pooled is None or torch.equal(got[hs.numel():], pooled.cpu().reshape(-1)))


# ---------------------------------------------------------------------------------------------------- the opt-in switch
def test_opt_in_switch_leaves_generate_grid_unchanged(hip):
    """T5EncoderModel.use_handle / CLIPTextModel.use_handle route the prompt encoders of the whole pixel-to-pixel path through the
    handle: the same pixels.  The models and inputs are those of tests/test_vae_handle_gpu.py's switch test."""
    from tests.helpers import tiny_model
    from tests.procedural import TINY, procedural_ae_param
    from visualcloze_amd import pipeline
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m, _ = tiny_model()
    dev = "cuda"
    AE = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 1, 1, 1], num_res_blocks=1, z_channels=16,
              scale_factor=0.3611, shift_factor=0.1159)
    CL = dict(vocab_size=128, hidden_size=TINY["vec_in_dim"], intermediate_size=128, num_hidden_layers=1,
              num_attention_heads=1, max_position_embeddings=16, layer_norm_eps=1e-5, eos_token_id=127)
    ae = AutoEncoder(AutoEncoderParams(**AE))
    ae.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in ae.state_dict().items()})
    ae = ae.to(dev).to(torch.bfloat16)
    t5m, _ = make_t5(TINY_T5)
    clm, _ = make_clip(CL)
    H, W = 32, 64
    c = lambda t: t.to(dev, torch.bfloat16)  # noqa: E731
    rows = [c(ptensor((3, H, W), 201 + i, q=7)) for i in range(2)]
    masks = [c(torch.zeros(1, 1, H, W)), c(torch.cat((torch.zeros(1, 1, H, W // 2), torch.ones(1, 1, H, W // 2)), -1))]
    enoise = [c(ptensor((1, 16, H // 8, W // 8), 211 + i, q=5)) for i in range(2)]
    t5_ids, cl_ids = tiny_ids(64, 128, seed=5)[None].to(dev), tiny_ids(16, 128, seed=6, eos=127, eos_at=7)[None].to(dev)

    def run():
        out = pipeline.generate_grid(m, ae, t5m, clm, rows, masks, t5_ids, cl_ids, seed=3, cfg=30.0, steps=4, encode_noise=enoise)
        torch.cuda.synchronize()
        return out
    assert t5m.use_handle is False and clm.use_handle is False
    off = run()
    assert t5m.__dict__.get("_text_handle") is None and clm.__dict__.get("_text_handle") is None      # off: no handle is built
    t5m.use_handle = clm.use_handle = True
    on = run()
    assert t5m.handle().plan_count() >= 1 and clm.handle().plan_count() >= 1
    assert len(on) == len(off) == 2
    for a, b in zip(on, off):
        assert a.shape == (3, H, W) and torch.equal(a, b)
    assert float(off[1].std()) > 0
    # and the modules' own return values
    assert torch.equal(t5m(t5_ids), make_t5(TINY_T5)[0](t5_ids))
    p_on, h_on = clm(cl_ids)
    p_off, h_off = make_clip(CL)[0](cl_ids)
    assert torch.equal(p_on, p_off) and torch.equal(h_on, h_off)
