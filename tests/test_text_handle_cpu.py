"""CPU: the C-ABI surface of the text-encoder handle (vc_text_*, detected by symbol: VC_ABI_VERSION does not move) and of the three
glue entry points it adds (vc_t5_*, vc_clip_*) - exported, declared, bound - its tensor list against the modules' `state_dict()`,
the host-side relative-position buckets against `text.t5_relative_buckets`, and the argument errors that are raised on the host
before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from tests.procedural import TINY_CLIP, TINY_T5

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -3
FAKE = 0x10000          # a 256-byte aligned "device pointer" that is never dereferenced: binding is by pointer, on the host


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        h.build()
    return h


def t5_config(hip, cfg):
    return hip.TextConfig(hip.TEXT_T5, cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads,
                          cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance, 0, 0, cfg.layer_norm_epsilon)


def clip_config(hip, cfg):
    return hip.TextConfig(hip.TEXT_CLIP, cfg.vocab_size, cfg.hidden_size, cfg.hidden_size // cfg.num_attention_heads, cfg.intermediate_size,
                          cfg.num_hidden_layers, cfg.num_attention_heads, 0, 0, cfg.max_position_embeddings, cfg.eos_token_id,
                          cfg.layer_norm_eps)


def create(hip, cfg):
    h = C.c_void_p()
    rc = hip.lib().vc_text_create(C.byref(cfg) if cfg is not None else None, C.byref(h))
    return rc, h


def names_of(hip, h):
    names, buf = [], C.create_string_buffer(160)
    while hip.lib().vc_text_weight_name(h, len(names), buf, 160) == 0:
        names.append(buf.value.decode())
    return names


def test_header_declares_exactly_the_exported_text_symbols(hip):
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    mine = lambda s: s.startswith(("vc_text_", "vc_t5_", "vc_clip_"))  # noqa: E731
    declared = {s for s in re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr) if mine(s)}
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and mine(ln.split()[-1])}
    bound = {s for s in hip.SYMBOLS if mine(s)}
    assert declared == exported == bound, (declared ^ exported, declared ^ bound)
    assert {"vc_text_struct_sizes", "vc_text_create", "vc_text_destroy", "vc_text_weight_name", "vc_text_bind_tensor", "vc_text_workspace_bytes",
            "vc_text_prepare", "vc_text_encode", "vc_text_plan_count", "vc_t5_relative_buckets", "vc_t5_position_bias", "vc_clip_embed",
            "vc_clip_pool"} == declared
    # additive: the version a caller checks did not move, the handle is detected by symbol
    assert int(re.search(r"#define VC_ABI_VERSION (\d+)\b", hdr).group(1)) == hip.ABI_VERSION == hip.lib().vc_abi_version() == 11


def test_config_mirror_has_the_size_the_library_reports(hip):
    size = (C.c_int32 * 1)()
    hip.lib().vc_text_struct_sizes(size)
    assert size[0] == C.sizeof(hip.TextConfig) == 12 * 4
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    for name, val in (("VC_TEXT_T5", hip.TEXT_T5), ("VC_TEXT_CLIP", hip.TEXT_CLIP)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert (hip.TEXT_T5, hip.TEXT_CLIP) == (1, 2)


@pytest.mark.parametrize("which", ["tiny_t5", "tiny_clip", "t5_xxl", "clip_l"])
def test_weight_list_is_the_state_dict_in_order(hip, which):
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    with torch.device("meta"):                       # the real widths without their 9 GB
        if which.endswith("t5") or which == "t5_xxl":
            cfg = T5Config(**TINY_T5) if which == "tiny_t5" else T5Config()
            model, ccfg = T5EncoderModel(cfg), t5_config(hip, cfg)
        else:
            cfg = CLIPTextConfig(**TINY_CLIP) if which == "tiny_clip" else CLIPTextConfig()
            model, ccfg = CLIPTextModel(cfg), clip_config(hip, cfg)
    rc, h = create(hip, ccfg)
    assert rc == 0, hip.lib().vc_last_error()
    try:
        sd = model.state_dict()
        names = names_of(hip, h)
        assert names == list(sd)
        if ccfg.kind == hip.TEXT_T5:
            assert names[:2] == ["shared.weight", "encoder.embed_tokens.weight"]
        # every listed shape is the module's: a bind with the state dict's shape is accepted, one with another shape is not
        L = hip.lib()
        for k in (names[0], names[1], names[len(names) // 2], names[-1]):
            shape = (C.c_int64 * sd[k].dim())(*sd[k].shape)
            assert L.vc_text_bind_tensor(h, k.encode(), FAKE, shape, sd[k].dim()) == 0, (k, L.vc_last_error())
            shape[0] += 1
            assert L.vc_text_bind_tensor(h, k.encode(), FAKE, shape, sd[k].dim()) == ERR_ARG and k.encode() in L.vc_last_error()
    finally:
        hip.lib().vc_text_destroy(h)


@pytest.mark.parametrize("nb,md", [(32, 128), (8, 16)])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 64, 65, 128, 129, 192, 512])
def test_relative_buckets_equal_the_torch_table(hip, L, nb, md):
    from visualcloze_amd.text import t5_relative_buckets
    want = t5_relative_buckets(L, nb, md)                                   # [L, L] for key j - query i
    got = torch.tensor(hip.t5_relative_buckets(L, nb, md))
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    assert got.shape == (2 * L - 1,) and torch.equal(got[(j - i) + L - 1], want)
    # ... which reads the torch table along (j - i): its first column (j - i <= 0, reversed) and its first row (j - i >= 0)
    assert got.tolist() == want[:, 0].flip(0).tolist() + want[0, 1:].tolist()


def test_relative_buckets_argument_errors(hip):
    L = hip.lib()
    out = (C.c_int32 * 3)()
    for args in ((0, 32, 128), (2, 2, 128), (2, 33, 128), (2, 256, 128), (2, 32, 8)):
        assert L.vc_t5_relative_buckets(*args, out) == ERR_ARG and L.vc_last_error(), args
    assert L.vc_t5_relative_buckets(2, 32, 128, None) == ERR_ARG


def bind_all(hip, h, model):
    sd = model.state_dict()
    for k in names_of(hip, h):
        shape = (C.c_int64 * sd[k].dim())(*sd[k].shape)
        assert hip.lib().vc_text_bind_tensor(h, k.encode(), FAKE, shape, sd[k].dim()) == 0, k


def test_host_only_argument_errors(hip):
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    L = hip.lib()
    # create
    h = C.c_void_p()
    assert L.vc_text_create(None, C.byref(h)) == ERR_ARG and L.vc_last_error()
    t5c, clc = T5Config(**TINY_T5), CLIPTextConfig(**TINY_CLIP)
    bad = t5_config(hip, t5c)
    bad.kind = 0
    assert create(hip, bad)[0] == ERR_ARG and b"kind" in L.vc_last_error()
    bad = t5_config(hip, t5c)
    bad.d_model = 136                                    # a multiple of 8, not of the GEMM's 64-wide K tile
    assert create(hip, bad)[0] == ERR_ARG and b"d_model" in L.vc_last_error()
    bad = clip_config(hip, clc)
    bad.d_model = 96                                     # a head of 48
    assert create(hip, bad)[0] == ERR_ARG and L.vc_last_error()
    with torch.device("meta"):
        t5m, clm = T5EncoderModel(t5c), CLIPTextModel(clc)
    n = C.c_int64(-7)
    rc, t5 = create(hip, t5_config(hip, t5c))
    assert rc == 0
    rc, cl = create(hip, clip_config(hip, clc))
    assert rc == 0
    try:
        # sequence lengths
        for bad_l in (0, -64, 63, 65, 100):
            assert L.vc_text_workspace_bytes(t5, bad_l, C.byref(n)) == ERR_ARG and n.value == -7, bad_l
            assert L.vc_text_prepare(t5, bad_l, FAKE, 1 << 40, None) == ERR_ARG
        assert b"64" in L.vc_last_error()
        for bad_l in (0, -1, clc.max_position_embeddings + 1):
            assert L.vc_text_workspace_bytes(cl, bad_l, C.byref(n)) == ERR_ARG and n.value == -7, bad_l
            assert L.vc_text_prepare(cl, bad_l, FAKE, 1 << 40, None) == ERR_ARG
        assert b"max_positions" in L.vc_last_error()
        assert L.vc_text_workspace_bytes(t5, 64, None) == ERR_ARG and L.vc_text_workspace_bytes(None, 64, C.byref(n)) == ERR_ARG
        assert L.vc_text_workspace_bytes(t5, 64, C.byref(n)) == 0 and n.value > 0
        small = n.value
        assert L.vc_text_workspace_bytes(t5, 128, C.byref(n)) == 0 and n.value > small
        assert L.vc_text_workspace_bytes(cl, 7, C.byref(n)) == 0 and n.value > 0
        seven = n.value
        assert L.vc_text_workspace_bytes(cl, 24, C.byref(n)) == 0 and n.value >= seven       # both pad to 64 rows
        # a workspace that is too small, or misaligned
        assert L.vc_text_prepare(t5, 64, FAKE, small - 1, None) == ERR_ARG and b"too small" in L.vc_last_error()
        assert L.vc_text_prepare(t5, 64, FAKE + 8, small + 8, None) == ERR_ARG and L.vc_text_prepare(t5, 64, None, small, None) == ERR_ARG
        # binding: unknown key, wrong shape, null pointer - the key is in the message
        shape = (C.c_int64 * 2)(t5c.vocab_size, t5c.d_model)
        assert L.vc_text_bind_tensor(t5, b"shared.weightt", FAKE, shape, 2) == ERR_ARG and b"shared.weightt" in L.vc_last_error()
        assert L.vc_text_bind_tensor(t5, b"shared.weight", FAKE, shape, 1) == ERR_ARG and b"shared.weight" in L.vc_last_error()
        assert b"[128, 128]" in L.vc_last_error()
        shape[1] += 8
        assert L.vc_text_bind_tensor(t5, b"encoder.embed_tokens.weight", FAKE, shape, 2) == ERR_ARG       # the tied key is shape-checked too
        assert b"encoder.embed_tokens.weight" in L.vc_last_error()
        shape[1] -= 8
        assert L.vc_text_bind_tensor(t5, b"shared.weight", None, shape, 2) == ERR_ARG and b"shared.weight" in L.vc_last_error()
        assert L.vc_text_bind_tensor(t5, None, FAKE, shape, 2) == ERR_ARG
        # encode: argument errors first, then the state - nothing bound, then nothing prepared
        assert L.vc_text_encode(t5, FAKE, 1, FAKE, FAKE, None) == ERR_ARG and b"pooled" in L.vc_last_error()
        assert L.vc_text_encode(t5, FAKE, 1, None, None, None) == ERR_ARG and L.vc_text_encode(cl, FAKE, 1, None, None, None) == ERR_ARG
        assert L.vc_text_encode(t5, None, 1, FAKE, None, None) == ERR_ARG and L.vc_text_encode(t5, FAKE, 0, FAKE, None, None) == ERR_ARG
        assert L.vc_text_encode(t5, FAKE, 1, FAKE, None, None) == ERR_STATE and b"'shared.weight'" in L.vc_last_error()
        assert L.vc_text_encode(cl, FAKE, 1, FAKE, FAKE, None) == ERR_STATE and b"token_embedding.weight" in L.vc_last_error()
        bind_all(hip, t5, t5m)
        bind_all(hip, cl, clm)
        assert L.vc_text_encode(t5, FAKE, 1, FAKE, None, None) == ERR_STATE and b"vc_text_prepare" in L.vc_last_error()
        assert L.vc_text_encode(cl, FAKE, 1, None, FAKE, None) == ERR_STATE and b"vc_text_prepare" in L.vc_last_error()
        assert L.vc_text_plan_count(t5) == 0 and L.vc_text_plan_count(None) == -1
    finally:
        L.vc_text_destroy(t5)
        L.vc_text_destroy(cl)


@pytest.mark.parametrize("which", ["t5", "clip"])
def test_copies_of_the_module_do_not_share_its_handle(which):
    """copy.deepcopy / pickling a text encoder whose TextHandle exists: the handle (a C pointer) stays with the original; the copy
    keeps the switch and builds its own on first use."""
    import copy
    import pickle

    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel

    class Owner:                                   # stands for handle.TextHandle: must never be copied
        def __reduce__(self):
            raise RuntimeError("the handle was copied")

    m = T5EncoderModel(T5Config(**TINY_T5)) if which == "t5" else CLIPTextModel(CLIPTextConfig(**TINY_CLIP))
    assert m.use_handle is False
    m.use_handle = True
    m.__dict__["_text_handle"] = (("key",), Owner())
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert twin.__dict__["_text_handle"] is None and twin.use_handle is True
        assert list(twin.state_dict()) == list(m.state_dict())
    assert m.__dict__["_text_handle"] is not None
