"""CPU: the host-only surface of the torch noise stream (include/vcloze_hip.h, THE TORCH STREAM; csrc/rng_torch.hip) - the grid and
offset rule vc_torch_randn_policy held to a few-line restatement of the header's formula, the argument errors that come back before
any device work, the declarations, the unchanged ABI, `pipeline.TorchNoiseStream`'s bookkeeping and the C demo compiling as C99.
The values themselves are held to torch.randn on the device (tests/test_torch_noise_gpu.py)."""
import ctypes as C
import os
import re
import shutil

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC_ERR_ARG, VC_ERR_HIP = -1, -2
P = 0x10000000          # a 16-byte aligned stand-in for a device pointer; never dereferenced
NEW = ("vc_torch_randn_policy", "vc_randn_torch", "vc_randn_torch_tokens", "vc_grid_set_noise")
NS = [1, 4, 255, 256, 257, 524288, 524289, 1 << 31]
CAPS = [(256, 2048), (1, 256), (304, 2560)]


def policy(n: int, sm_count: int, threads_per_sm: int):
    """the header's rule: (G, the advance of the offset)"""
    cap = sm_count * (threads_per_sm // 256)
    G = min(-(-n // 256), cap)
    return G, ((n - 1) // (4 * 256 * G) + 1) * 4


@pytest.fixture(scope="module")
def hdr():
    return open(os.path.join(REPO, "include", "vcloze_hip.h")).read()


@pytest.fixture(scope="module")
def L():
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def _policy(L, n, sm, tpsm):
    g, adv = C.c_int32(-1), C.c_uint64(0)
    rc = L.vc_torch_randn_policy(n, sm, tpsm, C.byref(g), C.byref(adv))
    return rc, g.value, adv.value


@pytest.mark.parametrize("caps", CAPS)
@pytest.mark.parametrize("n", NS)
def test_policy_is_the_headers_formula(L, n, caps):
    assert _policy(L, n, *caps) == (0, *policy(n, *caps))


def test_policy_spot_values():
    """the restatement itself, at values worked out by hand: below the cap one round of ceil(n/256) blocks; at the cap T = 524288
    threads take four elements each per round"""
    assert policy(1, 256, 2048) == (1, 4) and policy(257, 256, 2048) == (2, 4)
    assert policy(524288, 256, 2048) == (2048, 4) and policy(524289, 256, 2048) == (2048, 4)
    assert policy(4 * 524288, 256, 2048) == (2048, 4) and policy(4 * 524288 + 1, 256, 2048) == (2048, 8)
    assert policy(257, 1, 256) == (1, 4) and policy(1025, 1, 256) == (1, 8) and policy(1 << 31, 1, 256) == (1, 1 << 23)
    assert policy(1 << 31, 304, 2560) == (3040, ((2 ** 31 - 1) // (4 * 256 * 3040) + 1) * 4)


@pytest.mark.parametrize("args, word", [
    ((0, 256, 2048), "n >= 1"),
    ((-3, 256, 2048), "n >= 1"),
    (((1 << 48) + 1, 256, 2048), "2^48"),
    ((16, -1, 2048), "sm_count"),
    ((16, 256, 255), "threads_per_sm"),
    ((16, 256, -256), "threads_per_sm"),
    ((16, 1 << 30, 1 << 30), "cap"),
])
def test_policy_argument_errors(L, args, word):
    rc, _, _ = _policy(L, *args)
    msg = L.vc_last_error().decode()
    assert rc == VC_ERR_ARG and msg.startswith("torch_randn_policy:") and word in msg, msg
    assert L.vc_torch_randn_policy(16, 256, 2048, None, None) == VC_ERR_ARG and b"null" in L.vc_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine without a device")
def test_the_current_devices_properties_need_a_device(L):
    """sm_count = 0 / threads_per_sm = 0 mean the current device's: without one the call says so, it does not guess"""
    for sm, tpsm in ((0, 0), (0, 2048), (256, 0)):
        rc, _, _ = _policy(L, 16, sm, tpsm)
        assert rc == VC_ERR_HIP and b"device" in L.vc_last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(out=None), "null"),
    (dict(n=0), "n >= 1"),
    (dict(n=-5), "n >= 1"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(offset=2), "multiple of 4"),
    (dict(offset=(1 << 64) - 1), "multiple of 4"),
    (dict(offset=(1 << 64) - 4, n=1025, sm=1, tpsm=256), "wraps"),       # two rounds: the advance is 8
    (dict(offset=(1 << 64) - 4, n=1 << 21, tpsm=256), "wraps"),
    (dict(out=P + 1, dtype=0), "aligned"),
    (dict(out=P + 2, dtype=1), "aligned"),
    (dict(out=P + 2, dtype=2), "aligned"),
    (dict(tpsm=255), "threads_per_sm"),
    (dict(tpsm=1), "threads_per_sm"),
    (dict(sm=-2), "sm_count"),
])
def test_randn_torch_argument_errors_come_back_before_any_device_work(L, kw, word):
    a = dict(out=P, dtype=0, n=16, seed=1, offset=0, sm=256, tpsm=2048)
    a.update(kw)
    assert L.vc_randn_torch(a["out"], a["dtype"], a["n"], a["seed"], a["offset"], a["sm"], a["tpsm"], None) == VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert msg.startswith("randn_torch:") and word in msg, msg


@pytest.mark.parametrize("kw, word", [
    (dict(tokens=None), "null"),
    (dict(C=0), "even"),
    (dict(C=15), "even"),
    (dict(h=3), "even"),
    (dict(w=-2), "even"),
    (dict(ld=68), "multiples of 8"),
    (dict(col0=4), "multiples of 8"),
    (dict(ld=64, col0=8), "col0 + 4C <= ld"),
    (dict(tokens=P + 8), "16-byte"),
    (dict(offset=6), "multiple of 4"),
    (dict(offset=(1 << 64) - 4, sm=1, tpsm=256), "wraps"),            # 384 elements on 256 threads: one round, the advance 4 wraps
    (dict(C=1 << 30, h=1 << 30, w=1 << 30, ld=1 << 40), "2^48"),
    (dict(tpsm=128), "threads_per_sm"),
])
def test_randn_torch_tokens_argument_errors_come_back_before_any_device_work(L, kw, word):
    a = dict(tokens=P, C=16, h=4, w=6, ld=64, col0=0, seed=1, offset=0, sm=256, tpsm=2048)
    a.update(kw)
    assert L.vc_randn_torch_tokens(a["tokens"], a["C"], a["h"], a["w"], a["ld"], a["col0"], a["seed"], a["offset"], a["sm"], a["tpsm"],
                                   None) == VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert msg.startswith("randn_torch_tokens:") and word in msg, msg


def test_the_last_offset_is_a_legal_one(L):
    """offset + advance may reach 2^64 - 4 + 4 only by wrapping; 2^64 - 8 + 4 does not: only the null pointer is left to object to"""
    assert L.vc_randn_torch(None, 0, 4, 1, (1 << 64) - 8, 256, 2048, None) == VC_ERR_ARG and b"null" in L.vc_last_error()


def test_grid_set_noise_refusals(L):
    assert L.vc_grid_set_noise(None, 1, 0, 0) == VC_ERR_ARG and b"null handle" in L.vc_last_error()


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_is_unchanged(L, hdr):
    from visualcloze_amd import hip
    declared = set(re.findall(r"^(?:int|void|int64_t|const char\*)\s+(vc_\w+)\s*\(", hdr, re.M))
    lib = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, hdr)
        assert m and name in declared and hasattr(lib, name), name
        assert name in hip.SYMBOLS and len(hip.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    assert declared == set(hip.SYMBOLS), declared ^ set(hip.SYMBOLS)
    assert re.search(r"#define VC_ABI_VERSION 11\b", hdr) and hip.ABI_VERSION == 11 and L.vc_abi_version() == 11
    assert re.search(r"#define VC_NOISE_OWN 0\b", hdr) and re.search(r"#define VC_NOISE_TORCH 1\b", hdr)
    assert (hip.NOISE_OWN, hip.NOISE_TORCH) == (0, 1)
    assert "look up vc_randn_torch" in hdr and "THE TORCH STREAM" in hdr
    assert callable(hip.randn_torch) and callable(hip.torch_randn_policy) and callable(hip.randn_torch_tokens)


SIZES = {"vc_struct_sizes": [240, 1032, 56, 152, 56, 80, 56], "vc_vae_struct_sizes": [64], "vc_text_struct_sizes": [48],
         "vc_monitor_struct_sizes": [16], "vc_grid_struct_sizes": [32, 536, 224], "vc_photo_struct_sizes": [48, 176, 224]}


@pytest.mark.parametrize("fn", sorted(SIZES))
def test_struct_sizes_are_what_they_were(L, fn):
    """no Vc* struct grew with the noise switch (it is a call on the handle, not a field): the sizes before this entry point existed"""
    out = (C.c_int32 * len(SIZES[fn]))()
    getattr(L, fn)(out)
    assert list(out) == SIZES[fn]


def test_torch_noise_stream_bookkeeping(monkeypatch):
    from visualcloze_amd import hip, pipeline
    calls = []

    def fake(shape, seed, offset=0, dtype=torch.bfloat16, device=None, sm_count=0, threads_per_sm=0, out=None, stream=None):
        calls.append((tuple(shape), seed, offset, dtype, sm_count, threads_per_sm))
        return torch.zeros(shape, dtype=dtype)
    monkeypatch.setattr(hip, "randn_torch", fake)
    s = pipeline.TorchNoiseStream(77, sm_count=1, threads_per_sm=512)       # cap 2: T = 512 threads at most
    assert isinstance(s, pipeline.NoiseStream) and s.seed == 77 and s.offset == 0
    a = s.randn([1, 16, 4, 8])                                              # 512 elements: G = 2, one round
    assert a.shape == (1, 16, 4, 8) and a.dtype == torch.bfloat16 and s.offset == 4
    s.randn((3, 700), torch.float32)                                        # 2100 elements on 512 threads: two rounds
    assert s.offset == 12
    s.randn([7])
    assert s.offset == 16
    assert calls == [((1, 16, 4, 8), 77, 0, torch.bfloat16, 1, 512), ((3, 700), 77, 4, torch.float32, 1, 512), ((7,), 77, 12, torch.bfloat16, 1, 512)]
    for bad in (-4, 1 << 64, 6):
        with pytest.raises(ValueError):
            s.offset = bad
    s.offset = (1 << 64) - 4
    with pytest.raises(ValueError):
        s.randn([5])                       # the advance would wrap; nothing was drawn, nothing moved
    with pytest.raises(ValueError):
        s.randn([0])
    assert s.offset == (1 << 64) - 4 and len(calls) == 3
    s.offset = (1 << 64) - 8
    s.randn([4])                           # ... the last advance that fits
    assert s.offset == (1 << 64) - 4
    assert pipeline.TorchNoiseStream(5, offset=8).offset == 8


def test_the_stochastic_sampler_refuses_the_torch_stream():
    from visualcloze_amd import pipeline
    from visualcloze_amd.transport import Sampler, create_transport
    rng = pipeline.TorchNoiseStream(3, sm_count=256, threads_per_sm=2048)
    fn = Sampler(create_transport("Linear", "velocity", do_shift=True)).sample_sde(diffusion_form="linear", num_steps=4, rng=rng)
    with pytest.raises(ValueError, match="TorchNoiseStream"):
        fn(torch.zeros(1, 4, 8), lambda x, t, **kw: x)
    with pytest.raises(ValueError, match="TorchNoiseStream"):
        pipeline._no_torch_stream(rng, "sde")
    pipeline._no_torch_stream(pipeline.NoiseStream(3), "sde")


def test_documents_state_the_stream_and_its_caveats(hdr):
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(REPO, doc)).read()
        assert "vc_randn_torch" in txt and "TorchNoiseStream" in txt, doc
    assert "cannot be restated by a host without" not in hdr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_demo_compiles_and_links_as_c99(L, tmp_path):
    """tests/c_abi/torch_noise_demo.c names nothing but the C ABI and the HIP runtime (it runs in tests/test_torch_noise_gpu.py)"""
    from tests.torch_noise_demo_build import build_torch_noise_demo
    assert os.path.getsize(build_torch_noise_demo(tmp_path)) > 0
