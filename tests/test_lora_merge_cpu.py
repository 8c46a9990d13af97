"""CPU: the C-ABI surface of vc_lora_merge (ABI 11) - exported, declared, bound - and its argument checks, which run before
the first HIP call: host integers stand in for device pointers and no device is touched."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC_ERR_ARG = -1
P = 0x10000000          # a 16-byte aligned stand-in for a device pointer; never dereferenced


@pytest.fixture(scope="module")
def L():
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def call(L, w=P, w_is_f32=0, ldw=64, a=P + 0x1000000, lda=64, b=P + 0x2000000, ldb=16, scale=1.0, out=P + 0x3000000, ldo=64,
         bias=None, bias_is_f32=0, bB=None, bias_out=None, O=32, I=64, R=16):
    return L.vc_lora_merge(w, w_is_f32, ldw, a, lda, b, ldb, scale, out, ldo, bias, bias_is_f32, bB, bias_out, O, I, R, None)


def test_abi_11_declares_exports_and_binds_vc_lora_merge(L):
    from visualcloze_amd import hip
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    assert re.search(r"#define VC_ABI_VERSION 11\b", hdr)
    assert re.search(r"\bint vc_lora_merge\s*\(", hdr) and "lora.py:66-67" in hdr and "92-98" in hdr
    assert hip.ABI_VERSION == 11 and L.vc_abi_version() == 11
    assert "vc_lora_merge" in hip.SYMBOLS and hasattr(C.CDLL(hip.LIB_PATH), "vc_lora_merge")
    assert len(hip.SYMBOLS["vc_lora_merge"][1]) == 18
    assert callable(hip.lora_merge)


@pytest.mark.parametrize("kw, word", [
    (dict(w=None), "null"),
    (dict(out=None), "null"),
    (dict(a=None), "factor"),
    (dict(b=None), "factor"),
    (dict(R=513), "rank"),
    (dict(R=-1), "rank"),
    (dict(O=0), "positive"),
    (dict(I=0), "positive"),
    (dict(O=-4), "positive"),
    (dict(ldw=63), "stride"),
    (dict(ldo=63), "stride"),
    (dict(lda=63), "stride"),
    (dict(ldb=15), "stride"),
    (dict(out=P, w_is_f32=1), "in place"),                    # out == w with an f32 weight
    (dict(out=P, ldo=128), "in place"),                       # out == w, different strides
    (dict(out=P + 2), "overlaps"),                            # shifted by one element
    (dict(out=P + 64 * 2 * 31), "overlaps"),                  # out begins in the last row of w
    (dict(out=P - 64 * 2 * 31), "overlaps"),                  # out ends in the first row of w
    (dict(w_is_f32=1, out=P + 64 * 4 * 32 - 4), "overlaps"),  # the f32 weight is twice as long
    (dict(out=P + 0x1000000), "lora_a"),
    (dict(out=P + 0x2000000), "lora_b"),
    (dict(bias=P + 0x4000000), "bias_out"),
    (dict(bB=P + 0x4000000), "bias_out"),
    (dict(bias_out=P + 0x5000000), "bias_out"),
    (dict(bias=P + 0x4000000, bias_is_f32=1, bias_out=P + 0x4000000), "in place"),
    (dict(bias=P + 0x4000000, bias_out=P + 0x4000000 + 2), "overlaps"),
])
def test_argument_errors_come_back_before_any_device_work(L, kw, word):
    assert call(L, **kw) == VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert msg.startswith("lora_merge:") and word in msg, msg


def test_model_knob_and_fingerprint():
    from tests.procedural import TINY, TINY_RANK
    from visualcloze_amd.model import Flux, FluxLoraWrapper, FluxParams, Linear
    m = FluxLoraWrapper(lora_rank=TINY_RANK, params=FluxParams(**TINY))
    assert m.lora_merge == "torch"
    f0 = m._weights_fingerprint()
    m.lora_merge = "hip"
    assert m._weights_fingerprint() != f0
    with pytest.raises(ValueError):
        Flux.merged_linear(Linear(8, 8), backend="blas")
