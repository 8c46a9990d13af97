"""CPU: the C-ABI surface of the autoencoder handle (vc_vae_*, detected by symbol: VC_ABI_VERSION does not move) - exported,
declared, bound - its weight list against `AutoEncoder.state_dict()`, and the argument errors that are raised on the host before
a device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.procedural import TINY_AE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        h.build()
    return h


def make_handle(hip, P):
    m = P["ch_mult"]
    cfg = hip.VaeConfig(P["in_channels"], P["ch"], P["out_ch"], (C.c_int32 * 8)(*m), len(m), P["num_res_blocks"], P["z_channels"],
                        P["scale_factor"], P["shift_factor"])
    h = C.c_void_p()
    rc = hip.lib().vc_vae_create(C.byref(cfg), C.byref(h))
    return rc, h


def test_header_declares_exactly_the_exported_vae_symbols(hip):
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    declared = {s for s in re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr) if s.startswith("vc_vae_")}
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("vc_vae_")}
    bound = {s for s in hip.SYMBOLS if s.startswith("vc_vae_")}
    assert declared == exported == bound, (declared ^ exported, declared ^ bound)
    assert {"vc_vae_create", "vc_vae_destroy", "vc_vae_bind_weight", "vc_vae_workspace_bytes", "vc_vae_prepare", "vc_vae_decode",
            "vc_vae_encode", "vc_vae_plan_count", "vc_vae_struct_sizes"} <= declared
    # additive: the version a caller checks did not move, the handle is detected by symbol
    assert int(re.search(r"#define VC_ABI_VERSION (\d+)\b", hdr).group(1)) == hip.ABI_VERSION == hip.lib().vc_abi_version()


def test_config_mirror_has_the_size_the_library_reports(hip):
    size = (C.c_int32 * 1)()
    hip.lib().vc_vae_struct_sizes(size)
    assert size[0] == C.sizeof(hip.VaeConfig) == (3 + 8 + 3) * 4 + 2 * 4
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    for name, val in (("VC_VAE_ENCODER", hip.VAE_ENCODER), ("VC_VAE_DECODER", hip.VAE_DECODER), ("VC_VAE_LATENT_BF16", hip.VAE_LATENT_BF16),
                      ("VC_VAE_LATENT_F32", hip.VAE_LATENT_F32), ("VC_VAE_TOKENS", hip.VAE_TOKENS)):
        assert re.search(rf"#define {name} {val}\b", hdr), name


@pytest.mark.parametrize("which", ["tiny", "flux"])
def test_weight_list_is_the_state_dict_in_order(hip, which):
    from visualcloze_amd.vae import FLUX_AE, AutoEncoder, AutoEncoderParams
    P = TINY_AE if which == "tiny" else FLUX_AE
    rc, h = make_handle(hip, P)
    assert rc == 0, hip.lib().vc_last_error()
    try:
        names, buf = [], C.create_string_buffer(160)
        while hip.lib().vc_vae_weight_name(h, len(names), buf, 160) == 0:
            names.append(buf.value.decode())
        sd = AutoEncoder(AutoEncoderParams(**P)).state_dict()
        assert [n + ".weight" for n in names] == [k for k in sd if k.endswith(".weight")]
        assert all(n + ".bias" in sd for n in names) and 2 * len(names) == len(sd)
    finally:
        hip.lib().vc_vae_destroy(h)


def test_host_only_argument_errors(hip):
    L = hip.lib()
    rc, h = make_handle(hip, TINY_AE)
    assert rc == 0
    try:
        n = C.c_int64(-7)
        for H, W, which in ((13, 16, 3), (16, 0, 3), (-8, 16, 3), (16, 16, 0), (16, 16, 4), (1 << 17, 16, 3)):
            assert L.vc_vae_workspace_bytes(h, H, W, which, C.byref(n)) == ERR_ARG, (H, W, which)
            assert L.vc_last_error() and n.value == -7
        assert L.vc_vae_workspace_bytes(h, 16, 24, 3, None) == ERR_ARG
        assert L.vc_vae_workspace_bytes(None, 16, 24, 3, C.byref(n)) == ERR_ARG
        assert L.vc_vae_workspace_bytes(h, 16, 24, hip.VAE_DECODER, C.byref(n)) == 0 and n.value > 0
        dec = n.value
        assert L.vc_vae_workspace_bytes(h, 16, 24, hip.VAE_ENCODER | hip.VAE_DECODER, C.byref(n)) == 0 and n.value > dec
        # an unknown name and a wrong shape are refused before the pointers are looked at
        shape = (C.c_int64 * 4)(64, 3, 3, 3)
        assert L.vc_vae_bind_weight(h, b"encoder.conv_inn", 0x1000, 0x1000, 0, shape, 4, None) == ERR_ARG
        assert b"encoder.conv_inn" in L.vc_last_error()
        shape = (C.c_int64 * 4)(64, 4, 3, 3)
        assert L.vc_vae_bind_weight(h, b"encoder.conv_in.weight", 0x1000, 0x1000, 0, shape, 4, None) == ERR_ARG
        assert b"encoder.conv_in" in L.vc_last_error() and b"[64, 3, 3, 3]" in L.vc_last_error()
        assert L.vc_vae_plan_count(h) == 0 and L.vc_vae_plan_count(None) == -1
    finally:
        L.vc_vae_destroy(h)
    bad = dict(TINY_AE, ch=48)
    rc, _ = make_handle(hip, bad)
    assert rc == ERR_ARG and b"ch_mult" in L.vc_last_error()


def test_copies_of_the_module_do_not_share_its_handle():
    """copy.deepcopy / pickling an AutoEncoder whose VaeHandle exists: the handle (a C pointer that owns device memory) stays with
    the original; the copy keeps the switch and builds its own on first use."""
    import copy
    import pickle

    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams

    class Owner:                                   # stands for handle.VaeHandle: must never be copied
        def __reduce__(self):
            raise RuntimeError("the handle was copied")

    ae = AutoEncoder(AutoEncoderParams(**TINY_AE))
    ae.use_handle = True
    ae.__dict__["_vae_handle"] = (("key",), Owner())
    for twin in (copy.deepcopy(ae), pickle.loads(pickle.dumps(ae))):
        assert twin.__dict__["_vae_handle"] is None and twin.use_handle is True
        assert list(twin.state_dict()) == list(ae.state_dict())
    assert ae.__dict__["_vae_handle"] is not None
