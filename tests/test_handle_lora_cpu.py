"""CPU: the C-ABI surface of the handle's un-merged LoRA mode and per-block taps (vc_flux_bind_lora, vc_flux_set_lora_scale,
vc_flux_set_tap, vc_flux_tap_shape - detected by symbol: VC_ABI_VERSION and the struct sizes do not move), the bindings behind
`handle.FluxHandle`, and the model attributes that choose who runs lora_mode "ref"."""
import inspect
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_flux_bind_lora", "vc_flux_set_lora_scale", "vc_flux_set_tap", "vc_flux_tap_shape"]


def test_new_entry_points_are_declared_exported_and_bound():
    from visualcloze_amd import handle, hip
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    lib = hip.lib()
    src = inspect.getsource(handle.FluxHandle)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name                       # declared
        fn = getattr(lib, name)                                                  # exported
        res, args = hip.SYMBOLS[name]
        assert fn.argtypes == args and fn.restype is res and len(args) >= 2      # argtypes set where handle.py calls through
        assert f"lib().{name}(" in src, f"handle.FluxHandle never calls {name}"
    # the header's parameter counts are the bindings'
    for name in NEW:
        params = re.search(r"\bint %s\(([^;]*)\);" % name, hdr, re.S).group(1)
        assert len(params.split(",")) == len(hip.SYMBOLS[name][1]), name
    for method in ("bind_lora", "set_lora_mode", "set_lora_scale", "set_tap", "tap_shape"):
        assert callable(getattr(handle.FluxHandle, method))
    assert int(re.search(r"#define VC_ABI_VERSION (\d+)\b", hdr).group(1)) == hip.ABI_VERSION == lib.vc_abi_version()
    assert (hip.LAUNCH_PASS, hip.LAUNCH_TAP) == (4, 5) and re.search(r"VC_LAUNCH_PASS = 4\b", hdr) and re.search(r"VC_LAUNCH_TAP = 5\b", hdr)


def test_null_handles_are_refused_without_a_device():
    import ctypes as C
    from visualcloze_amd import hip
    L = hip.lib()
    rows, cols = C.c_int64(0), C.c_int32(0)
    for rc in (L.vc_flux_bind_lora(None, b"img_in", None, 0, None, 0, None, 0, 0, 0), L.vc_flux_set_lora_scale(None, 1.0),
               L.vc_flux_set_tap(None, b"img_in", None), L.vc_flux_tap_shape(None, b"img_in", C.byref(rows), C.byref(cols))):
        assert rc == -1 and b"null handle" in L.vc_last_error()


def test_ref_plan_defaults_and_values():
    from tests.procedural import TINY
    from visualcloze_amd.model import Flux, FluxLoraWrapper, FluxParams
    m = FluxLoraWrapper(lora_rank=8, lora_scale=1.0, params=FluxParams(**TINY))
    assert m.lora_mode == "merged" and m.ref_plan == "python" and m.use_handle is True      # the defaults are what they were
    assert Flux.set_lora_scale is FluxLoraWrapper.set_lora_scale and callable(Flux.block_taps)
    m.set_lora_scale(0.5)                                                                    # un-prepared: the modules' scale alone
    assert all(lin.scale == 0.5 for _, lin in m._linears())
    for bad in ("c", "Handle", None, 1):
        m.ref_plan = bad
        with pytest.raises(ValueError, match="ref_plan"):
            m.handle()
        with pytest.raises(ValueError, match="ref_plan"):
            m.set_lora_scale(1.0)
        assert all(lin.scale == 0.5 for _, lin in m._linears())
    for ok in ("python", "handle"):
        m.ref_plan = ok
        m._check_ref_plan()
