"""CPU: the opt-in first-block step cache of the fused Euler loop as far as it works without a GPU - the C ABI
additions (header, binding and library agree), the `StepCache` value type and the sampler's refusals.

The ABI version: the additions are new entry points only, so - like the solver entry points before them - they are detected by
SYMBOL and VC_ABI_VERSION does not move (tests/test_lora_merge_cpu.py and tests/test_solvers_cpu.py pin the number); what is
asserted here is that header, binding and library name the SAME version and the same set of symbols."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vc_residual_change", "vc_residual_sub", "vc_residual_add", "vc_flux_set_step_cache", "vc_flux_step_cache_stats"}


def _lib():
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def test_abi_header_binding_and_library_agree():
    from visualcloze_amd import hip
    lib = _lib()
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    version = int(re.search(r"#define VC_ABI_VERSION (\d+)\b", hdr).group(1))
    assert version == hip.ABI_VERSION == lib.vc_abi_version()
    declared = set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(hip.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("vc_")}
    assert exported == declared
    raw = ctypes.CDLL(hip.LIB_PATH)
    assert all(hasattr(raw, n) for n in NEW)
    assert re.search(r"#define VC_RESIDUAL_CHANGE_MAX_BLOCKS 256\b", hdr) and hip.RESIDUAL_CHANGE_MAX_BLOCKS == 256
    # the header says in plain words what the cache is
    for phrase in ("IT CHANGES RESULTS", "unmeasured", "no default\n * threshold is recommended"):
        assert phrase in hdr, phrase


def test_argument_checks_that_need_no_device():
    lib = _lib()
    assert lib.vc_flux_set_step_cache(None, 0.1, 1) == -1 and b"null handle" in lib.vc_last_error()       # VC_ERR_ARG
    assert lib.vc_flux_step_cache_stats(None, None, None, None, 0) == -1
    assert lib.vc_residual_change(None, None, None, None, None, None, None, 1, 8, None) == -1
    assert b"residual_change" in lib.vc_last_error()
    assert lib.vc_residual_sub(None, 0, None, 0, None, 0, 1, 8, None) == -1 and b"residual_sub" in lib.vc_last_error()
    assert lib.vc_residual_add(None, 0, None, 0, None, 0, 1, 8, None) == -1 and b"residual_add" in lib.vc_last_error()
    # 16-byte accesses only: n and the strides in multiples of 8 (no device is touched before the check)
    assert lib.vc_residual_add(0x1000, 16, 0x2000, 16, 0x3000, 16, 2, 12, None) == -1 and b"multiples of 8" in lib.vc_last_error()
    assert lib.vc_residual_change(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, None, 0x6000, 1, 12, None) == -1
    assert b"multiple of 8" in lib.vc_last_error()


def test_step_cache_value_type():
    from visualcloze_amd.transport import StepCache
    c = StepCache(0.05)
    assert (c.threshold, c.max_consecutive) == (0.05, 1)
    c = StepCache(threshold=math.inf, max_consecutive=3)
    assert c.threshold == math.inf and c.max_consecutive == 3 and "max_consecutive=3" in repr(c)
    assert StepCache(1, -1).max_consecutive == -1 and StepCache(1, -1) == StepCache(1.0, -1) and StepCache(1, 2) != StepCache(1, 3)
    assert len({StepCache(0.5, 2), StepCache(0.5, 2)}) == 1
    with pytest.raises(AttributeError):
        c.threshold = 1.0
    for bad in (0, 0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="threshold"):
            StepCache(bad)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="max_consecutive"):
            StepCache(0.1, bad)
    for bad in ("0.1", None, True):
        with pytest.raises(TypeError):
            StepCache(bad)
    for bad in (1.0, "1", True):
        with pytest.raises(TypeError):
            StepCache(0.1, bad)


def test_sampler_keyword_default_and_refusals():
    import torch
    from visualcloze_amd.transport import Sampler, StepCache, create_transport
    s = Sampler(create_transport("Linear", "velocity", do_shift=True))
    sig = inspect.signature(s.sample_ode)
    assert sig.parameters["step_cache"].default is None and sig.parameters["step_cache"].kind is inspect.Parameter.KEYWORD_ONLY
    assert s.last_step_cache_stats is None
    for m in ("midpoint", "rk4"):
        with pytest.raises(ValueError, match="euler"):
            s.sample_ode(sampling_method=m, num_steps=4, step_cache=StepCache(0.1))
    with pytest.raises(NotImplementedError):          # an unknown solver is still that error, cache or not
        s.sample_ode(sampling_method="dopri5", step_cache=StepCache(0.1))
    with pytest.raises(TypeError, match="StepCache"):
        s.sample_ode(sampling_method="euler", step_cache=0.1)
    # a foreign callable has no cache: refused, never silently ignored
    fn = s.sample_ode(sampling_method="euler", num_steps=3, step_cache=StepCache(0.1))
    with pytest.raises(ValueError, match="foreign"):
        fn(torch.zeros(1, 8, 2), lambda x, timesteps, **k: x, {})
    # and without the keyword the same callable steps as ever
    out = s.sample_ode(sampling_method="euler", num_steps=3)(torch.zeros(1, 8, 2), lambda x, timesteps, **k: torch.ones_like(x), {})
    assert torch.allclose(out, torch.full_like(out, -1.0), atol=1e-6)


def test_pipeline_entry_points_pass_the_cache_through():
    from visualcloze_amd import pipeline
    for name in ("denoise_grid", "sdedit_upsample", "sdedit_upsample_batch", "generate_grid", "upsample_image", "upsample_images",
                 "generate_and_upsample"):
        p = inspect.signature(getattr(pipeline, name)).parameters
        assert "step_cache" in p and p["step_cache"].default is None, name


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c99_demo_still_links_and_the_new_entry_points_are_c_clean(tmp_path):
    from tests.test_c_abi import build_demo
    exe = build_demo(tmp_path)
    assert os.path.getsize(exe) > 0
    src = tmp_path / "cache.c"
    src.write_text('#include "vcloze_hip.h"\n'
                   "int main(void) {\n"
                   "  int32_t c = 0, r = 0; float m[4];\n"
                   "  int rc = vc_flux_set_step_cache((void*)0, 0.1f, 1);\n"
                   "  rc |= vc_flux_step_cache_stats((void*)0, &c, &r, m, 4);\n"
                   "  rc |= vc_residual_sub((void*)0, 0, (void*)0, 0, (void*)0, 0, 1, 8, (void*)0);\n"
                   "  return rc == VC_ERR_ARG && VC_RESIDUAL_CHANGE_MAX_BLOCKS == 256 ? 0 : 1;\n"
                   "}\n")
    from visualcloze_amd import hip
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(hip.LIB_PATH)
    out = tmp_path / "cache"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem",
                        os.path.join(rocm, "include"), str(src), "-o", str(out), "-L" + libdir, "-lvcloze_hip",
                        "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert subprocess.run([str(out)]).returncode == 0          # argument errors only: no device is touched
