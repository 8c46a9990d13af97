"""CPU: true classifier-free guidance (Flux.forward_with_cfg, models/model.py:126-145) as far as it works without a GPU - the C ABI
additions (header, binding and library agree; VC_ABI_VERSION and the struct sizes do not move), the argument errors that need no
device, the Python refusals, and the fixture tests/golden/cfg_golden.npz (the reference's own runs, make_cfg_golden.py) against the
oracle's tiny forward followed by the literal torch expression."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vc_cfg_combine", "vc_flux_set_cfg"}
VC_ERR_ARG = -1


def _lib():
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def _generator():
    spec = importlib.util.spec_from_file_location("make_cfg_golden", os.path.join(REPO, "tests", "golden", "make_cfg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cg():
    return np.load(os.path.join(REPO, "tests", "golden", "cfg_golden.npz"))


def test_abi_header_binding_and_library_agree():
    from visualcloze_amd import hip
    lib = _lib()
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    assert int(re.search(r"#define VC_ABI_VERSION (\d+)\b", hdr).group(1)) == hip.ABI_VERSION == lib.vc_abi_version() == 11
    declared = set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(hip.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("vc_")}
    assert exported == declared
    raw = ctypes.CDLL(hip.LIB_PATH)
    assert all(hasattr(raw, n) for n in NEW)
    # no struct changed: the sizes of the parent commit, which the ctypes mirrors (untouched by this feature) still have
    sizes = (ctypes.c_int32 * 7)()
    lib.vc_struct_sizes(sizes)
    assert list(sizes) == [240, 1032, 56, 152, 56, 80, 56]
    assert list(sizes) == [ctypes.sizeof(t) for t in (hip.GemmProblem, hip.GemmArgs, hip.LnStream, hip.Attention, hip.FluxConfig,
                                                      hip.FluxInputs, hip.FluxLaunchClass)]
    # the header cites the reference and states the roundings
    for phrase in ("model.py:126-145", "bf16( uncond[i] + bf16( f32(cfg_scale) * bf16( cond[i] - uncond[i] ) ) )", "NOT rounded to bf16",
                   "not the identity"):
        assert phrase in hdr, phrase


def test_argument_checks_that_need_no_device():
    lib = _lib()
    a, b, c = 0x10000, 0x20000, 0x30000
    for args, word in (((None, b, c, 8, 1.0), b"null"), ((a, None, c, 8, 1.0), b"null"), ((a, b, None, 8, 1.0), b"null"),
                       ((a, b, c, 0, 1.0), b"positive"), ((a, b, c, -8, 1.0), b"positive"),
                       ((a, b, c, 8, float("inf")), b"finite"), ((a, b, c, 8, float("nan")), b"finite"),
                       ((a, b, a + 2, 8, 1.0), b"overlap"),          # out one element into cond
                       ((a, b, b - 2, 8, 1.0), b"overlap"),          # out's last element is uncond's first
                       ((a, a + 16, a + 8, 8, 1.0), b"overlap")):
        assert lib.vc_cfg_combine(*args, None) == VC_ERR_ARG, args
        assert b"cfg_combine" in lib.vc_last_error() and word in lib.vc_last_error(), (args, lib.vc_last_error())
    assert lib.vc_flux_set_cfg(None, 1, 3.5) == VC_ERR_ARG and b"null handle" in lib.vc_last_error()
    assert lib.vc_flux_set_cfg(None, 0, 0.0) == VC_ERR_ARG


def _tiny_cpu_model():
    from tests.procedural import TINY
    from visualcloze_amd.model import Flux, FluxParams
    return Flux(FluxParams(**TINY))


def test_python_surface_and_refusals():
    from visualcloze_amd.handle import FluxHandle
    from visualcloze_amd.model import Flux, FluxLoraWrapper
    from visualcloze_amd.transport import Sampler, StepCache, create_transport
    p = inspect.signature(Flux.forward_with_cfg).parameters
    assert list(p) == ["self", "img", "img_ids", "txt", "txt_ids", "timesteps", "y", "txt_mask", "img_mask", "guidance", "cfg_scale"]
    assert p["cfg_scale"].default == 1.0 and p["guidance"].default is None
    assert FluxLoraWrapper.forward_with_cfg is Flux.forward_with_cfg and callable(FluxHandle.set_cfg)
    m = _tiny_cpu_model()
    z = torch.zeros
    with pytest.raises(ValueError, match="odd batch of 3"):
        m.forward_with_cfg(z(3, 24, 384), z(3, 24, 3), z(3, 16, 128), z(3, 16, 3), z(3), z(3, 64), guidance=z(3), cfg_scale=2.0)
    s = Sampler(create_transport("Linear", "velocity", do_shift=True))
    fn = s.sample_ode(sampling_method="euler", num_steps=3, step_cache=StepCache(0.1))
    with pytest.raises(ValueError, match="forward_with_cfg"):
        fn(z(2, 24, 64), m.forward_with_cfg, dict(cfg_scale=2.0))


def _oracle(sd, inp, t, P, guidance_is_bf16):
    import oracle.flux_oracle as O
    from tests.procedural import TINY
    G = O.FluxGeometry(**TINY)
    orig = O.compute_vec
    O.compute_vec = lambda *a, **k: orig(*a, **{**k, "guidance_is_bf16": guidance_is_bf16})
    try:
        return O.flux_forward(sd, G, torch.cat((inp["x"], inp["cond"]), -1), inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"],
                              inp["txt_mask"], inp["img_mask"], inp["guidance"], P=P)
    finally:
        O.compute_vec = orig


@pytest.mark.parametrize("B", [2, 4])
def test_oracle_forward_plus_the_torch_expression_reproduces_the_fixture(cg, tiny_sd, B):
    """fp32: the bound tests/test_oracle_golden.py holds the tiny model to (2e-5 of the output's scale, max-abs).  bf16: that file's
    bf16 bound for the tiny model (rel-L2 5e-2 against the reference's own bf16 autocast run, bf16 guidance)."""
    import oracle.flux_oracle as O
    gen = _generator()
    inp, t, s = gen.cfg_inputs(B), torch.tensor(cg[f"fwd_b{B}_t"]), float(cg["cfg_scale"])
    assert s == 3.5 and torch.equal(t, gen.cfg_timesteps(B))
    h = B // 2
    v = _oracle(tiny_sd, inp, t, O.Prec("fp32"), False)
    c, u = v[:h], v[h:]
    got = torch.cat([u + s * (c - u), u], dim=0)
    ref = torch.tensor(cg[f"fwd_b{B}"])
    err = (got - ref).abs().max().item()
    print(f"\n[tiny, B={B}] oracle fp32 forward + torch expression vs the reference's forward_with_cfg: max-abs {err:.2e}")
    assert got.shape == ref.shape and err <= 2e-5 * max(1.0, ref.abs().max().item())
    vb = _oracle(tiny_sd, inp, t, O.Prec("bf16", "ref"), True).to(torch.bfloat16)
    c, u = vb[:h], vb[h:]
    gotb = torch.cat([u + s * (c - u), u], dim=0)
    assert gotb.dtype == torch.bfloat16
    refb = torch.tensor(cg[f"fwd_b{B}_bf16"])
    rel = ((gotb.float() - refb).norm() / refb.norm()).item()
    print(f"[tiny, B={B}] oracle bf16 forward + torch expression vs the reference's bf16 autocast run: rel-L2 {rel:.2e}")
    assert rel < 5e-2


def test_the_recipe_is_the_torch_expression_bitwise():
    """out = bf16(u + bf16(f32(s) * bf16(c - u))), s not rounded to bf16: the recipe vc_cfg_combine implements, against torch's own
    `u + s * (c - u)` on bf16 tensors (CPU), and that s = 1 is not the identity."""
    g = torch.Generator().manual_seed(3)
    c, u = (torch.randn(1 << 14, generator=g) * 2).bfloat16(), (torch.randn(1 << 14, generator=g) * 2).bfloat16()
    bf = lambda x: x.bfloat16().float()  # noqa: E731
    for s in (1.0, 3.7, 0.0, -1.5, 7.123456789, 1e-3):
        want = u + s * (c - u)
        s32 = torch.tensor(s, dtype=torch.float32)
        got = bf(u.float() + bf(s32 * bf(c.float() - u.float())))
        assert torch.equal(got, want.float()), s
    assert not torch.equal(u + 1.0 * (c - u), c)


def test_pair_chunks_and_mask_layout_with_index_lists():
    """The sampler chunks a true-CFG batch by pairs; `MaskLayout` then takes lists of sample indices where it took slices: the rows of
    a list are the rows of its samples one by one, and what went through img_rows comes back through img_rows_back."""
    from visualcloze_amd.model import MaskLayout
    from visualcloze_amd.transport import cfg_chunks
    assert cfg_chunks(2, 4) == [[0, 1]] and cfg_chunks(4, 4) == [[0, 1, 2, 3]]
    assert cfg_chunks(6, 4) == [[0, 1, 3, 4], [2, 5]] and cfg_chunks(10, 4) == [[0, 1, 5, 6], [2, 3, 7, 8], [4, 9]]
    assert cfg_chunks(4, 2) == [[0, 2], [1, 3]]
    for B in (2, 4, 6, 10):
        assert sorted(i for c in cfg_chunks(B, 4) for i in c) == list(range(B))
    with pytest.raises(ValueError):
        cfg_chunks(3, 4)
    B, T, N = 6, 5, 7
    g = torch.Generator().manual_seed(1)
    tm, im = (torch.rand(B, T, generator=g) > 0.3).int(), (torch.rand(B, N, generator=g) > 0.3).int()
    x, ids = torch.randn(B, N, 4, generator=g), torch.randn(B, T, 3, generator=g)
    for lay in (MaskLayout(tm, im, B, T, N), MaskLayout(None, None, B, T, N)):
        for idx in ([0, 1, 3, 4], [2, 5], [5]):
            one = [slice(i, i + 1) for i in idx]
            assert torch.equal(lay.img_rows(x, idx), torch.cat([lay.img_rows(x, s) for s in one]))
            assert torch.equal(lay.txt_rows(ids, idx), torch.cat([lay.txt_rows(ids, s) for s in one]))
            assert lay.kv_len(idx) == [lay.kv_len(s)[0] for s in one]
            gaps = [(lay.kv_gap(s) or [(0, 0)])[0] for s in one]
            assert (lay.kv_gap(idx) or [(0, 0)] * len(idx)) == gaps
            assert torch.equal(lay.img_rows_back(lay.img_rows(x, idx), idx), x[idx])
        assert torch.equal(lay.img_rows(x, slice(1, 4)), lay.img_rows(x, [1, 2, 3]))      # a slice is the list of its samples
