"""The flow-matching loss without a GPU: transport.fm_loss_terms pinned to the reference's own Transport.training_losses in float64,
Transport.sample / fm_times pinned to its times (f64) and to the host rule vc_fm_times (f32), the ABI surface and every argument
refusal of vc_fm_plan / vc_fm_loss / vc_fm_times, and Transport.training_losses on a foreign callable.

The pin: tests/golden/fm_loss_golden.npz holds what the reference computed in float64 (tests/golden/make_fm_loss_golden.py) and the
draws it made.  fm_loss_terms restates it expression for expression; the allowed relative gap is the summation bound n * 2^-53 with
n the summed elements (at most 5 * 8 = 40 per sample here).  Measured: 0.0 over the 25 cases - bit-equal."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW_SYMBOLS = ("vc_fm_plan", "vc_fm_loss", "vc_fm_times", "vc_flux_eval_loss")
P = 0x10000          # a non-null, 16-byte aligned address no refused call ever touches


@pytest.fixture(scope="module")
def gen():
    """the fixture generator as a module: the toy model, the cases and the shapes are defined there, once"""
    spec = importlib.util.spec_from_file_location("make_fm_loss_golden", os.path.join(GOLDEN, "make_fm_loss_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "fm_loss_golden.npz"))


def _case(gen, golden, case):
    name, snr, shift, masked, with_cond, bs = case
    g = lambda k: torch.from_numpy(golden[k])  # noqa: E731
    kw = {"img_mask": g("mask")[:bs]} if masked else {}
    return (g("x1")[:bs], g("cond")[:bs] if with_cond else None, kw, g(name + "_base"), g(name + "_t"), g(name + "_x0"), g(name + "_loss"))


def _model(gen):
    return lambda xin, timesteps, img_mask=None: gen.toy_model(xin, timesteps)


# ---------------------------------------------------------------------------------------------- 1. the reference pin
def test_fm_loss_terms_equals_the_reference_in_f64(gen, golden):
    """every golden case: relative gap <= n * 2^-53, n the elements summed per sample.  Measured maximum: 0.0 (bit-equal)."""
    from visualcloze_amd import transport as T
    cases = gen.cases()
    assert len(cases) == 25 and {c[1] for c in cases} == set(gen.SNR_TYPES) and any(c[5] == 1 for c in cases)
    worst = 0.0
    for case in cases:
        x1, cond, kw, _, t, x0, ref = _case(gen, golden, case)
        terms = T.fm_loss_terms(_model(gen), x1, t, x0, kw, cond)
        assert terms["loss"].dtype == torch.float64 and terms["loss"].shape == ref.shape == (case[5],)
        assert torch.equal(terms["t"], t) and torch.equal(terms["loss"], terms["task_loss"])
        n = gen.N * gen.C
        gap = float(((terms["loss"] - ref).abs() / ref.abs()).max())
        worst = max(worst, gap)
        assert gap <= n * 2.0 ** -53, f"{case[0]}: {gap:.3e}"
    print(f"fm_loss_terms vs the reference, f64: max relative gap {worst:.3e}")


def test_times_equal_the_reference_in_f64(gen, golden, monkeypatch):
    """fm_times on the recorded base draws, and Transport.sample with those draws replayed: the reference's t and x0, bit for bit"""
    from visualcloze_amd import transport as T
    for case in gen.cases():
        name, snr, shift, masked, with_cond, bs = case
        x1, _, _, base, t, x0, _ = _case(gen, golden, case)
        assert torch.equal(T.fm_times(base, snr, gen.N, shift), t), name
        monkeypatch.setattr(torch, "randn_like", lambda x: x0.clone())
        monkeypatch.setattr(torch, "rand", lambda size: base.clone())
        monkeypatch.setattr(torch, "normal", lambda mean, std, size: base.clone())
        ts, xs, x1s = T.create_transport("Linear", "velocity", snr_type=snr, do_shift=shift).sample(x1)
        assert torch.equal(ts, t) and torch.equal(xs, x0) and x1s is x1, name


def test_sample_draws_as_the_reference_does(gen, golden):
    """the same torch.manual_seed gives the golden t and x0: randn_like first, then rand / normal of (B,)"""
    from visualcloze_amd import transport as T
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        for i, case in enumerate(gen.cases()):
            x1, _, _, _, t, x0, _ = _case(gen, golden, case)
            torch.manual_seed(500 + i)
            ts, xs, _ = T.create_transport("Linear", "velocity", snr_type=case[1], do_shift=case[2]).sample(x1)
            assert torch.equal(ts, t) and torch.equal(xs, x0), case[0]
    finally:
        torch.set_default_dtype(prev)


@pytest.mark.parametrize("n_tokens", [256, 3456, 14400])
def test_f32_times_equal_the_host_rule_bit_for_bit(n_tokens):
    from visualcloze_amd import hip, transport as T
    g = torch.Generator().manual_seed(n_tokens)
    uni = torch.cat((torch.tensor([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23, 1.0]), torch.rand(250, generator=g)))
    nrm = torch.cat((torch.tensor([0.0, -0.0, 17.0, 17.5, 30.0, 100.0, -30.0, -100.0, -200.0]), torch.randn(250, generator=g)))
    for snr, base in (("uniform", uni), ("uniform_0.2_0.8", uni), ("uniform_1e-3_0.999", uni), ("lognorm", nrm)):
        for shift in (True, False):
            a, b = T.fm_times(base, snr, n_tokens, shift), hip.fm_times(base, snr, n_tokens, shift)
            assert a.dtype == b.dtype == torch.float32
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (snr, shift, (a != b).nonzero().flatten().tolist())
    # the endpoints go through inf arithmetic: t = 1 stays 1 under the shift (draw 1.0; a lognorm draw whose sigmoid rounds to 1)
    assert float(hip.fm_times(torch.tensor([1.0]), "uniform", n_tokens, True)) == 1.0
    assert float(hip.fm_times(torch.tensor([100.0]), "lognorm", n_tokens, True)) == 1.0
    assert float(hip.fm_times(torch.tensor([-200.0]), "lognorm", n_tokens, True)) == 0.0


# ---------------------------------------------------------------------------------------------- 2. the ABI surface
def test_abi_surface():
    from visualcloze_amd import hip
    L = hip.lib()
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    declared = set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NEW_SYMBOLS:
        assert name in declared and name in hip.SYMBOLS and name in exported, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m and len(hip.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    assert declared == set(hip.SYMBOLS)
    assert L.vc_abi_version() == 11 == hip.ABI_VERSION and re.search(r"#define VC_ABI_VERSION 11\b", hdr)
    sizes = (C.c_int32 * 7)()
    L.vc_struct_sizes(sizes)
    assert list(sizes) == [240, 1032, 56, 152, 56, 80, 56]
    assert hip.FM_LOSS_MAX_BLOCKS == int(re.search(r"#define VC_FM_LOSS_MAX_BLOCKS (\d+)", hdr).group(1))
    assert hip.FM_MAX_HOST_COUNTS == int(re.search(r"#define VC_FM_MAX_HOST_COUNTS (\d+)", hdr).group(1))


def _refused(rc, L, *words):
    assert rc == -1, rc                                   # VC_ERR_ARG
    msg = L.vc_last_error().decode()
    assert all(w in msg for w in words), msg


def test_fm_plan_argument_errors_without_a_device():
    from visualcloze_amd import hip
    L = hip.lib()
    ok = dict(x1=P, f32=0, bs=5 * 64, ld=64, t=P, x0=None, seed=1, off=0, xt=P, xld=384, ut=P, B=2, rows=5, cols=64)

    def call(**k):
        a = dict(ok, **k)
        return L.vc_fm_plan(a["x1"], a["f32"], a["bs"], a["ld"], a["t"], a["x0"], a["seed"], a["off"], a["xt"], a["xld"], a["ut"], a["B"], a["rows"],
                            a["cols"], None)

    for k in ("x1", "t", "xt", "ut"):
        _refused(call(**{k: None}), L, "null")
    for k in ("B", "rows", "cols"):
        _refused(call(**{k: 0}), L, "positive")
        _refused(call(**{k: -3}), L, "positive")
    _refused(call(bs=-1), L, "x1_bstride")
    _refused(call(ld=63), L, "smaller than cols")
    _refused(call(xld=63), L, "smaller than cols")
    _refused(call(x1=P + 1), L, "aligned")
    _refused(call(x1=P + 2, f32=1), L, "aligned")
    _refused(call(x0=P + 1), L, "aligned")
    _refused(call(xt=P + 1), L, "aligned")
    _refused(call(ut=P + 2), L, "aligned")
    _refused(call(t=P + 2), L, "aligned")
    _refused(call(off=(1 << 64) - 2 * 5 * 64 + 1), L, "wraps")            # the last position would be 2^64
    _refused(call(B=1 << 30, rows=1 << 40, cols=1 << 20, ld=1 << 20, xld=1 << 20), L, "64-bit")


def test_fm_loss_argument_errors_without_a_device():
    from visualcloze_amd import hip
    L = hip.lib()
    ok = dict(out=P, ld=64, ut=P, valid=None, host=0, loss=P, scratch=P, B=3, rows=70, cols=64)

    def call(**k):
        a = dict(ok, **k)
        v = a["valid"]
        keep = (C.c_int32 * len(v))(*v) if isinstance(v, (list, tuple)) else None
        vp = C.cast(keep, C.c_void_p) if keep is not None else v
        return L.vc_fm_loss(a["out"], a["ld"], a["ut"], vp, a["host"], a["loss"], a["scratch"], a["B"], a["rows"], a["cols"], None)

    for k in ("out", "ut", "loss", "scratch"):
        _refused(call(**{k: None}), L, "null")
    for k in ("B", "rows", "cols"):
        _refused(call(**{k: 0}), L, "positive")
    _refused(call(B=65536), L, "65535")
    _refused(call(ld=63), L, "smaller than cols")
    _refused(call(out=P + 1), L, "aligned")
    _refused(call(ut=P + 2), L, "aligned")
    _refused(call(loss=P + 1), L, "aligned")
    _refused(call(valid=P + 2), L, "aligned")
    _refused(call(rows=1 << 31, cols=8), L, "units")
    _refused(call(valid=[70, 0, 1], host=1), L, "valid_rows[1] = 0")      # zero valid rows: no loss
    _refused(call(valid=[70, 33, 71], host=1), L, "valid_rows[2] = 71")
    _refused(call(valid=[1] * 65, host=1, B=65), L, "at most 64")


def test_fm_times_argument_errors():
    from visualcloze_amd import hip, transport as T
    L = hip.lib()
    buf = (C.c_float * 4)(0.1, 0.2, 0.3, 0.4)
    out = (C.c_float * 4)()
    assert L.vc_fm_times(b"uniform", buf, 4, 256, 1, out) == 0
    _refused(L.vc_fm_times(None, buf, 4, 256, 1, out), L, "null")
    _refused(L.vc_fm_times(b"uniform", None, 4, 256, 1, out), L, "null")
    _refused(L.vc_fm_times(b"uniform", buf, 4, 256, 1, None), L, "null")
    _refused(L.vc_fm_times(b"uniform", buf, 0, 256, 1, out), L, "n = 0")
    _refused(L.vc_fm_times(b"uniform", buf, 4, 0, 1, out), L, "n_tokens")
    for bad in ("", "Uniform", "cosine", "lognormal", "uniformly"):
        _refused(L.vc_fm_times(bad.encode(), buf, 4, 256, 1, out), L, "Not implemented snr_type")
        with pytest.raises(NotImplementedError):
            T.parse_snr_type(bad)
        with pytest.raises(NotImplementedError):
            T.create_transport(snr_type=bad).sample(torch.zeros(2, 3, 4))
    for bad in ("uniform_", "uniform_0.2", "uniform_0.2_", "uniform__0.8", "uniform_a_b", "uniform_0.1_0.2_0.3", "uniform_0x1_2", "uniform_inf_1",
                "uniform_nan_1", "uniform_ 0.2_0.8", "uniform_1e999_2"):
        _refused(L.vc_fm_times(bad.encode(), buf, 4, 256, 1, out), L, "uniform_<t0>_<t1>")
        with pytest.raises(ValueError):
            T.parse_snr_type(bad)
    assert T.parse_snr_type("uniform_0.2_0.8") == ("uniform", 0.2, 0.8) and T.parse_snr_type("lognorm") == ("lognorm", 0.0, 1.0)
    assert T.create_transport().snr_type == "uniform" and T.create_transport(snr_type="lognorm").snr_type == "lognorm"


def test_flux_eval_loss_refuses_a_null_handle():
    from visualcloze_amd import hip
    L = hip.lib()
    t = (C.c_float * 1)(0.5)
    _refused(L.vc_flux_eval_loss(None, P, 0, P, t, None, 0, 0, P, None), L, "null handle")


# ---------------------------------------------------------------------------------------------- 3. training_losses, eager
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_training_losses_on_a_foreign_callable(gen, golden, dtype):
    from visualcloze_amd import transport as T
    x1 = torch.from_numpy(golden["x1"]).to(dtype)
    cond = torch.from_numpy(golden["cond"]).to(dtype)
    mask = torch.from_numpy(golden["mask"])
    model = lambda xin, timesteps, img_mask=None: gen.toy_model(xin.float(), timesteps.float()).to(xin.dtype)  # noqa: E731
    tr = T.create_transport("Linear", "velocity", snr_type="lognorm", do_shift=True)
    for kw in ({}, {"img_mask": mask}):
        for c in (cond, None):
            torch.manual_seed(7)
            t, x0, _ = tr.sample(x1)
            assert t.dtype == dtype and x0.dtype == dtype and t.shape == (3,)
            torch.manual_seed(7)
            terms = tr.training_losses(model, x1, kw, {"cond": c})
            ref = T.fm_loss_terms(model, x1, t, x0, kw, c)
            assert set(terms) == {"loss", "task_loss", "t"}
            assert torch.equal(terms["loss"], ref["loss"]) and torch.equal(terms["t"], t) and torch.equal(terms["task_loss"], terms["loss"])
            assert terms["loss"].shape == (3,) and terms["loss"].dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
            assert not terms["loss"].requires_grad and terms["loss"].grad_fn is None
            given = tr.training_losses(model, x1, kw, {"cond": c}, t=t, x0=x0)           # given draws: the same numbers
            assert torch.equal(given["loss"], terms["loss"])
            if dtype != torch.float64:      # the ordered sum is the same sum in another order: within n * 2^-24 of torch's
                o = T.fm_loss_terms(model, x1, t, x0, kw, c, ordered=True)["loss"]
                assert float(((o - ref["loss"]).abs() / ref["loss"]).max()) <= 40 * 2.0 ** -24


def test_training_losses_carries_no_graph_and_refuses_lists():
    from visualcloze_amd import transport as T
    w = torch.ones(8, requires_grad=True)
    model = lambda xin, timesteps: xin * w  # noqa: E731
    x1 = torch.randn(2, 5, 8, requires_grad=True)
    tr = T.create_transport()
    terms = tr.training_losses(model, x1, None, None)
    assert terms["loss"].requires_grad is False and terms["loss"].grad_fn is None and terms["task_loss"].requires_grad is False
    doc = T.Transport.training_losses.__doc__.lower()
    assert "back-propagated" in doc and "evaluation" in doc
    for call in (lambda: tr.training_losses(model, [x1[0], x1[1]]), lambda: tr.training_losses(model, (x1[0],)), lambda: tr.sample([x1[0]])):
        with pytest.raises(NotImplementedError, match="list of tensors"):
            call()
    with pytest.raises(ValueError):
        tr.training_losses(model, x1, t=torch.zeros(3))
