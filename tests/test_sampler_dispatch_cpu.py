"""CPU: which path - the fused solve on the C handle or the eager one on the host - each of the four Sampler methods takes for a
model callable, a state dtype and a pair of masks; that `cfg_scale` leaves the kwargs and reaches the path that runs; and every
`step_cache` refusal of sample_ode.  The runners are replaced by recorders and `Flux.handle` by a stub, so nothing is computed: the
table below IS the routing, written out from the four methods as they stood when each still spelt it for itself."""
import pytest
import torch

from tests.procedural import TINY, tiny_inputs

bf16, f32, f16, f64 = torch.bfloat16, torch.float32, torch.float16, torch.float64
# sample_ode is listed at two solvers: without the C handle the Python-ordered plan steps "euler" and nothing else
METHODS = ("ode_euler", "ode_rk4", "adaptive", "multistep", "sde")
# (model kind, handle present, B, state dtype, image masks equal across a pair) -> fused? per METHODS
ROUTES = [
    (("foreign", True, 2, bf16, True), (False, False, False, False, False)),
    (("foreign", True, 2, f32, False), (False, False, False, False, False)),
    (("forward", True, 2, bf16, True), (True, True, True, True, True)),
    (("forward", True, 2, f32, True), (True, True, True, True, True)),
    (("forward", True, 2, f16, True), (False, False, False, False, False)),
    (("forward", True, 2, f64, True), (False, False, False, False, False)),
    (("forward", False, 2, bf16, True), (True, False, False, False, False)),
    (("forward_with_cfg", True, 2, bf16, True), (True, True, True, True, True)),
    (("forward_with_cfg", True, 2, bf16, False), (False, False, False, False, False)),
    (("forward_with_cfg", True, 3, bf16, True), (False, False, False, False, False)),
]
CFG = 2.5


@pytest.fixture()
def rig(monkeypatch):
    """-> (model, calls): a tiny Flux whose handle() is `model.stub` (an object, or None), whose forward_with_cfg records its
    cfg_scale, and a transport whose eight runners append (name, args, kwargs) to `calls` instead of running"""
    from visualcloze_amd import transport as T
    from visualcloze_amd.model import Flux, FluxParams
    calls = []
    m = Flux(FluxParams(**TINY))
    m.stub = object()
    monkeypatch.setattr(Flux, "handle", lambda self: self.stub)

    def forward_with_cfg(self, xin, cfg_scale=1.0, **k):
        calls.append(("forward_with_cfg", cfg_scale))
        return torch.zeros(xin.shape[0], xin.shape[1], 64)

    monkeypatch.setattr(Flux, "forward_with_cfg", forward_with_cfg)
    out = torch.zeros(1, 2, 24, 64)
    for name in ("_sample_fused", "_sample_foreign", "_sample_multistep_fused", "_sample_multistep_foreign", "_sample_sde_fused",
                 "_sample_sde_foreign"):
        monkeypatch.setattr(T, name, lambda *a, _n=name, **k: (calls.append((_n, a, k)), out)[1])
    monkeypatch.setattr(T, "_sample_adaptive_fused", lambda *a, **k: (calls.append(("_sample_adaptive_fused", a, k)), (out, [{}]))[1])
    monkeypatch.setattr(T, "_sample_adaptive_foreign", lambda *a, **k: (calls.append(("_sample_adaptive_foreign", a, k)), (out, {}))[1])
    return m, calls


def _call(method, model, x, kw, **over):
    from visualcloze_amd.transport import Sampler, create_transport
    s = Sampler(create_transport())
    if method.startswith("ode_"):
        return s.sample_ode(sampling_method=method[4:], num_steps=3, **over)(x, model, kw)
    if method == "adaptive":
        return s.sample_ode_adaptive(num_steps=3, method="bosh3")(x, model, kw)
    if method == "multistep":
        return s.sample_ode_multistep(order=2, num_steps=3)(x, model, kw)
    return s.sample_sde(sampling_method="Euler", diffusion_form="sigma", num_steps=3)(x, model, **kw)


def _inputs(kind, B, dtype, equal):
    inp = tiny_inputs(B=B)
    kw = {k: inp[k] for k in ("txt", "txt_ids", "txt_mask", "y", "img_ids", "img_mask", "cond", "guidance")}
    if not equal:
        kw["img_mask"] = kw["img_mask"].clone()
        kw["img_mask"][-1, -1] = 0                 # the last sample's last image row: its pair no longer shares the mask
    if kind == "forward_with_cfg":
        kw["cfg_scale"] = CFG
    return inp["x"].to(dtype), kw


RUNNERS = {"ode_euler": "_sample", "ode_rk4": "_sample", "adaptive": "_sample_adaptive", "multistep": "_sample_multistep", "sde": "_sample_sde"}


# where a fused runner takes cfg_scale: a keyword of _sample_fused, a position of the others
CFG_ARG = {"_sample_adaptive_fused": 8, "_sample_multistep_fused": 6, "_sample_sde_fused": 9}


@pytest.mark.parametrize("row,fused", ROUTES, ids=["-".join(str(c).replace("torch.", "") for c in row) for row, _ in ROUTES])
@pytest.mark.parametrize("method", METHODS)
def test_route(rig, method, row, fused):
    m, calls = rig
    kind, has_handle, B, dtype, equal = row
    m.stub = object() if has_handle else None
    x, kw = _inputs(kind, B, dtype, equal)
    model = (lambda xin, **k: xin[..., :64]) if kind == "foreign" else getattr(m, kind)
    given = dict(kw)
    _call(method, model, x, kw)
    assert kw.keys() == given.keys()                                           # the caller's dict is left as it came
    ran = [c for c in calls if c[0].startswith("_sample")]
    want = RUNNERS[method] + ("_fused" if fused[METHODS.index(method)] else "_foreign")
    assert [c[0] for c in ran] == [want], (method, row)
    name, a, k = ran[0]
    passed_kw = next(v for v in a if isinstance(v, dict) and "txt" in v)
    assert "cfg_scale" not in passed_kw and passed_kw.keys() == given.keys() - {"cfg_scale"}
    if name.endswith("_fused"):
        assert a[0] is m
        handed = k.get("cfg_scale") if name == "_sample_fused" else a[CFG_ARG[name]]
        assert handed == (CFG if kind == "forward_with_cfg" else None), (method, row, handed)
    elif kind == "forward_with_cfg":                                           # the eager callable is forward_with_cfg at the popped scale
        a[0](torch.zeros(2, 24, 448), timesteps=torch.ones(2))
        assert calls[-1] == ("forward_with_cfg", CFG)
    elif kind == "foreign":
        assert a[0] is model


def test_cfg_scale_defaults_to_one_and_is_a_float(rig):
    m, calls = rig
    x, kw = _inputs("forward", 2, bf16, True)
    _call("ode_euler", m.forward_with_cfg, x, kw)                              # no "cfg_scale" key: the reference's default
    assert calls[-1][0] == "_sample_fused" and calls[-1][2]["cfg_scale"] == 1.0
    _call("ode_euler", m.forward_with_cfg, x, dict(kw, cfg_scale=3))
    assert calls[-1][2]["cfg_scale"] == 3.0 and isinstance(calls[-1][2]["cfg_scale"], float)
    _call("ode_euler", m.forward, x, kw)
    assert calls[-1][0] == "_sample_fused" and calls[-1][2].get("cfg_scale") is None


def test_step_cache_refusals_of_sample_ode(rig):
    from visualcloze_amd.transport import StepCache
    m, calls = rig
    sc = StepCache(0.1)
    x, kw = _inputs("forward", 2, bf16, True)
    with pytest.raises(TypeError, match=r"^step_cache must be a StepCache or None, got float$"):
        _call("ode_euler", m.forward, x, kw, step_cache=0.1)
    with pytest.raises(ValueError, match=r"^step_cache works with sampling_method='euler' only, not 'rk4'$"):
        _call("ode_rk4", m.forward, x, kw, step_cache=sc)
    with pytest.raises(ValueError, match=r"^step_cache works with Flux\.forward only, not with forward_with_cfg \(true CFG\)$"):
        _call("ode_euler", m.forward_with_cfg, x, dict(kw, cfg_scale=CFG), step_cache=sc)
    m.stub = None
    with pytest.raises(ValueError, match=r"^step_cache needs the C handle: not available with lora_mode='ref' \(unless ref_plan='handle'\) "
                                         r"or the Python-ordered plan \(use_handle False\)$"):
        _call("ode_euler", m.forward, x, kw, step_cache=sc)
    m.stub = object()
    with pytest.raises(ValueError, match=r"^step_cache: a torch\.float16 state is stepped eagerly, where no cache exists$"):
        _call("ode_euler", m.forward, x.to(f16), kw, step_cache=sc)
    with pytest.raises(ValueError, match=r"^step_cache: only the fused loop of a visualcloze_amd\.Flux implements it, not a foreign callable$"):
        _call("ode_euler", lambda xin, **k: xin[..., :64], x, kw, step_cache=sc)
    assert not [c for c in calls if c[0].startswith("_sample")]                # a refused call runs nothing
    # the order a call meets them in: true CFG before everything else about the state; the missing handle before the dtype
    with pytest.raises(ValueError, match="forward_with_cfg"):
        _call("ode_euler", m.forward_with_cfg, x.to(f16), dict(kw, cfg_scale=CFG), step_cache=sc)
    m.stub = None
    with pytest.raises(ValueError, match="needs the C handle"):
        _call("ode_euler", m.forward, x.to(f16), kw, step_cache=sc)
    m.stub = object()
    _call("ode_euler", m.forward, x, kw, step_cache=sc)                        # ... and the one route that takes it
    assert calls[-1][0] == "_sample_fused" and any(v is sc for v in calls[-1][1])
