"""-m gpu: the results do not depend on what the library's memory held before, nor on what masked rows hold.

Every handle works inside buffers whose contents nothing promises (the Python classes allocate them with torch.empty, a C caller
hands over what hipMalloc returned).  DESIGN.md section 9 lists, region by region, who writes each first; this file holds the code to it:

  * every entry point is built and run FROM SCRATCH - model, handle, workspace, arena, argument slots - under
    tests/poison.poisoned_empty(b) for b = 0x00, 0xFF (NaN in bf16 / f32, -1 as int32) and 0x7F (3.39e38, finite); every returned
    tensor and every log is compared with the 0x00 run through integer views, so NaN payloads and the sign of a zero count;
  * stale bytes: a second geometry prepared on the bytes the first one left == a fresh handle on a zeroed buffer;
  * the slack behind vc_*_workspace_bytes keeps the pattern; the block did allocate (the counter), the workspace did hold the pattern
    before prepare, and at 0xFF a never-zeroed region (the split-K scratch, unused at the tiny geometry) still holds it afterwards;
  * the split-K / stream-K GEMM and the attention tail split, which the tiny geometry cannot reach, at op level with their scratch
    poisoned (the attention's flag words stay zero, as include/vcloze_hip.h tells the caller);
  * live rows depend on live inputs only: masked positions of x, cond and txt filled from two seeds, one scaled by 64.

Tiny models (tests/helpers.py, tests/procedural.py): T = 16, N = 96, L = 112, Lp = 128 - 16 pad keys are live in the last tile.
No tolerance anywhere.  True CFG pairs the two halves of a batch, so it runs at B = 2 only."""
import math
import os

import numpy as np
import pytest
import torch

from tests.poison import any_byte, holds, poisoned_empty

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15
BYTES = (0x00, 0xFF, 0x7F)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- plumbing
def bits(t):
    """the bytes of a tensor (or the thing itself where it is no tensor), for comparisons that see NaN payloads and -0"""
    if torch.is_tensor(t):
        return t.detach().contiguous().view(-1).view(torch.uint8).cpu()
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).view(np.uint8).copy()
    if isinstance(t, float):
        return np.float64(t).tobytes()
    if isinstance(t, dict):
        return {k: bits(v) for k, v in t.items()}
    if isinstance(t, (list, tuple)):
        return [bits(v) for v in t]
    return t


def same_bits(a, b) -> bool:
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and bool((a == b).all())
    return a == b


ROWS_HW = ((8, 24), (8, 24))          # two rows of 4 x 12 tokens: N = 96; with T = 16, L = 112 and Lp = 128


def flux_inputs(kind):
    """the inputs of a Flux case on the device: "b1", the ragged "b2" of tests/test_dopri5_gpu.py, or "gap" (holes in both streams of
    sample 0: MaskLayout moves the valid rows first, kv_len + kv_gap)"""
    from tests.procedural import tiny_inputs
    inp = tiny_inputs(B=1, rows_hw=ROWS_HW) if kind == "b1" else tiny_inputs(B=2, rows_hw=ROWS_HW, seed=7)
    assert inp["x"].shape[1] == 96 and inp["txt"].shape[1] == 16
    if kind == "b2":
        inp["img_mask"][1, -12:] = 0
        inp["txt_mask"][0, -5:] = 0
    if kind == "gap":
        inp["txt_mask"][0, [0, 5]] = 0
        inp["img_mask"][0, [1, 2, 9]] = 0
        inp["img_mask"][1, -12:] = 0
    return inp


def on_device(inp):
    B = inp["x"].shape[0]
    args = dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
                y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
                guidance=inp["guidance"].to(DEV))
    cond = inp["cond"].to(DEV, torch.bfloat16)
    return dict(B=B, args=args, kw=dict(args, cond=cond), cond=cond, x=inp["x"].to(DEV, torch.bfloat16), x32=inp["x"].to(DEV, torch.float32),
                img=torch.cat((inp["x"], inp["cond"]), -1).to(DEV, torch.bfloat16), t=torch.tensor([0.7, 0.3][:B], device=DEV),
                t_loss=torch.tensor([0.37, 0.81][:B]))


def _sampler():
    from visualcloze_amd.transport import Sampler, create_transport
    return Sampler(create_transport())


def _ode(method, **over):
    opts = dict(sampling_method=method, num_steps=4, do_shift=True, time_shifting_factor=1, return_trajectory=True)
    opts.update(over)
    return _sampler().sample_ode(**opts)


_SD = {}


def _model(**attrs):
    """tests/helpers.tiny_model, built anew on every call (its parameters and everything behind them are then allocated inside the
    caller's poisoned block); the procedural values are computed once"""
    from tests.procedural import TINY, TINY_RANK, procedural_param
    from visualcloze_amd.model import FluxLoraWrapper, FluxParams
    m = FluxLoraWrapper(lora_rank=TINY_RANK, lora_scale=1.0, params=FluxParams(**TINY))
    if not _SD:
        _SD.update({k: procedural_param(k, v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(_SD, strict=True)
    m = m.eval().to(DEV, torch.bfloat16)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


SDE = {"euler_mean": dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=0.7, last_step="Mean", last_step_size=0.25, num_steps=4),
       "heun_tweedie": dict(sampling_method="Heun", diffusion_form="decreasing", diffusion_norm=0.7, last_step="Tweedie", last_step_size=0.25,
                            num_steps=4)}


# ---------------------------------------------------------------------------------------------- the Flux cases: I -> (model, results)
def case_forward(I):
    m = _model()
    return m, {"out": m(I["img"], timesteps=I["t"], **I["args"])}


def case_forward_twin(I):
    m = _model(lora_mode="ref", ref_plan="python")          # the Python-ordered plan: engine.py's buffers are torch.empty too
    return m, {"out": m(I["img"], timesteps=I["t"], **I["args"])}


def _solver_case(method, f32):
    def case(I):
        m = _model()
        return m, {"traj": _ode(method)(I["x32"] if f32 else I["x"], m.forward, I["kw"])}
    return case


def case_cfg(I):
    m = _model()
    kw = dict(I["kw"], cfg_scale=2.5)
    return m, {"forward_with_cfg": m.forward_with_cfg(I["img"], timesteps=I["t"], cfg_scale=2.5, **I["args"]),
               "euler": _ode("euler")(I["x"], m.forward_with_cfg, kw), "rk4_f32": _ode("rk4")(I["x32"], m.forward_with_cfg, kw)}


def _adaptive_case(method):
    def case(I):
        m = _model()
        s = _sampler()
        out = s.sample_ode_adaptive(num_steps=4, rtol=1e-2, atol=1e-6, do_shift=True, time_shifting_factor=1, return_trajectory=True,
                                    method=method)(I["x32"], m.forward, I["kw"])
        torch.cuda.synchronize()
        logs = [{"attempts": [list(a) for a in lg["attempts"]], "evaluations": lg["evaluations"], "rejected": lg["rejected"]}
                for lg in s.last_adaptive_log]
        assert logs and all(lg["attempts"] for lg in logs)
        return m, {"traj": out, "log": logs}
    return case


def _sde_case(setting):
    def case(I):
        from visualcloze_amd.pipeline import NoiseStream
        m = _model()
        rng = NoiseStream(SEED, 1003, device=DEV)
        out = _sampler().sample_sde(rng=rng, return_trajectory=True, **SDE[setting])(I["x32"], m.forward, **I["kw"])
        return m, {"traj": out, "offset": rng.offset}
    return case


def case_loss(I):
    from visualcloze_amd import transport as T
    from visualcloze_amd.pipeline import NoiseStream
    m = _model()
    res = {}
    for name, x1 in (("bf16", I["x"]), ("f32", I["x32"])):
        rng = NoiseStream(SEED, 1003, device=DEV)
        got = T.create_transport().training_losses(m.forward, x1, I["args"], {"cond": I["cond"]}, t=I["t_loss"], rng=rng)
        res[name] = {k: v for k, v in got.items() if torch.is_tensor(v)}
        res[name + "_offset"] = rng.offset
        assert res[name]["loss"].shape == (I["B"],)
    return m, res


def case_step_cache(I):
    from visualcloze_amd.transport import StepCache
    m = _model()
    s = _sampler()
    out = s.sample_ode(sampling_method="euler", num_steps=6, do_shift=True, time_shifting_factor=1, return_trajectory=True,
                       step_cache=StepCache(math.inf, 1))(I["x"], m.forward, I["kw"])
    torch.cuda.synchronize()
    stats = [dict(st) for st in s.last_step_cache_stats]
    assert all(st["reused"] >= 1 and st["computed"] >= 2 for st in stats), stats       # some evaluations reused, some computed
    return m, {"traj": out, "stats": stats}


def case_lora_taps(I):
    m = _model(lora_mode="ref", ref_plan="handle")
    taps = m.block_taps(I["img"], timesteps=I["t"], **I["args"])
    assert "single.1" in taps and "out" in taps
    return m, {"taps": taps, "euler": _ode("euler")(I["x"], m.forward, I["kw"])}


def case_monitor(I):
    m = _model(monitor=2)
    out = _ode("midpoint")(I["x"], m.forward, I["kw"])
    torch.cuda.synchronize()
    logs = m.last_monitor_log
    assert logs and "single.1" in logs[0] and logs[0]["v"]["count"].shape[0] == 6      # 3 steps of 2 evaluations, every row written
    fwd = m(I["img"], timesteps=I["t"], **I["args"])
    return m, {"traj": out, "log": logs, "report": m.last_monitor_report, "forward": fwd, "forward_log": m.last_monitor_log}


def case_load_in_library(I):
    m = _model(load_in_library=True)
    out = m(I["img"], timesteps=I["t"], **I["args"])
    h = m.handle()
    assert getattr(h, "_loaded", None) and m._engine is None
    return m, {"out": out, "euler": _ode("euler", num_steps=3)(I["x"], m.forward, I["kw"])}


def case_from_state_dict(I):
    """FluxHandle.from_state_dict driven directly, then one vc_flux_forward: the arena holds every bound weight"""
    from visualcloze_amd.handle import FluxHandle
    m = _model()
    h = FluxHandle.from_state_dict(m.params, m.state_dict(), 1.0, torch.device(DEV))
    a = I["args"]
    B, N = I["img"].shape[:2]
    assert not a["txt_mask"].eq(0).any() and not a["img_mask"].eq(0).any()
    h.prepare(a["txt"], a["y"], a["guidance"], False, a["img_ids"], a["txt_ids"], 1)
    out = torch.empty(B, N, m.out_channels, dtype=torch.bfloat16, device=DEV)
    h.forward(I["img"], I["t"], False, out)
    torch.cuda.synchronize()
    m._handle = h                                           # so that the checks below look at this handle
    return m, {"out": out, "modulation_bias": h.W.mod_b.clone()}


FLUX_CASES = {
    "forward": case_forward, "forward_twin": case_forward_twin,
    **{f"{meth}_{'f32' if f32 else 'bf16'}": _solver_case(meth, f32) for meth in ("euler", "midpoint", "rk4") for f32 in (False, True)},
    "dopri5": _adaptive_case("dopri5"), "bosh3": _adaptive_case("bosh3"),
    "sde_euler_mean": _sde_case("euler_mean"), "sde_heun_tweedie": _sde_case("heun_tweedie"),
    "loss": case_loss, "step_cache": case_step_cache, "lora_taps": case_lora_taps, "monitor": case_monitor,
    "load_in_library": case_load_in_library,
}


@pytest.fixture(scope="module")
def inputs():
    """the case inputs, made once outside every poisoned block and never written"""
    return {k: on_device(flux_inputs(k)) for k in ("b1", "b2", "gap")}


class Watch:
    """_Handle._aligned sees every workspace, arena and grid buffer right before the library is handed it: the first time a tensor
    comes by it must still hold the pattern, whole"""

    def __init__(self, byte, monkeypatch):
        from visualcloze_amd.handle import _Handle
        self.byte, self.seen, self.keep = byte, 0, []
        orig = _Handle._aligned

        def aligned(ws):
            if not any(ws is t for t in self.keep):
                assert holds(ws, byte), f"a workspace of {ws.numel()} bytes does not hold 0x{byte:02X} before the library prepares in it"
                self.keep.append(ws)
                self.seen += 1
            return orig(ws)
        monkeypatch.setattr(_Handle, "_aligned", staticmethod(aligned))


def slack_holds(h, ws, byte) -> bool:
    """the class allocates vc_*_workspace_bytes + 256: what lies behind aligned base + those bytes is nobody's"""
    base, _ = h._aligned(ws)
    off = base - ws.data_ptr() + ws.numel() - 256
    return off < ws.numel() and holds(ws[off:], byte)


def flux_checks(m, byte, what):
    h = m._handle
    if h is None:
        return
    tensors = list(h._ws.values()) + ([h._arena] if getattr(h, "_arena", None) is not None else [])
    assert tensors, what
    for ws in tensors:
        assert slack_holds(h, ws, byte), f"{what}: the bytes behind the workspace's end were written"
    if byte == 0xFF:      # written before read, never zeroed - and at this geometry no GEMM takes a split: the pattern is still there
        assert any_byte(h._sk_ws, 0xFF), f"{what}: the split-K scratch holds no 0xFF any more - was the block poisoned at all?"


def run_flux(name, I, byte, monkeypatch):
    with monkeypatch.context() as mp, poisoned_empty(byte, mp) as p:
        w = Watch(byte, mp)
        m, res = FLUX_CASES[name](I) if name in FLUX_CASES else name(I)
        torch.cuda.synchronize()
        assert p.count > 0
        if m._handle is not None:
            assert w.seen > 0, "no workspace went by"
        flux_checks(m, byte, f"{name} 0x{byte:02X}")
        return bits(res)


# ---------------------------------------------------------------------------------------------- 3. the cases
@pytest.mark.parametrize("kind", ["b1", "b2"])
@pytest.mark.parametrize("name", sorted(FLUX_CASES))
def test_flux_results_do_not_depend_on_the_workspace_contents(inputs, monkeypatch, name, kind):
    I = inputs[kind]
    want = run_flux(name, I, 0x00, monkeypatch)
    for byte in BYTES[1:]:
        got = run_flux(name, I, byte, monkeypatch)
        diff = [k for k in want if not same_bits(want[k], got[k])]
        assert not diff, f"{name} {kind}: {diff} differ between a workspace of 0x00 and of 0x{byte:02X}"


def test_true_cfg_results_do_not_depend_on_the_workspace_contents(inputs, monkeypatch):
    want = run_flux(case_cfg, inputs["b2"], 0x00, monkeypatch)
    for byte in BYTES[1:]:
        got = run_flux(case_cfg, inputs["b2"], byte, monkeypatch)
        assert not [k for k in want if not same_bits(want[k], got[k])], f"0x{byte:02X}"


def test_from_state_dict_arena_contents_do_not_matter(inputs, monkeypatch):
    want = run_flux(case_from_state_dict, inputs["b1"], 0x00, monkeypatch)
    for byte in BYTES[1:]:
        got = run_flux(case_from_state_dict, inputs["b1"], byte, monkeypatch)
        assert not [k for k in want if not same_bits(want[k], got[k])], f"0x{byte:02X}"


# ---- VAE
def _ae(cfg):
    from tests.procedural import procedural_ae_param
    from visualcloze_amd.vae import AutoEncoder, AutoEncoderParams
    m = AutoEncoder(AutoEncoderParams(**cfg))
    m.load_state_dict({k: procedural_ae_param(k, v.shape) for k, v in m.state_dict().items()})
    return m.to(DEV).to(torch.bfloat16)


VAE_SIZES = ((4, 4), (6, 10))          # latent (h, w) of tests/test_vae_handle_gpu.py: 16 and 60 attention tokens (zero pads live)


@pytest.fixture(scope="module")
def vae_inputs():
    from tests.procedural import TINY_AE, ptensor
    F, Z = 2 ** (len(TINY_AE["ch_mult"]) - 1), TINY_AE["z_channels"]
    return [dict(z=ptensor((Z, h, w), 71 + i, q=5, kmax=96).to(DEV, torch.bfloat16),
                 img=ptensor((3, F * h, F * w), 75 + i, q=7, kmax=127).to(DEV, torch.bfloat16),
                 noise=ptensor((Z, h, w), 79 + i, q=5, kmax=80).to(DEV, torch.bfloat16)) for i, (h, w) in enumerate(VAE_SIZES)]


def run_vae(V, byte, monkeypatch):
    from tests.procedural import TINY_AE
    from visualcloze_amd.handle import VaeHandle
    with monkeypatch.context() as mp, poisoned_empty(byte, mp) as p:
        w = Watch(byte, mp)
        h = VaeHandle(_ae(TINY_AE))
        res = {}
        for rnd in range(2):                                # two image sizes alternating
            for i, v in enumerate(V):
                res[f"enc{i}.{rnd}"] = h.encode(v["img"], noise=v["noise"])
                res[f"dec{i}.{rnd}"] = h.decode(v["z"])
        res["dec_f32"] = h.decode(V[1]["z"].float(), pixels_f32=True)
        torch.cuda.synchronize()
        assert p.count > 0 and w.seen >= 4 and len(h._ws) >= 1
        for ws in h._ws.values():
            assert slack_holds(h, ws, byte), f"vae 0x{byte:02X}: the bytes behind the workspace's end were written"
        return bits(res)


def test_vae_results_do_not_depend_on_the_workspace_contents(vae_inputs, monkeypatch):
    want = run_vae(vae_inputs, 0x00, monkeypatch)
    assert same_bits(want["enc1.0"], want["enc1.1"]) and same_bits(want["dec0.0"], want["dec0.1"])
    for byte in BYTES[1:]:
        got = run_vae(vae_inputs, byte, monkeypatch)
        assert not [k for k in want if not same_bits(want[k], got[k])], f"0x{byte:02X}"


# ---- text
def _t5(cfg):
    from tests.procedural import procedural_text_param
    from visualcloze_amd.text import T5Config, T5EncoderModel
    m = T5EncoderModel(T5Config(**cfg))
    sd = {k: procedural_text_param(k, v.shape) for k, v in m.state_dict().items()}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    m.load_state_dict(sd)
    return m.to(DEV).to(torch.bfloat16)


def _clip(cfg):
    from tests.procedural import procedural_text_param
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel
    m = CLIPTextModel(CLIPTextConfig(**cfg))
    m.load_state_dict({k: procedural_text_param(k, v.shape) for k, v in m.state_dict().items()})
    return m.to(DEV).to(torch.bfloat16)


@pytest.fixture(scope="module")
def text_inputs():
    from tests.procedural import TINY_CLIP, TINY_T5, tiny_ids
    eos = TINY_CLIP["eos_token_id"]
    return {"t5": [torch.stack([tiny_ids(L, TINY_T5["vocab_size"], seed=31 + i) for i in range(2)]).to(DEV) for L in (64, 128)],
            "clip": [torch.stack([tiny_ids(L, TINY_CLIP["vocab_size"], seed=41 + i, eos=eos, eos_at=at - i) for i in range(2)]).to(DEV)
                     for L, at in ((8, 6), (23, 9))]}


def run_text(kind, ids, byte, monkeypatch):
    from tests.procedural import TINY_CLIP, TINY_T5
    from visualcloze_amd.handle import TextHandle
    with monkeypatch.context() as mp, poisoned_empty(byte, mp) as p:
        w = Watch(byte, mp)
        h = TextHandle(_t5(TINY_T5) if kind == "t5" else _clip(TINY_CLIP))
        res = {}
        for rnd in range(2):                                # two lengths alternating: CLIP 8 and 23 (off 64: its rows are padded to
            #                                                     64), T5 64 and 128 (vc_text_* takes multiples of 64 only for T5)
            for i in ids:
                hidden, pooled = h.encode(i)
                res[f"hidden{i.shape[1]}.{rnd}"] = hidden
                if pooled is not None:
                    res[f"pooled{i.shape[1]}.{rnd}"] = pooled
        torch.cuda.synchronize()
        assert p.count > 0 and w.seen == 2 and len(h._ws) == 2
        for ws in h._ws.values():
            assert slack_holds(h, ws, byte), f"{kind} 0x{byte:02X}: the bytes behind the workspace's end were written"
        return bits(res)


@pytest.mark.parametrize("kind", ["t5", "clip"])
def test_text_results_do_not_depend_on_the_workspace_contents(text_inputs, monkeypatch, kind):
    want = run_text(kind, text_inputs[kind], 0x00, monkeypatch)
    assert ("pooled8.0" in want) == (kind == "clip")
    for byte in BYTES[1:]:
        got = run_text(kind, text_inputs[kind], byte, monkeypatch)
        assert not [k for k in want if not same_bits(want[k], got[k])], f"0x{byte:02X}"


# ---- grid
GRID_AE = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 1, 1, 1], num_res_blocks=1, z_channels=16,
               scale_factor=0.3611, shift_factor=0.1159)                      # 8x down, as tests/test_grid_handle_gpu.py
GRID_ROWS = [(32, 64), (32, 48)]


@pytest.fixture(scope="module")
def grid_inputs():
    from tests.procedural import ptensor, tiny_ids
    c = lambda t: t.to(DEV, torch.bfloat16)  # noqa: E731
    g = np.load(os.path.join(REPO, "tests", "golden", "resample_golden.npz"))
    a, b = (torch.from_numpy(g[f"photo_{j}"]).to(DEV) for j in range(2))
    return dict(rows=[c(ptensor((3, H, W), 301 + i, q=7)) for i, (H, W) in enumerate(GRID_ROWS)],
                masks=[c(torch.zeros(1, 1, *GRID_ROWS[0])),
                       c(torch.cat((torch.zeros(1, 1, 32, 16), torch.ones(1, 1, 32, 16), torch.zeros(1, 1, 32, 16)), -1))],
                cells=[c(ptensor((3, 32, 32), 311 + i, q=7)) for i in range(2)], photos=[[a, b], [b, None]],
                up_cell=torch.from_numpy(g["up_cell"]).to(DEV),
                t5_ids=tiny_ids(64, 128, seed=5)[None].to(DEV), clip_ids=tiny_ids(16, 128, seed=6, eos=127, eos_at=7)[None].to(DEV))


def run_grid(D, byte, monkeypatch):
    from tests.procedural import TINY, TINY_T5
    from visualcloze_amd.handle import GridHandle
    cl = dict(vocab_size=128, hidden_size=TINY["vec_in_dim"], intermediate_size=128, num_hidden_layers=1, num_attention_heads=1,
              max_position_embeddings=16, layer_norm_eps=1e-5, eos_token_id=127)
    with monkeypatch.context() as mp, poisoned_empty(byte, mp) as p:
        w = Watch(byte, mp)
        m, ae, t5, clip = _model(), _ae(GRID_AE), _t5(TINY_T5), _clip(cl)
        ae.use_handle = t5.use_handle = clip.use_handle = True
        gh = GridHandle(m, ae, t5, clip)
        ids = (D["t5_ids"], D["clip_ids"])
        res = {}
        res["generate"], res["generate_off"] = gh.generate(D["rows"], D["masks"], *ids, 11, 5, cfg=30.0, steps=4)
        res["sdedit"], res["sdedit_off"] = gh.sdedit(D["cells"], *ids, 11, 3, cfg=30.0, steps=3, strength=0.4)
        res["photos"], res["photos_off"] = gh.generate_photos(D["photos"], 32, *ids, 11, 5, cfg=30.0, steps=4, uint8=True)
        res["sdedit_u8"], res["sdedit_u8_off"] = gh.sdedit_u8([D["up_cell"]], (48, 32), *ids, 11, 3, cfg=30.0, steps=3, strength=0.4)
        res["generate_rk4"], _ = gh.generate(D["rows"], D["masks"], *ids, 11, 5, cfg=30.0, steps=4, solver="rk4")
        torch.cuda.synchronize()
        assert p.count > 0 and w.seen >= 1 and gh._ws is not None
        return bits(res)


def test_grid_results_do_not_depend_on_the_workspace_contents(grid_inputs, monkeypatch):
    want = run_grid(grid_inputs, 0x00, monkeypatch)
    for byte in BYTES[1:]:
        got = run_grid(grid_inputs, byte, monkeypatch)
        assert not [k for k in want if not same_bits(want[k], got[k])], f"0x{byte:02X}"


# ---------------------------------------------------------------------------------------------- stale bytes
def test_flux_second_geometry_on_the_bytes_of_the_first(inputs):
    """B = 2 ragged, then B = 1 with T = 24 prepared on the same bytes == a fresh handle on a zeroed buffer"""
    from tests.procedural import tiny_inputs
    first, second = inputs["b2"], on_device(tiny_inputs(B=1, rows_hw=ROWS_HW, T=24, seed=3))
    keys = [(2, 16, 96, 1, False), (1, 24, 96, 1, False)]

    def handle_on(fill):
        m = _model()
        h = m.handle()
        need = max(h.workspace(*k[:4]).numel() for k in keys)             # (each the library's bytes + 256)
        assert list(h._ws) == keys
        buf = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        for k in keys:
            h._ws[k] = buf
        return m, h, buf

    m, h, stale = handle_on(0x7F)
    a = m(first["img"], timesteps=first["t"], **first["args"])
    assert h.geom[:3] == (2, 16, 96) and h._keep[2] is stale
    got = m(second["img"], timesteps=second["t"], **second["args"])
    assert h.geom[:3] == (1, 24, 96) and h._keep[2] is stale and len(h._ws) == 2
    m2, h2, zeroed = handle_on(0x00)
    want = m2(second["img"], timesteps=second["t"], **second["args"])
    assert h2._keep[2] is zeroed
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and same_bits(bits(got), bits(want))


def test_vae_second_size_on_the_bytes_of_the_first(vae_inputs):
    from tests.procedural import TINY_AE
    from visualcloze_amd import hip
    from visualcloze_amd.handle import VaeHandle
    ae = _ae(TINY_AE)
    F = 2 ** (len(TINY_AE["ch_mult"]) - 1)
    keys = [(F * h, F * w, hip.VAE_DECODER) for h, w in VAE_SIZES]

    def handle_on(fill):
        h = VaeHandle(ae)
        buf = torch.full((max(h.workspace_bytes(*k) for k in keys) + 256,), fill, dtype=torch.uint8, device=DEV)
        for k in keys:
            h._ws[k] = buf
        return h, buf

    h, stale = handle_on(0x7F)
    a = h.decode(vae_inputs[0]["z"])
    got = h.decode(vae_inputs[1]["z"])
    assert len(h._ws) == 2 and all(t is stale for t in h._ws.values())
    want = handle_on(0x00)[0].decode(vae_inputs[1]["z"])
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and same_bits(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------- routes beyond the tiny geometry
def _poisoned_bytes(n, byte, keep_zero_from=None):
    t = torch.zeros(n, dtype=torch.uint8, device=DEV)
    t[:n if keep_zero_from is None else keep_zero_from] = byte
    return t


@pytest.mark.parametrize("route", ["splitk2", "splitk3", "streamk"])
def test_gemm_split_routes_do_not_read_the_scratch_before_writing_it(route):
    """(257, 264, 320) of tests/test_hotpath_gpu.py: every tile a remainder tile, f32 partials through splitk_ws"""
    from tests.helpers import gemm_plan_answer
    from visualcloze_amd import hip
    hip.require_gpu()
    M, N, K = 257, 264, 320
    S = {"splitk2": 2, "splitk3": 3}.get(route)
    cfg = hip.GEMM_STREAMK if S is None else hip.GEMM_SPLITK(S)
    g = torch.Generator().manual_seed(M)
    a = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV, torch.bfloat16)
    b = torch.randn(N, generator=g).to(DEV, torch.bfloat16)
    outs = []
    for byte in BYTES:
        ws = _poisoned_bytes(hip.GEMM_SPLITK_WS_BYTES, byte)
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        p = hip.make_problem(a, w, b, out)
        args = hip.GemmArgs()
        args.nprob, args.epi, args.p[0] = 1, hip.EPI_GELU, p
        args.splitk_ws, args.splitk_ws_bytes = ws.data_ptr(), ws.numel()
        plan = gemm_plan_answer(hip.lib(), args, cfg)
        assert len(plan) == 8 and plan[7] > 0 and (plan[6] == S if S else plan[6] < 0), f"{route}: the plan {plan} takes no split"
        hip.gemm(p, epi=hip.EPI_GELU, tile_cfg=cfg, splitk_ws=ws)
        torch.cuda.synchronize()
        if byte:
            assert not holds(ws, byte), "the route wrote no partial tile"
        outs.append(bits(out))
    assert torch.isfinite(outs[0].view(torch.bfloat16).float()).all()
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])


def _tail_plan(hip, L, H, variant, prescaled):
    a = hip.Attention()
    a.qkv = a.vt = a.out = a.scratch = 0x1000                              # never dereferenced by the planner
    a.B, a.L, a.Lpad, a.H, a.variant = 1, L, (L + 63) // 64 * 64, H, variant
    a.ld, a.bstride, a.ldo, a.out_bstride = 3 * H * 128, L * 3 * H * 128, H * 128, L * H * 128
    a.scratch_bytes = hip.lib().vc_attention_scratch_bytes()
    a.q_prescaled, a.logit_bound = int(prescaled), 0.0
    return hip.attention_plan(a)


@pytest.mark.parametrize("variant", [7, 12, 28])
def test_attention_tail_split_does_not_read_the_partials_before_writing_them(variant):
    """the all_tail schedule (tests/attn_schedule.py, tests/test_hotpath_gpu.py): H = 24, the smallest L at which every item is a tail
    item.  The partials of the scratch are poisoned; the flag words behind them stay zero, as vc_attention's header requires."""
    from visualcloze_amd import hip
    hip.require_gpu()
    H, pre = 24, variant != 7
    L = next(L for L in range(65, 4000) if (lambda p: p[8] >= 0 and p[9] > 0)(_tail_plan(hip, L, H, variant, pre)))
    plan = _tail_plan(hip, L, H, variant, pre)
    assert plan[8] == 0 and plan[9] == plan[7] > 0 and plan[14] > 0, plan       # split, every item a tail item, the scratch is used
    flags = plan[13]
    n = hip.lib().vc_attention_scratch_bytes()
    assert 0 < flags < n
    g = torch.Generator().manual_seed(L)
    x = torch.randn(L, 3, H, 128, generator=g)
    x[:, :2] = x[:, :2] / x[:, :2].pow(2).mean(-1, keepdim=True).sqrt()
    qkv = x.reshape(L, 3 * H * 128).to(torch.bfloat16)
    if pre:
        qkv[:, :H * 128] = (qkv[:, :H * 128].float() * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)
    qd = qkv.to(DEV)
    vt = torch.zeros(1, H, 128, (L + 63) // 64 * 64, dtype=torch.bfloat16, device=DEV)
    vt[0, :, :, :L] = qd[:, 2 * H * 128:].reshape(L, H, 128).permute(1, 2, 0)
    outs = []
    for byte in BYTES:
        scratch = _poisoned_bytes(n, byte, keep_zero_from=flags)
        out = torch.full((L, H * 128), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.attention(qd, vt, out, L, H, variant=variant, q_prescaled=pre, scratch=scratch)
        torch.cuda.synchronize()
        assert not scratch[flags:].any(), "every launch leaves the flag words zero"
        if byte:
            assert not holds(scratch[:flags], byte), "the split wrote no partial"
        outs.append(bits(out))
    assert torch.isfinite(outs[0].view(torch.bfloat16).float()).all()
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])


# ---------------------------------------------------------------------------------------------- 4. live rows, live inputs
def _refill_masked(I, inp, seed, scale):
    """the masked positions of x, cond and txt <- ordinary finite values of `seed` times `scale`; the live ones untouched"""
    g = torch.Generator().manual_seed(seed)
    im, tm = inp["img_mask"].eq(0), inp["txt_mask"].eq(0)
    assert im.any() and tm.any()
    x, cond, txt = inp["x"].clone(), inp["cond"].clone(), inp["txt"].clone()
    x[im] = (torch.randn(int(im.sum()), x.shape[-1], generator=g) * scale).to(torch.bfloat16).float()
    cond[im] = (torch.randn(int(im.sum()), cond.shape[-1], generator=g) * scale).to(torch.bfloat16).float()
    txt[tm] = (torch.randn(int(tm.sum()), txt.shape[-1], generator=g) * scale).to(torch.bfloat16).float()
    J = on_device(dict(inp, x=x, cond=cond, txt=txt))
    live = inp["img_mask"].ne(0)
    assert torch.equal(J["x"][live.to(DEV)], I["x"][live.to(DEV)]) and not torch.equal(J["x"], I["x"])
    return J


def _live_results(m, J):
    from visualcloze_amd import transport as T
    from visualcloze_amd.pipeline import NoiseStream
    kw = J["kw"]
    res = {"forward": m(J["img"], timesteps=J["t"], **J["args"]),
           "forward_with_cfg": m.forward_with_cfg(J["img"], timesteps=J["t"], cfg_scale=2.5, **J["args"])}
    for meth in ("euler", "midpoint", "rk4"):
        res[meth + "_bf16"] = _ode(meth)(J["x"], m.forward, kw).transpose(0, 1)          # [B, S, N, C]: the mask indexes B, then N
        res[meth + "_f32"] = _ode(meth)(J["x32"], m.forward, kw).transpose(0, 1)
    # a true-CFG trajectory: the combine hands row n of the unconditional sample to row n of the conditional one whatever their masks
    # say (the reference's forward_with_cfg does), so where the two halves' masks differ a masked row reaches a live STATE row after one
    # step and, through that live key, every row after two: the property is the first step's, at rows live in both halves
    res["cfg_euler_step0"] = _ode("euler")(J["x"], m.forward_with_cfg, dict(kw, cfg_scale=2.5)).transpose(0, 1)[:, :1]
    for name, opts in SDE.items():
        res["sde_" + name] = _sampler().sample_sde(rng=NoiseStream(SEED, 1003, device=DEV), return_trajectory=True, **opts)(
            J["x32"], m.forward, **kw).transpose(0, 1)
    loss = T.create_transport().training_losses(m.forward, J["x32"], J["args"], {"cond": J["cond"]}, t=J["t_loss"],
                                                rng=NoiseStream(SEED, 1003, device=DEV))
    torch.cuda.synchronize()
    return res, loss["loss"]


@pytest.mark.parametrize("kind", ["b2", "gap"])
def test_live_rows_depend_on_live_inputs_only(inputs, kind):
    """NaN in a masked row is not part of the property (the reference's own masked softmax turns 0 * NaN into NaN); large finite
    values are.  The adaptive solvers' error norm and the step cache's metric sum over every row, masked ones included
    (rk_embedded.hip, step_cache.hip take no mask), so those two are not asserted here."""
    inp = flux_inputs(kind)
    I = inputs[kind]
    m = _model()
    live = inp["img_mask"].ne(0).to(DEV)
    runs = [_live_results(m, _refill_masked(I, inp, seed, scale)) for seed, scale in ((101, 1.0), (202, 64.0))]
    (a, la), (b, lb) = runs
    for k in a:
        # true CFG combines row n of the conditional sample with row n of the unconditional one: live there = live in both halves
        lv = (live[:1] & live[1:]).expand_as(live) if "cfg" in k else live
        ra, rb = (r[k].movedim(-2, 1)[lv] for r in (a, b))                   # [B, N, ...] -> the live rows
        assert ra.numel() > 0 and torch.isfinite(ra.float()).all(), k
        assert same_bits(bits(ra), bits(rb)), f"{kind}: the live rows of {k} moved with the masked inputs"
    assert same_bits(bits(la), bits(lb)), f"{kind}: the loss moved with the masked inputs: {la.tolist()} vs {lb.tolist()}"
    masked = ~live
    assert not same_bits(bits(a["forward"][masked]), bits(b["forward"][masked]))      # the masked rows did differ: the inputs reached the kernels
