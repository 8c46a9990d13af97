"""GPU: a checkpoint as stored behind the Flux handle (vc_lora_merge_qkv, vc_flux_load_*, csrc/lora_merge.hip, csrc/flux_load.hip).
Everything here is BIT equality: the library's preparation against Flux.prepare() with lora_merge="hip" (the same merge kernel, then
torch indexing / stacking / casts), the loaded handle's forward and Euler trajectory against model.handle()'s, and the C99 host
program against the same calls from Python."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from tests.procedural import TINY

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANK, SCALE = 16, 0.75


# ---------------------------------------------------------------- 1. the kernels
def _operands(O, I, R, f32, ld_extra=0, bias=True, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * O + 10 * I + R + seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    W = (r(O, I + ld_extra) * 0.05).to(DEV, torch.float32 if f32 else torch.bfloat16)[:, :I]
    A = B = bB = b = None
    if R:
        A = (r(R, I + ld_extra) * 0.1).to(DEV, torch.bfloat16)[:, :I]
        B = (r(O, R + ld_extra) * 0.1).to(DEV, torch.bfloat16)[:, :R]
    if bias:
        b = (r(O) * 0.05).to(DEV, torch.float32 if f32 else torch.bfloat16)
        bB = (r(O) * 0.02).to(DEV, torch.bfloat16) if R else None
    return W, A, B, b, bB


def _both(O, I, R, f32, H, ld_extra=0, bias=True):
    from visualcloze_amd import hip
    W, A, B, b, bB = _operands(O, I, R, f32, ld_extra, bias)
    out_ld = lambda: torch.full((O, I + ld_extra), 7.0, dtype=torch.bfloat16, device=DEV)[:, :I]  # noqa: E731
    ref, ref_b = hip.lora_merge(W, A, B, SCALE, out=out_ld(), bias=b, lora_b_bias=bB)
    got, got_b = hip.lora_merge(W, A, B, SCALE, out=out_ld(), bias=b, lora_b_bias=bB, qkv_heads=H)
    torch.cuda.synchronize()
    return ref, ref_b, got, got_b


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("R", [0, 16, 64, 200])
@pytest.mark.parametrize("O", [768, 768 + 1024], ids=["qkv", "linear1"])
def test_merge_qkv_is_merge_then_row_permutation(O, R, f32):
    from visualcloze_amd import hip
    H, D, I = 2, 256, 256
    perm = hip.qkv_head_permutation(H).to(DEV)
    for ld_extra, bias in ((0, True), (8, False), (24, True)):         # dense rows; row strides larger than the width
        ref, ref_b, got, got_b = _both(O, I, R, f32, H, ld_extra, bias)
        want = ref.clone()
        want[:3 * D] = ref[:3 * D][perm]
        assert torch.equal(got, want) and not torch.equal(got, ref)
        assert (got_b is None) == (not bias)
        if bias:
            want_b = ref_b.clone()
            want_b[:3 * D] = ref_b[:3 * D][perm]
            assert torch.equal(got_b, want_b)


@pytest.mark.parametrize("R", [0, 16])
def test_merge_qkv_elementwise_path_and_heads_zero(R):
    from visualcloze_amd import hip
    H, D = 2, 256
    perm = hip.qkv_head_permutation(H).to(DEV)
    ref, ref_b, got, got_b = _both(768 + 40, 12, R, False, H)          # in_features 12: no 16-byte access anywhere
    want, want_b = ref.clone(), ref_b.clone()
    want[:3 * D], want_b[:3 * D] = ref[:3 * D][perm], ref_b[:3 * D][perm]
    assert torch.equal(got, want) and torch.equal(got_b, want_b)
    # qkv_heads = 0 IS vc_lora_merge, in-place form included
    L = hip.lib()
    W, A, B, b, bB = _operands(768, 256, R, False)
    ref, ref_b = hip.lora_merge(W, A, B, SCALE, bias=b, lora_b_bias=bB)
    out, out_b = W.clone(), torch.empty_like(ref_b)
    args = (out.data_ptr(), 0, 256, hip._p(A), 256 if R else 0, hip._p(B), R, SCALE, out.data_ptr(), 256, b.data_ptr(), 0, hip._p(bB),
            out_b.data_ptr(), 768, 256, R)
    hip._check(L.vc_lora_merge_qkv(*args, 0, hip.cur_stream()), "vc_lora_merge_qkv")
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(out_b, ref_b)
    # with heads: no in-place form, no short matrix - refused before anything runs
    assert L.vc_lora_merge_qkv(*args, H, hip.cur_stream()) == -1 and b"overlaps weight" in L.vc_last_error()
    other = torch.empty_like(out)
    short = args[:8] + (other.data_ptr(),) + args[9:14] + (767,) + args[15:]
    assert L.vc_lora_merge_qkv(*short, H, hip.cur_stream()) == -1 and b"out_features" in L.vc_last_error()


# ---------------------------------------------------------------- the model both routes prepare
def make_model(f32=False, scale=SCALE, key_scale_factor=None):
    from visualcloze_amd.model import FluxLoraWrapper, FluxParams, Linear
    torch.manual_seed(5)
    m = FluxLoraWrapper(RANK, scale, FluxParams(**TINY))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".lora_B." in n:
                p.uniform_(-0.05, 0.05)
            elif n.endswith("norm.scale"):
                p.uniform_(0.8, 1.2)
        if key_scale_factor:
            m.single_blocks[1].norm.key_norm.scale.mul_(key_scale_factor)
    m.txt_in.rank = 0                       # one Linear without a pair
    del m.txt_in.lora_A, m.txt_in.lora_B
    m = m.to(DEV, torch.float32 if f32 else torch.bfloat16)
    if f32:                                 # base weights, biases and scales f32; the factors bf16 (vc_lora_merge's rule)
        for mod in m.modules():
            if isinstance(mod, Linear) and mod.rank:
                mod.lora_A.to(torch.bfloat16)
                mod.lora_B.to(torch.bfloat16)
    m.lora_merge = "hip"
    return m


def load(m, scale=SCALE):
    from visualcloze_amd.handle import FluxHandle
    return FluxHandle.from_state_dict(m.params, m.state_dict(), scale, torch.device(DEV))


@pytest.fixture(scope="module")
def pair():
    m = make_model()
    return m, load(m)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_loaded_set_equals_prepare_bitwise(pair, f32):
    m, h = pair if not f32 else (lambda mm: (mm, load(mm)))(make_model(f32=True))
    sd = m.state_dict()
    assert "txt_in.lora_A.weight" not in sd and "img_in.lora_A.weight" in sd
    assert (sd["img_in.weight"].dtype == torch.float32) == f32 and sd["img_in.lora_A.weight"].dtype == torch.bfloat16
    W = m.prepare().W
    torch.cuda.synchronize()
    assert W.qkv_heads == h.W.qkv_heads == 2 and W.mod_off == h.W.mod_off and W.n_mod == h.W.n_mod
    assert set(W.w) == set(h.W.w) and set(W.b) == set(h.W.b)
    for name, t in W.w.items():
        assert h.W.w[name].shape == t.shape and torch.equal(h.W.w[name], t), name
    for name, t in W.b.items():
        assert (t is None) == (h.W.b[name] is None) and (t is None or torch.equal(h.W.b[name], t)), name
    assert torch.equal(h.W.mod_w, W.mod_w) and torch.equal(h.W.mod_b, W.mod_b)
    assert h.W.logit_bound == W.logit_bound and h.W.logit_bounds == W.logit_bounds
    # what vc_flux_bound reports is inside the arena, and the un-permuted rows are not what is bound
    p, b, rows, cols, ld = h.bound("double_blocks.0.img_attn.qkv")
    a0 = h._arena.data_ptr()
    assert (rows, cols, ld) == (768, 256, 256) and a0 <= p < a0 + h._arena.numel() and a0 <= b < a0 + h._arena.numel()
    # the scale kernel: bf16 casts (above, through W.w) and max|.| of every vector, one f32 each behind the scales
    from visualcloze_amd import hip
    names = [k for k in sd if k.endswith("norm.scale")]
    need = hip.lib().vc_flux_load_bytes(h.h)
    base, _ = h._aligned(h._arena)
    off = base - a0 + need - (4 * len(names) + 255) // 256 * 256
    amax = h._arena[off:off + 4 * len(names)].view(torch.float32)
    want = torch.stack([sd[k].to(torch.bfloat16).float().abs().max() for k in names])
    assert len(names) == 12 and torch.equal(amax, want)


def _run(h, inp, stream):
    """one vc_flux_forward at t = 0.7 and a 4-step Euler trajectory"""
    S = 4
    bf = lambda t: t.to(DEV, torch.bfloat16).contiguous()  # noqa: E731
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        h.prepare(bf(inp["txt"]), bf(inp["y"]), inp["guidance"], False, inp["img_ids"], inp["txt_ids"], S, stream=s)
        x, cond = bf(inp["x"]).clone(), bf(inp["cond"])
        fwd = torch.empty_like(x)
        h.forward(torch.cat((x, cond), -1).contiguous(), torch.tensor([0.7]), False, fwd, stream=s)
        traj = torch.empty((S,) + tuple(x.shape), dtype=torch.bfloat16, device=DEV)
        h.sample_euler(x, cond, torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0]), True, s, trajectory=traj)
    stream.synchronize()
    return fwd, x, traj


@pytest.mark.parametrize("outlier", [False, True], ids=["plain", "outlier_block"])
def test_forward_and_trajectory_equal_the_prepared_handle_bitwise(pair, outlier):
    from tests.procedural import tiny_inputs
    # outlier: one block's key scales x 8 - its bound (1.02 sqrt(128) log2(e) max|q| max|k| > 100) leaves the bounded softmax's range,
    # so the cap and the per-block template choice both matter
    m, h = pair if not outlier else (lambda mm: (mm, load(mm)))(make_model(key_scale_factor=8.0))
    ref = m.handle()
    if outlier:
        b = m.engine().W.logit_bounds
        assert b["single_blocks.1"] > 100 > b["single_blocks.0"]
    assert ref is not None and ref is not h and ref._opts["logit_bound_milli"] == h._opts["logit_bound_milli"] > 0
    assert ref._opts == h._opts
    inp = tiny_inputs(B=1)
    st = torch.cuda.Stream()
    a, b = _run(h, inp, st), _run(ref, inp, st)
    for x, y in zip(a, b):
        assert torch.isfinite(x.float()).all() and torch.equal(x, y)
    assert not torch.equal(a[2][0], a[2][1])


def test_second_finish_remerges_and_in_flight_is_refused():
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    m = make_model()
    h = load(m)
    before = h.W.w["img_in"].clone()
    h.reload(0.5)
    torch.cuda.synchronize()
    W = make_model(scale=0.5).prepare().W
    torch.cuda.synchronize()
    assert not torch.equal(h.W.w["img_in"], before)
    for name, t in W.w.items():
        assert torch.equal(h.W.w[name], t), name
    for name, t in W.b.items():
        assert t is None or torch.equal(h.W.b[name], t), name
    assert torch.equal(h.W.mod_w, W.mod_w) and torch.equal(h.W.mod_b, W.mod_b)
    # between vc_flux_sample_begin and vc_flux_sample_end
    inp = tiny_inputs(B=1)
    bf = lambda t: t.to(DEV, torch.bfloat16).contiguous()  # noqa: E731
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        h.prepare(bf(inp["txt"]), bf(inp["y"]), inp["guidance"], False, inp["img_ids"], inp["txt_ids"], 2, stream=s)
        x, cond = bf(inp["x"]).clone(), bf(inp["cond"])
        h.sample_begin(x, cond, torch.tensor([0.0, 0.5, 1.0]), True, s)
        base, nbytes = h._aligned(h._arena)
        assert hip.lib().vc_flux_load_finish(h.h, 0.5, base, nbytes, s) == -3 and b"sample_begin" in hip.lib().vc_last_error()
        h.sample_steps(2, s)
        h.sample_end(x, s)
    st.synchronize()
    assert torch.isfinite(x.float()).all()


def test_flux_switch_builds_the_handle_in_the_library(pair):
    """Flux.load_in_library (opt-in): forward and the fused sampler run on a handle the library prepared, bit-equal to the default
    route; the Python-ordered twin is refused, not prepared a second time."""
    from tests.procedural import tiny_inputs
    from visualcloze_amd import hip
    from visualcloze_amd.transport import Sampler, create_transport
    m, _ = pair
    inp = tiny_inputs(B=2, seed=7)
    kw = dict(txt=inp["txt"].to(DEV, torch.bfloat16), txt_ids=inp["txt_ids"].to(DEV), txt_mask=inp["txt_mask"].to(DEV),
              y=inp["y"].to(DEV, torch.bfloat16), img_ids=inp["img_ids"].to(DEV), img_mask=inp["img_mask"].to(DEV),
              guidance=inp["guidance"].to(DEV))
    img = torch.cat((inp["x"], inp["cond"]), -1).to(DEV, torch.bfloat16)
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=3, do_shift=True, time_shifting_factor=1)
    x = inp["x"].to(DEV, torch.bfloat16)

    def both():
        f = m(img, timesteps=torch.tensor([0.9, 0.25], device=DEV), **kw)
        s = fn(x, m.forward, dict(kw, cond=inp["cond"].to(DEV, torch.bfloat16)))
        torch.cuda.synchronize()
        return f, s
    assert m.load_in_library is False
    ref = both()
    m.load_in_library = True
    try:
        got = both()
        h = m.handle()
        assert getattr(h, "_loaded", None) and m._engine is None and m.handle() is h
        with pytest.raises(hip.VclozeHipError, match="load_in_library"):
            m.engine()
        m.lora_mode = "ref"
        with pytest.raises(hip.VclozeHipError, match="merged"):
            m.handle()
    finally:
        m.lora_mode = "merged"
        m.load_in_library = False
        m.invalidate_engine()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


# ---------------------------------------------------------------- 5. the C99 host program
def test_c_host_program_equals_python_calls_bitwise(tmp_path):
    from tests.test_c_abi import CTX, D, DEPTH, HEADS, IN_CH, MLP, N, OUT_CH, SINGLE, STEPS, T, VEC, fill
    from tests.test_flux_load_cpu import build_demo
    from visualcloze_amd import hip
    L = hip.lib()
    exe = build_demo(tmp_path)
    out_file = tmp_path / "out.bin"
    r = subprocess.run([exe, str(out_file)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = torch.from_numpy(np.fromfile(out_file, dtype=np.int16)).view(torch.bfloat16).reshape(2 + STEPS, N, OUT_CH)

    keep = []
    h = C.c_void_p()
    cfg = hip.FluxConfig(IN_CH, OUT_CH, VEC, CTX, D, HEADS, DEPTH, SINGLE, MLP, 1, (C.c_int32 * 3)(16, 56, 56), 10000)
    hip._check(L.vc_flux_create(C.byref(cfg), C.byref(h)), "create")
    try:
        buf, shape, nd, n_keys = C.create_string_buffer(160), (C.c_int64 * 2)(), C.c_int32(0), 0
        while L.vc_flux_load_key(h, n_keys, buf, 160, shape, C.byref(nd)) == 0:
            n_keys += 1
            key = buf.value.decode()
            if key.startswith("txt_in.lora_"):
                continue
            dims = [16 if v < 0 else v for v in shape[:nd.value]]
            scale, offset = 0.06, 0.0
            if key.endswith(".scale"):
                scale, offset = 0.1, 1.0
            elif key.endswith((".lora_A.weight", ".lora_B.weight")):
                scale = 0.1
            elif key.endswith(".lora_B.bias"):
                scale = 0.02
            elif key.endswith(".bias"):
                scale = 0.05
            t = fill(key, int(np.prod(dims)), scale, offset)
            keep.append(t)
            hip._check(L.vc_flux_load_tensor(h, key.encode(), t.data_ptr(), 0, (C.c_int64 * len(dims))(*dims), len(dims)), key)
        st = torch.cuda.Stream()
        s = st.cuda_stream
        arena = torch.empty(L.vc_flux_load_bytes(h) + 256, dtype=torch.uint8, device=DEV)
        abase = (arena.data_ptr() + 255) & ~255
        torch.cuda.synchronize()
        hip._check(L.vc_flux_load_finish(h, 0.75, abase, arena.numel() - 256, s), "finish")
        txt, y = fill("input.txt", T * CTX, 1.0), fill("input.y", VEC, 1.0)
        x, cond = fill("input.x", N * OUT_CH, 1.0).reshape(N, OUT_CH), fill("input.cond", N * (IN_CH - OUT_CH), 1.0).reshape(N, IN_CH - OUT_CH)
        r_ = np.arange(N)
        img_ids = np.stack([r_ // 12 + 1, (r_ % 12) // 6, r_ % 6], 1).astype(np.float32).copy()
        txt_ids, guidance = np.zeros((T, 3), np.float32), np.asarray([30.0], np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        ws = torch.empty(L.vc_flux_workspace_bytes(h, 1, T, N, STEPS) + 256, dtype=torch.uint8, device=DEV)
        base = (ws.data_ptr() + 255) & ~255
        inp = hip.FluxInputs(1, T, N, STEPS, txt.data_ptr(), y.data_ptr(), fp(guidance), fp(img_ids), fp(txt_ids), None, None, 0, 0)
        torch.cuda.synchronize()
        hip._check(L.vc_flux_prepare(h, C.byref(inp), base, ws.numel() - 256, s), "prepare")
        img = torch.empty(N, IN_CH, dtype=torch.bfloat16, device=DEV)
        fwd = torch.empty(N, OUT_CH, dtype=torch.bfloat16, device=DEV)
        traj = torch.empty(STEPS, N, OUT_CH, dtype=torch.bfloat16, device=DEV)
        hip._check(L.vc_concat_cols(x.data_ptr(), OUT_CH, cond.data_ptr(), IN_CH - OUT_CH, img.data_ptr(), N, s), "concat")
        t07 = np.asarray([0.7], np.float32)
        hip._check(L.vc_flux_forward(h, img.data_ptr(), fp(t07), 0, fwd.data_ptr(), s), "forward")
        grid = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)
        xs = x.clone()
        hip._check(L.vc_flux_sample_euler(h, xs.data_ptr(), cond.data_ptr(), fp(grid), STEPS + 1, 1, traj.data_ptr(), s), "sample")
        torch.cuda.synchronize()
    finally:
        L.vc_flux_destroy(h)
    assert f"{n_keys - 3} of {n_keys} keys recorded" in r.stdout
    assert torch.isfinite(got.float()).all() and float(got.float().abs().max()) > 0
    assert torch.equal(got[0].cpu(), fwd.cpu())
    assert torch.equal(got[1].cpu(), xs.cpu())
    assert torch.equal(got[2:].cpu(), traj.cpu()) and torch.equal(traj[-1], xs)
    assert not torch.equal(traj[0], traj[1])
