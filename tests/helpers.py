"""Test helpers: the tiny procedural-weight model on the GPU and the smoke check of the HIP path against the CPU
oracle (used by tests/ and __graft_entry__.smoke(); lives outside the product package because it imports oracle/)."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def tiny_model(dev="cuda:0", dtype=torch.bfloat16):
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from tests.procedural import TINY, TINY_RANK, procedural_param
    from visualcloze_amd.model import FluxLoraWrapper, FluxParams
    m = FluxLoraWrapper(lora_rank=TINY_RANK, lora_scale=1.0, params=FluxParams(**TINY))
    sd = {k: procedural_param(k, v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    return m.eval().to(dev, dtype), sd


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


# sentinel-filled output buffers of the kernel tests: everything a kernel must not write is checked to be untouched
def sentinel(shape, value=7.0):
    return torch.full(shape, value, dtype=torch.bfloat16, device="cuda:0")


def untouched(buf, value=7.0):
    """every element still holds the sentinel's bit pattern"""
    from tests.budget import bits_equal
    return bits_equal(buf, torch.full(buf.shape, value, dtype=torch.bfloat16))


def patterned(shape):
    """bf16 tensor whose element i holds bit pattern i + 1: every value distinct, none a NaN (numel < 0x7F80)"""
    n = 1
    for s in shape:
        n *= s
    assert n < 0x7F80
    return (torch.arange(n, dtype=torch.int32) + 1).to(torch.int16).view(torch.bfloat16).reshape(shape)


def smoke() -> None:
    from visualcloze_amd import hip
    hip.require_gpu()
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import oracle.flux_oracle as O  # test infrastructure: the checker, not the thing run
    from tests.procedural import TINY, tiny_inputs
    model, sd = tiny_model()
    inp = tiny_inputs(B=1)
    dev = "cuda:0"
    img = torch.cat((inp["x"], inp["cond"]), -1)
    t = torch.tensor([0.7])
    got = model(img.to(dev, torch.bfloat16), img_ids=inp["img_ids"].to(dev), txt=inp["txt"].to(dev, torch.bfloat16),
                txt_ids=inp["txt_ids"].to(dev), timesteps=t.to(dev), y=inp["y"].to(dev, torch.bfloat16),
                txt_mask=inp["txt_mask"].to(dev), img_mask=inp["img_mask"].to(dev), guidance=inp["guidance"].to(dev))
    torch.cuda.synchronize()
    G = O.FluxGeometry(**TINY)
    orig = O.compute_vec
    O.compute_vec = lambda *a, **k: orig(*a, **{**k, "guidance_is_bf16": False})
    try:
        want = O.flux_forward(sd, G, img, inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], inp["txt_mask"],
                              inp["img_mask"], inp["guidance"], P=O.Prec("bf16", "merged"))
    finally:
        O.compute_vec = orig
    err = rel_l2(got, want)
    print(f"smoke: tiny Flux.forward on {torch.cuda.get_device_name(0)}: rel-L2 vs bf16 oracle = {err:.3e}")
    assert torch.isfinite(got.float()).all() and err < 2e-2, f"HIP path deviates from the oracle: {err}"


def parity_log(line: str) -> None:
    """Print a measured deviation and, when VC_PARITY_LOG names a file, append it there (the numbers DESIGN.md quotes
    come from these lines; pytest swallows stdout of passing tests)."""
    print("\n" + line)
    path = os.environ.get("VC_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def gemm_plan_case(group: dict, case: list):
    """One case of tests/golden/gemm_plans.json.gz -> (GemmArgs, tile_cfg, expected).  group = {"p": [[M, N, K, {field: value}?] ...],
    "epi", "args": {GemmArgs field: value}?}; case = [tile_cfg, scratch state (index into the header's "ws"), batch, expected].
    Fields a problem does not name: A = W = C = res = gate = 0x1000 (the planner never dereferences them), lda = ldw = K,
    ldc = ldres = N, rows_per_batch = M, everything else 0."""
    from visualcloze_amd import hip
    tile_cfg, ws, batch, expected = case
    a = hip.GemmArgs()
    a.nprob, a.epi, a.batch = len(group["p"]), group["epi"], batch
    a.splitk_ws, a.splitk_ws_bytes = GEMM_PLAN_WS[ws]
    for i, (M, N, K, *extra) in enumerate(group["p"]):
        p = a.p[i]
        p.A = p.W = p.C = p.res = p.gate = 0x1000
        p.lda, p.ldw, p.ldc, p.ldres = K, K, N, N
        p.M, p.N, p.K, p.rows_per_batch = M, N, K, M
        for k, v in (extra[0] if extra else {}).items():
            setattr(p, k, v)
    for k, v in group.get("args", {}).items():
        setattr(a, k, v)
    return a, tile_cfg, expected


# the split-K scratch on offer: none / the size the product allocates / too small for most remainders (4 MiB)
GEMM_PLAN_WS = [(0, 0), (0x1000, 2 * 256 * 256 * 192 * 4), (0x1000, 4 << 20)]


def gemm_plan_answer(lib, a, tile_cfg):
    """what vc_gemm_plan answers: the eight integers, or [return code, error text]"""
    import ctypes as C
    out = (C.c_int32 * 8)()
    rc = lib.vc_gemm_plan(C.byref(a), tile_cfg, out)
    return list(out) if rc == 0 else [rc, lib.vc_last_error().decode()]


def attn_scratch_states(n_cu: int):
    """the attention scratch on offer, by state index of tests/golden/attn_plans.json.gz: none / one byte short of the 64-query
    partials / exactly those / the whole buffer minus one byte / the whole buffer / a whole buffer's size behind a null pointer.
    The sizes are written out here (not asked of the library): 2 pieces per CU of 68 KiB (attention64) or 4 of 66 KiB (attention),
    the larger rounded up to 256, then 16 bytes of flag words per CU rounded up to 256."""
    p64, p32 = n_cu * 2 * (65536 + 4096), n_cu * 4 * (16384 + 512) * 4
    whole = (max(p64, p32) + 255) // 256 * 256 + (n_cu * 16 + 255) // 256 * 256
    return [(0, 0), (0x1000, p64 - 1), (0x1000, p64), (0x1000, whole - 1), (0x1000, whole), (0, whole)]


def attn_plan_case(group: dict, case: list):
    """One case of tests/golden/attn_plans.json.gz -> (hip.Attention, n_cu, expected).  group = {"B", "L", "H", "n_cu", "o": {Attention
    field: value}?}; case = [variant, mask, scratch state, query form, logit_bound, expected].  mask: bit 0 = kv_len, bit 1 = kv_gap;
    query form: bit 0 = q_scale, bit 1 = q_scale2 (with split = L // 2), bit 2 = rope, bit 3 = q_prescaled.  Fields the group does not
    name: every pointer 0x1000 (the planner never dereferences one), ld = 3 * 128 H, ldo = 128 H, sample strides L * ld and L * ldo,
    Lpad = L rounded up to 64."""
    from visualcloze_amd import hip
    variant, mask, scratch, qform, bound, expected = case
    B, L, H, n_cu = group["B"], group["L"], group["H"], group["n_cu"]
    a = hip.Attention()
    a.qkv = a.vt = a.out = 0x1000
    a.B, a.L, a.H, a.Lpad, a.variant = B, L, H, (L + 63) // 64 * 64, variant
    a.ld, a.ldo = 3 * 128 * H, 128 * H
    a.bstride, a.out_bstride = L * a.ld, L * a.ldo
    a.kv_len, a.kv_gap = 0x1000 if mask & 1 else 0, 0x1000 if mask & 2 else 0
    a.scratch, a.scratch_bytes = attn_scratch_states(n_cu)[scratch]
    a.q_scale, a.q_scale2, a.rope = 0x1000 if qform & 1 else 0, 0x1000 if qform & 2 else 0, 0x1000 if qform & 4 else 0
    a.split, a.rope_bstride, a.q_prescaled = L // 2 if qform & 2 else 0, L * 128 if qform & 4 else 0, 1 if qform & 8 else 0
    a.logit_bound = bound
    for k, v in group.get("o", {}).items():
        setattr(a, k, v)
    return a, n_cu, expected


def attn_plan_answer(lib, a, n_cu):
    """what vc_attention_plan answers: the sixteen integers, or [return code, error text]"""
    import ctypes as C
    out = (C.c_int32 * 16)()
    rc = lib.vc_attention_plan(C.byref(a), n_cu, out)
    return list(out) if rc == 0 else [rc, lib.vc_last_error().decode()]
