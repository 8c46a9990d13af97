"""CPU: the host side of vc_flux_load_* - a checkpoint as stored behind the Flux handle (include/vcloze_hip.h).  The key table
against FluxLoraWrapper.state_dict(), the arena formula, every argument / state error before the device is touched, the
destination-row rule of vc_lora_merge_qkv against hip.qkv_head_permutation, the C99 host program, and the key table alone as a
sanitized host program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.procedural import TINY

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NAMES = ("vc_lora_merge_qkv", "vc_flux_load_key", "vc_flux_load_tensor", "vc_flux_load_bytes", "vc_flux_load_finish", "vc_flux_bound")
ERR_ARG, ERR_STATE = -1, -3


def _lib():
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def _create(p: dict):
    from visualcloze_amd import hip
    L = _lib()
    D = p["hidden_size"]
    cfg = hip.FluxConfig(p["in_channels"], p["out_channels"], p["vec_in_dim"], p["context_in_dim"], D, p["num_heads"], p["depth"],
                         p["depth_single_blocks"], int(D * p["mlp_ratio"]), int(p["guidance_embed"]), (C.c_int32 * 3)(*p["axes_dim"]),
                         p["theta"])
    h = C.c_void_p()
    assert L.vc_flux_create(C.byref(cfg), C.byref(h)) == 0, L.vc_last_error()
    return L, h


def _keys(L, h) -> list:
    out, buf, shape, nd = [], C.create_string_buffer(160), (C.c_int64 * 2)(), C.c_int32(0)
    while L.vc_flux_load_key(h, len(out), buf, 160, shape, C.byref(nd)) == 0:
        out.append((buf.value.decode(), tuple(shape[:nd.value])))
    return out


def _record(L, h, key, shape, ptr=0x10000, f32=0):
    return L.vc_flux_load_tensor(h, key.encode(), ptr, f32, (C.c_int64 * max(len(shape), 1))(*shape), len(shape))


def _err(L) -> str:
    return L.vc_last_error().decode()


def test_entry_points_declared_exported_bound_and_abi_11():
    from visualcloze_amd import hip
    L = _lib()
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    raw = C.CDLL(hip.LIB_PATH)
    for name in NAMES:
        m = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m, f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in hip.SYMBOLS and len(hip.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    assert L.vc_abi_version() == 11 and "#define VC_ABI_VERSION 11" in hdr
    assert "look up vc_flux_load_tensor" in hdr
    # vc_lora_merge_qkv is vc_lora_merge with ONE more argument, in front of the stream
    assert hip.SYMBOLS["vc_lora_merge_qkv"][1] == hip.SYMBOLS["vc_lora_merge"][1][:-1] + [C.c_int32, C.c_void_p]


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_key_table_is_the_state_dict_of_the_lora_wrapper(which):
    from visualcloze_amd.model import FLUX_DEV_FILL, FluxLoraWrapper, FluxParams
    p = TINY if which == "tiny" else FLUX_DEV_FILL
    rank = 16
    with torch.device("meta"):
        sd = FluxLoraWrapper(rank, 1.0, FluxParams(**p)).state_dict()
    want = []
    for k, t in sd.items():
        shape = list(t.shape)
        if k.endswith(".lora_A.weight"):
            assert shape[0] == rank
            shape[0] = -1
        if k.endswith(".lora_B.weight"):
            assert shape[1] == rank
            shape[1] = -1
        want.append((k, tuple(shape)))
    L, h = _create(p)
    try:
        got = _keys(L, h)
        assert got == want, [x for x in zip(got, want) if x[0] != x[1]][:3]
        assert len(got) == len(set(k for k, _ in got))
        # past the end, and a truncated name buffer
        buf, shape, nd = C.create_string_buffer(8), (C.c_int64 * 2)(), C.c_int32(0)
        assert L.vc_flux_load_key(h, len(got), buf, 8, shape, C.byref(nd)) == ERR_ARG and "index" in _err(L)
        assert L.vc_flux_load_key(h, -1, buf, 8, shape, C.byref(nd)) == ERR_ARG
        assert L.vc_flux_load_key(h, 1, buf, 8, shape, C.byref(nd)) == 0 and buf.value.decode() == got[1][0][:7]
    finally:
        L.vc_flux_destroy(h)


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_arena_bytes_is_the_formula_of_the_header(which):
    from visualcloze_amd.model import FLUX_DEV_FILL
    p = TINY if which == "tiny" else FLUX_DEV_FILL
    L, h = _create(p)
    try:
        c = lambda v: (v + 255) // 256 * 256  # noqa: E731
        D, n_mod = p["hidden_size"], L.vc_flux_mod_offset(h, None)
        n_scales = 4 * p["depth"] + 2 * p["depth_single_blocks"]
        total = c(2 * n_mod * D) + c(2 * n_mod) + 256 * n_scales + c(4 * n_scales)
        for k, shape in _keys(L, h):
            if k.endswith(".weight") and ".lora_" not in k and L.vc_flux_mod_offset(h, k[:-len(".weight")].encode()) < 0:
                total += c(2 * shape[0] * shape[1]) + c(2 * shape[0])
        assert L.vc_flux_load_bytes(h) == total
        assert L.vc_flux_load_bytes(None) == -1
        if which == "full":
            assert 23.7e9 < total < 23.9e9          # the merged set of FLUX.1-Fill (23.8 GB)
    finally:
        L.vc_flux_destroy(h)


def test_argument_and_state_errors_before_the_device_is_touched():
    L, h = _create(TINY)
    try:
        keys = dict(_keys(L, h))
        D = TINY["hidden_size"]
        q = "double_blocks.1.txt_attn.qkv"
        # ---- vc_flux_load_tensor
        assert _record(L, h, "double_blocks.9.img_attn.qkv.weight", (3 * D, D)) == ERR_ARG and "double_blocks.9.img_attn.qkv.weight" in _err(L)
        assert _record(L, h, q, (3 * D, D)) == ERR_ARG and "no state_dict key" in _err(L)                  # a module path is no key
        assert _record(L, h, q + ".weight", (D, 3 * D)) == ERR_ARG and q + ".weight" in _err(L) and "768, 256" in _err(L)
        assert _record(L, h, q + ".weight", (3 * D * D,)) == ERR_ARG and q + ".weight" in _err(L)
        assert _record(L, h, q + ".bias", (3 * D, 1)) == ERR_ARG
        assert _record(L, h, q + ".lora_A.weight", (513, D)) == ERR_ARG and "rank" in _err(L)
        assert _record(L, h, q + ".lora_A.weight", (16, D), f32=1) == ERR_ARG and "bf16" in _err(L) and q + ".lora_A.weight" in _err(L)
        assert _record(L, h, q + ".lora_B.bias", (3 * D,), f32=1) == ERR_ARG and "bf16" in _err(L)
        assert _record(L, h, q + ".lora_A.weight", (16, D)) == 0
        assert _record(L, h, q + ".lora_B.weight", (3 * D, 32)) == ERR_ARG and "rank" in _err(L) and q + ".lora_B.weight" in _err(L)
        assert _record(L, h, q + ".lora_B.weight", (3 * D, 16)) == 0
        assert _record(L, h, q + ".lora_A.weight", (16, D), ptr=None) == 0                                    # NULL forgets the key
        assert _record(L, h, q + ".lora_B.weight", (3 * D, 512)) == 0 and _record(L, h, q + ".lora_B.weight", (3 * D, 0)) == 0
        assert _record(L, h, q + ".weight", (3 * D, D), f32=1) == 0                                           # base tensors may be f32
        assert _record(L, h, "double_blocks.1.txt_attn.norm.key_norm.scale", (128,), f32=1) == 0
        assert _record(L, h, "double_blocks.1.txt_attn.norm.key_norm.scale", (64,)) == ERR_ARG
        assert L.vc_flux_load_tensor(h, None, 0x10000, 0, None, 0) == ERR_ARG
        # ---- vc_flux_load_finish: the arena, the mode, what is missing
        need = L.vc_flux_load_bytes(h)
        arena = 0x7f0000000000
        assert L.vc_flux_load_finish(h, 1.0, None, need, None) == ERR_ARG and "arena" in _err(L)
        assert L.vc_flux_load_finish(h, 1.0, arena + 128, need, None) == ERR_ARG and "256-byte" in _err(L)
        assert L.vc_flux_load_finish(h, 1.0, arena, need - 1, None) == ERR_ARG and "arena_bytes" in _err(L) and str(need) in _err(L)
        assert L.vc_flux_set_option(h, b"lora_mode", 1) == 0
        assert L.vc_flux_load_finish(h, 1.0, arena, need, None) == ERR_ARG and "lora_mode" in _err(L)
        assert L.vc_flux_set_option(h, b"lora_mode", 0) == 0
        assert L.vc_flux_load_finish(h, 1.0, arena, need, None) == ERR_STATE and "'img_in.weight'" in _err(L)      # the first key
        for k, shape in keys.items():
            if k.endswith(".weight") and ".lora_" not in k and k not in ("time_in.out_layer.weight", "final_layer.linear.weight"):
                assert _record(L, h, k, shape) == 0, k
        assert L.vc_flux_load_finish(h, 1.0, arena, need, None) == ERR_STATE and "'time_in.out_layer.weight'" in _err(L)
        assert _record(L, h, "time_in.out_layer.weight", (D, D)) == 0
        assert L.vc_flux_load_finish(h, 1.0, arena, need, None) == ERR_STATE and "'double_blocks.0.img_attn.norm.query_norm.scale'" in _err(L)
        for k, shape in keys.items():
            if k.endswith(".scale"):
                assert _record(L, h, k, shape) == 0, k
        assert L.vc_flux_load_finish(h, 1.0, arena, need, None) == ERR_STATE and "'final_layer.linear.weight'" in _err(L)
        assert _record(L, h, "final_layer.linear.weight", (TINY["out_channels"], D)) == 0
        # the factor left over from above (lora_B of rank 0 without lora_A) is named too
        assert L.vc_flux_load_finish(h, 1.0, arena, need, None) == ERR_STATE and q + ".lora_B.weight" in _err(L)
        assert L.vc_flux_load_finish(None, 1.0, arena, need, None) == ERR_ARG
        # ---- vc_flux_bound
        w, b, rows, cols, ld = C.c_void_p(), C.c_void_p(), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        args = (C.byref(w), C.byref(b), C.byref(rows), C.byref(cols), C.byref(ld))
        assert L.vc_flux_bound(h, b"img_in", *args) == ERR_STATE and "img_in" in _err(L)
        assert L.vc_flux_bound(h, None, *args) == ERR_ARG
        assert L.vc_flux_bind_weight(h, b"img_in", 0x4000, 0x8000, D, 384, 392) == 0
        assert L.vc_flux_bound(h, b"img_in", *args) == 0
        assert (w.value, b.value, rows.value, cols.value, ld.value) == (0x4000, 0x8000, D, 384, 392)
        assert L.vc_flux_bound(h, b"img_in", None, None, None, None, None) == 0
    finally:
        L.vc_flux_destroy(h)


def _dest_row(r: int, H: int) -> int:
    """the rule of include/vcloze_hip.h (vc_lora_merge_qkv)"""
    D = 128 * H
    if r < 2 * D:
        return 192 * (r // 128) + r % 128
    if r < 3 * D:
        u = r - 2 * D
        return 192 * (u // 64) + 128 + u % 64
    return r


@pytest.mark.parametrize("H", [1, 2, 24])
def test_destination_rows_invert_the_head_permutation(H):
    from visualcloze_amd import hip
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    for line in ("192 * (r / 128) + r % 128", "192 * (u / 64) + 128 + u % 64,   u = r - 2D"):
        assert line in hdr
    D = 128 * H
    perm = hip.qkv_head_permutation(H)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(3 * D)
    dest = torch.tensor([_dest_row(r, H) for r in range(3 * D + 512)])
    assert torch.equal(dest[:3 * D], inv) and torch.equal(dest[3 * D:], torch.arange(3 * D, 3 * D + 512))
    # a wave's 16 source rows, which start at a multiple of 16, stay 16 consecutive rows
    d16 = dest[:3 * D].reshape(-1, 16)
    assert torch.equal(d16 - d16[:, :1], torch.arange(16).expand_as(d16)) and bool((d16[:, 0] % 16 == 0).all())


def build_demo(out_dir) -> str:
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    exe = os.path.join(str(out_dir), "flux_load_demo")
    libdir = os.path.dirname(hip.LIB_PATH)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(ROCM, "include"),
           os.path.join(REPO, "tests", "c_abi", "flux_load_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip",
           "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_host_program_compiles_and_links_as_c99(tmp_path):
    assert os.path.getsize(build_demo(tmp_path)) > 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_key_table_as_a_sanitized_host_program(tmp_path):
    """csrc/flux_keys.h + flux_keys.hip need nothing from HIP: tests/c_abi/flux_keys_check.cpp (its own main) walks the tables of four
    configurations - exact-size name buffers, truncated ones, indices out of range, long and foreign keys, every shape rule - under
    AddressSanitizer and UBSan.  The program runs directly, on the host."""
    csrc = os.path.join(REPO, "visualcloze_amd", "csrc")
    exe = str(tmp_path / "flux_keys_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I" + csrc,
           os.path.join(REPO, "tests", "c_abi", "flux_keys_check.cpp"), "-x", "c++", os.path.join(csrc, "flux_keys.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "flux_keys ok" and not r.stderr, r.stdout + r.stderr
