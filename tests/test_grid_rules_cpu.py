"""CPU: the host rules of one grid in the C ABI - vc_time_grid, vc_grid_tokens, vc_grid_img_ids (csrc/grid_rules.hip) - against the
Python functions they restate, BIT FOR BIT; their argument errors; the grid handle's struct sizes; and tests/c_abi/grid_demo.c as a
C99 program.  None of it needs a device."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ERR_ARG = -1

# every combination is finite in transport.solver_time_grid itself (asserted below, case by case)
N_POINTS = [2, 3, 5, 10, 30, 50]
N_TOKENS = [14, 1152, 3456, 4096, 6912]
FACTORS = [None, 0, 1, 1.5]
SPANS = [(0, 1), (0.4, 1)]


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        h.build()
    h.lib()
    return h


@pytest.mark.parametrize("n_points", N_POINTS)
@pytest.mark.parametrize("do_shift", [True, False])
def test_time_grid_equals_solver_time_grid_bitwise(hip, n_points, do_shift):
    from visualcloze_amd.transport import solver_time_grid
    for n_tokens, tsf, (t0, t1) in itertools.product(N_TOKENS, FACTORS, SPANS):
        want = solver_time_grid(n_points, n_tokens, t0, t1, do_shift, tsf)
        assert want.dtype == torch.float32 and torch.isfinite(want).all(), (n_points, n_tokens, tsf, t0)
        got = hip.time_grid(n_points, n_tokens, t0, t1, do_shift, tsf)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n_points, n_tokens, do_shift, tsf, t0, got, want)
    # the pipeline's two grids: 30 shifted points of a 3456-token grid, 10 un-shifted points from strength 0.4
    assert float(hip.time_grid(30, 3456)[0]) == 0.0 and float(hip.time_grid(30, 3456)[-1]) == 1.0


@pytest.mark.parametrize("args, word", [
    (dict(n_points=1), b"n_points"), (dict(n_points=0), b"n_points"), (dict(n_tokens=0), b"n_tokens"),
    (dict(t0=1.0, t1=1.0), b"forward time"), (dict(t0=0.7, t1=0.2), b"forward time"),
    (dict(t0=float("nan")), b"finite"), (dict(t1=float("inf")), b"finite"), (dict(tsf=float("nan")), b"finite"), (dict(null=True), b"null"),
])
def test_time_grid_argument_errors(hip, args, word):
    L = hip.lib()
    a = dict(n_points=4, n_tokens=14, t0=0.0, t1=1.0, tsf=1.0, null=False)
    a.update(args)
    out = (C.c_float * 8)(*([7.0] * 8))
    rc = L.vc_time_grid(a["n_points"], a["n_tokens"], a["t0"], a["t1"], 1, a["tsf"], None if a["null"] else out)
    assert rc == ERR_ARG and word in L.vc_last_error(), L.vc_last_error()
    assert list(out) == [7.0] * 8                       # nothing was written


@pytest.mark.parametrize("rows", [[(4, 8)], [(4, 8), (4, 6)], [(2, 2), (6, 10), (4, 4)]], ids=["one", "two_unequal", "three"])
def test_grid_img_ids_equal_prepare_grid(hip, rows):
    from visualcloze_amd import packing
    want = packing.grid_img_ids(rows)                   # what packing.prepare_grid writes into img_ids
    got = hip.grid_img_ids(rows)
    assert hip.grid_tokens(rows) == want.shape[0] == sum((h // 2) * (w // 2) for h, w in rows)
    assert got.shape == want.shape and torch.equal(got, want)
    assert got[0].tolist() == [1.0, 0.0, 0.0] and got[-1].tolist() == [float(len(rows)), rows[-1][0] // 2 - 1, rows[-1][1] // 2 - 1]


def test_grid_img_ids_argument_errors(hip):
    L = hip.lib()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    out = (C.c_float * 64)()
    assert L.vc_grid_tokens(0, i32(4), i32(4)) == ERR_ARG and b"rows" in L.vc_last_error()
    assert L.vc_grid_tokens(1, None, i32(4)) == ERR_ARG
    assert L.vc_grid_tokens(2, i32(4, 3), i32(4, 4)) == ERR_ARG and b"row 1" in L.vc_last_error()
    assert L.vc_grid_tokens(1, i32(4), i32(0)) == ERR_ARG and L.vc_grid_tokens(1, i32(-2), i32(4)) == ERR_ARG
    assert L.vc_grid_img_ids(1, i32(4), i32(4), None) == ERR_ARG and b"null" in L.vc_last_error()
    assert L.vc_grid_img_ids(1, i32(4), i32(5), out) == ERR_ARG and L.vc_grid_img_ids(0, i32(4), i32(4), out) == ERR_ARG
    assert L.vc_grid_tokens(1, i32(4), i32(6)) == 6


def test_grid_struct_sizes_match_the_ctypes_mirrors(hip):
    sizes = (C.c_int32 * 3)()
    hip.lib().vc_grid_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(hip.GridConfig), C.sizeof(hip.GridJob), C.sizeof(hip.GridSdedit)]
    R = hip.GRID_MAX_ROWS
    assert C.sizeof(hip.GridConfig) == 4 * 8
    assert C.sizeof(hip.GridJob) == 2 * 4 + 2 * R * 4 + 2 * R * 8 + R * 4 + 2 * 8 + 2 * 4 + 3 * 8 + 6 * 4 + 8
    assert C.sizeof(hip.GridSdedit) == 4 * 4 + R * 8 + 2 * 8 + 2 * 4 + 3 * 8 + 6 * 4 + 8
    # the entry points are there without an ABI bump: a binding detects them by symbol
    assert hip.lib().vc_abi_version() == 11 and hasattr(hip.lib(), "vc_grid_create")
    # host-only entry points refuse null arguments with a message, before any device work
    L = hip.lib()
    h = C.c_void_p()
    assert L.vc_grid_create(None, C.byref(h)) == ERR_ARG and b"null" in L.vc_last_error()
    cfg = hip.GridConfig(None, None, None, None)
    assert L.vc_grid_create(C.byref(cfg), C.byref(h)) == ERR_ARG and b"required" in L.vc_last_error()
    assert L.vc_grid_destroy(None) == ERR_ARG and L.vc_grid_generate(None, None, None, 0, None, None) == ERR_ARG
    assert L.vc_pixels_out(None, 0, 8, 8, 0, 8, None, 0, None) == ERR_ARG and b"null" in L.vc_last_error()


def test_use_grid_handle_is_never_silently_ignored():
    """the keyword is valid only with a NoiseStream (checked before anything else is touched)"""
    from visualcloze_amd import pipeline
    for fn, args in ((pipeline.generate_grid, (None, None, None, None, [], [], None, None, 0)),
                     (pipeline.generate_and_upsample, (None, None, None, None, [torch.zeros(3, 16, 16)], [], None, None, 0, 1, [True]))):
        with pytest.raises(ValueError, match="NoiseStream"):
            fn(*args, use_grid_handle=True)
        with pytest.raises(ValueError, match="NoiseStream"):
            fn(*args, use_grid_handle=True, rng=torch.Generator())
    with pytest.raises(ValueError, match="encode_noise"):
        pipeline.generate_grid(None, None, None, None, [torch.zeros(3, 16, 16)], [], None, None, 0, rng=pipeline.NoiseStream(1),
                               encode_noise=[torch.zeros(1)], use_grid_handle=True)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_grid_demo_compiles_and_links_as_c99(hip, tmp_path):
    from tests.grid_demo_build import build_grid_demo
    exe = build_grid_demo(tmp_path)
    assert os.path.getsize(exe) > 0
