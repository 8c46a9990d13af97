"""CPU: the host side of the numerics monitor (include/vcloze_hip.h: vc_tensor_stats, vc_flux_set_monitor and its companions) - the
surface, the VcStat mirror, every argument error before the device is touched, the site enumeration, and the site / log arithmetic alone
as a sanitized host program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.procedural import TINY

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vc_monitor_struct_sizes", "vc_tensor_stats", "vc_flux_step_nodes", "vc_flux_set_monitor", "vc_flux_monitor_sites", "vc_flux_monitor_bytes",
         "vc_flux_monitor_report")
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


def _err(L) -> str:
    return L.vc_last_error().decode()


def _sites(L, h) -> list:
    out, buf = [], C.create_string_buffer(64)
    while L.vc_flux_monitor_sites(h, len(out), buf, 64) == 0:
        out.append(buf.value.decode())
    return out


def test_entry_points_declared_exported_bound_and_abi_11():
    from visualcloze_amd import hip
    L = _lib()
    hdr = open(os.path.join(REPO, "include", "vcloze_hip.h")).read()
    raw = C.CDLL(hip.LIB_PATH)
    for name in NAMES:
        m = re.search(r"^(?:int|void) " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m, f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in hip.SYMBOLS and len(hip.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    assert L.vc_abi_version() == 11 and "#define VC_ABI_VERSION 11" in hdr
    assert "look up vc_flux_set_monitor" in hdr and re.search(r"#define VC_MONITOR_MAX_BLOCKS 256\b", hdr)
    assert hip.MONITOR_MAX_BLOCKS == 256


def test_vcstat_is_16_bytes_and_matches_the_mirror():
    from visualcloze_amd import hip
    L = _lib()
    size = (C.c_int32 * 1)()
    L.vc_monitor_struct_sizes(size)
    assert size[0] == 16 == C.sizeof(hip.Stat) == hip.STAT_DTYPE.itemsize
    fields = [(n, C.sizeof(t), getattr(hip.Stat, n).offset) for n, t in hip.Stat._fields_]
    assert fields == [("max_abs", 4, 0), ("sum_sq", 4, 4), ("nonfinite", 4, 8), ("count", 4, 12)]
    assert [(n, hip.STAT_DTYPE.fields[n][1]) for n in hip.STAT_DTYPE.names] == [(n, o) for n, _, o in fields]


def test_tensor_stats_argument_errors_before_the_device_is_touched():
    L = _lib()
    x, out, scratch = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000      # never dereferenced: every call fails its checks

    def call(x=x, f32=0, bstride=64, ld=8, B=2, rows=8, cols=8, out=out, out_stride=2, row_ptr=None, capacity=1, scratch=scratch):
        return L.vc_tensor_stats(x, f32, bstride, ld, B, rows, cols, out, out_stride, row_ptr, capacity, scratch, None)

    for kw, word in ((dict(x=None), "null"), (dict(out=None), "null"), (dict(scratch=None), "null"), (dict(B=0), "B = 0"),
                     (dict(B=70000), "B = 70000"), (dict(rows=0), "rows = 0"), (dict(rows=-4), "rows = -4"), (dict(cols=0), "cols = 0"),
                     (dict(capacity=0), "capacity = 0"), (dict(bstride=-1), "bstride = -1"), (dict(ld=7), "ld = 7"),
                     (dict(out_stride=1), "out_stride = 1"), (dict(out=out + 8), "16-byte"), (dict(x=x + 1), "aligned"),
                     (dict(f32=1, x=x + 2), "aligned"), (dict(rows=1 << 31, cols=8), "32-bit"), (dict(rows=1 << 30, cols=4, ld=4), "32-bit")):
        assert call(**kw) == ERR_ARG and word in _err(L), (kw, _err(L))


def test_set_monitor_argument_errors_and_site_lists():
    L, h = _create(TINY)
    log, scratch = 0x7f0000100000, 0x7f0000200000
    try:
        assert (TINY["depth"], TINY["depth_single_blocks"]) == (2, 2)
        assert _sites(L, h) == []                                            # off: no site
        assert L.vc_flux_monitor_sites(h, 0, C.create_string_buffer(8), 8) == ERR_ARG and "index = 0" in _err(L)
        assert L.vc_flux_set_monitor(None, 1, log, 4, scratch) == ERR_ARG
        assert L.vc_flux_set_monitor(h, 3, log, 4, scratch) == ERR_ARG and "level = 3" in _err(L)
        assert L.vc_flux_set_monitor(h, -1, log, 4, scratch) == ERR_ARG
        assert L.vc_flux_set_monitor(h, 1, None, 4, scratch) == ERR_ARG and "null" in _err(L)
        assert L.vc_flux_set_monitor(h, 1, log, 4, None) == ERR_ARG and "null" in _err(L)
        assert L.vc_flux_set_monitor(h, 1, log + 8, 4, scratch) == ERR_ARG and "16-byte" in _err(L)
        assert L.vc_flux_set_monitor(h, 2, log, 0, scratch) == ERR_ARG and "capacity_evals = 0" in _err(L)
        assert _sites(L, h) == []                                            # nothing of the refused calls stuck
        assert L.vc_flux_monitor_bytes(h, 4, None, None) == ERR_STATE and "off" in _err(L)
        assert L.vc_flux_monitor_report(h, None, None, None, None, None) == ERR_STATE and "off" in _err(L)
        assert L.vc_flux_set_monitor(h, 1, log, 4, scratch) == 0
        assert _sites(L, h) == ["v", "x"]
        assert L.vc_flux_set_monitor(h, 2, log, 4, scratch) == 0
        assert _sites(L, h) == ["v", "x", "img_in", "txt_in", "double.0.img", "double.0.txt", "double.1.img", "double.1.txt", "single.0",
                                "single.1"]
        # a truncated name buffer, an index out of range, null / empty buffers
        buf = C.create_string_buffer(8)
        assert L.vc_flux_monitor_sites(h, 4, buf, 8) == 0 and buf.value == b"double."
        assert L.vc_flux_monitor_sites(h, 10, buf, 8) == ERR_ARG and "index = 10" in _err(L) and L.vc_flux_monitor_sites(h, -1, buf, 8) == ERR_ARG
        assert L.vc_flux_monitor_sites(h, 0, None, 8) == ERR_ARG and L.vc_flux_monitor_sites(h, 0, buf, 0) == ERR_ARG
        # the byte sizes are those of the prepared batch: without a prepare there is none
        lb, sb = C.c_int64(0), C.c_int64(0)
        assert L.vc_flux_monitor_bytes(h, 4, C.byref(lb), C.byref(sb)) == ERR_STATE and "vc_flux_prepare" in _err(L)
        assert L.vc_flux_monitor_bytes(h, 0, C.byref(lb), C.byref(sb)) == ERR_ARG
        # nothing was logged yet: the report answers without a device, -1s and no evaluation
        ev, site, b, n = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_int32(7)
        assert L.vc_flux_monitor_report(h, C.byref(ev), C.byref(site), C.byref(b), C.byref(n), None) == 0
        assert (ev.value, site.value, b.value, n.value) == (-1, -1, -1, 0)
        nodes = (C.c_int32 * 3)()
        assert L.vc_flux_step_nodes(h, nodes) == ERR_STATE and "no captured step" in _err(L) and L.vc_flux_step_nodes(h, None) == ERR_ARG
        assert L.vc_flux_set_monitor(h, 0, None, 0, None) == 0 and _sites(L, h) == []
    finally:
        L.vc_flux_destroy(h)


class _Model:
    """stands in for a Flux in the refusals below: records what `monitor` is set to"""

    def __init__(self, monitor=0):
        self.seen = []
        self._monitor = monitor

    monitor = property(lambda self: self._monitor, lambda self, v: (self.seen.append(v), setattr(self, "_monitor", v))[0])


def test_pipeline_switch_is_passed_through_or_refused_never_ignored():
    from visualcloze_amd import pipeline
    args = (None, None, None, [], [], None, None, 0)
    for kw in (dict(use_grid_handle=True), dict(adaptive=dict(rtol=1e-3, atol=1e-6))):
        m = _Model()
        with pytest.raises(ValueError, match=r"generate_grid\(monitor=\.\.\.\)"):
            pipeline.generate_grid(m, *args, monitor=2, **kw)
        assert m.seen == []                                  # refused before anything is touched
    # passed through for the call and put back after it, whatever the call does (no rows: it ends at the first row it asks for)
    m = _Model(1)
    with pytest.raises(IndexError):
        pipeline.generate_grid(m, *args, monitor=2)
    assert m.seen == [2, 1] and m.monitor == 1
    # model.monitor set directly: the grid handle, which drives its own trajectory, refuses instead of ignoring it
    with pytest.raises(ValueError, match="numerics monitor does not log"):
        pipeline._grid_handle(_Model(2), None, None, None, pipeline.NoiseStream(0), "generate_grid")
    with pytest.raises(ValueError, match="numerics monitor does not log"):
        pipeline.generate_grid(_Model(1), *args, use_grid_handle=True, rng=pipeline.NoiseStream(0))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_site_and_log_arithmetic_as_a_sanitized_host_program(tmp_path):
    """csrc/monitor_sites.h needs nothing from HIP: tests/c_abi/monitor_check.cpp (its own main) walks the site lists of six (depth,
    depth_single) configurations through exact-size and truncated name buffers, the byte sizes, and the log's index arithmetic at the
    capacity edges over logs of exactly the computed size - under AddressSanitizer and UBSan.  The program runs directly, on the host."""
    csrc = os.path.join(REPO, "visualcloze_amd", "csrc")
    exe = str(tmp_path / "monitor_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I" + csrc,
           os.path.join(REPO, "tests", "c_abi", "monitor_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "monitor ok" and not r.stderr, r.stdout + r.stderr
