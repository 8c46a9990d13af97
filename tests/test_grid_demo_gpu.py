"""tests/c_abi/grid_demo.c on the GPU: a plain C99 program - no Python in its process - builds the four tiny handles from the
procedural weights this test writes, makes ONE vc_grid_generate call (twice: the second must capture nothing) and writes the rows.
Its file equals, bit for bit, `GridHandle.generate` over the same modules (tests/test_grid_handle_gpu.py holds that to
`pipeline.generate_grid`)."""
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests.grid_demo_build import build_grid_demo
from tests.test_grid_handle_gpu import CFG, ROWS, SEED, STEPS, data, gh, hip, mods  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _raw(t: torch.Tensor) -> bytes:
    t = t.detach().contiguous()
    if t.dtype not in (torch.bfloat16, torch.float32):
        t = t.to(torch.bfloat16)
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes()


def _tensor(f, name: str, w: torch.Tensor, b=None) -> None:
    elem = 4 if w.dtype == torch.float32 else 2
    f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<i", w.dim()) + struct.pack(f"<{w.dim()}q", *w.shape))
    f.write(struct.pack("<i", elem) + _raw(w) + struct.pack("<i", int(b is not None)))
    if b is not None:
        f.write(_raw(b.to(w.dtype)))


def write_demo_input(path, gh, mods, data) -> None:  # noqa: F811
    model, ae, t5, clip = mods
    fh, W = gh.flux, gh.flux.W
    with open(path, "wb") as f:
        f.write(bytes(_flux_config(fh)))
        f.write(struct.pack("<i", len(fh._opts)))
        for k, v in fh._opts.items():
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<i", v))
        recs = [(n, w, W.b.get(n)) for n, w in W.w.items() if not (n.endswith(".linear1.qkv") or n.endswith(".linear1.mlp"))]
        recs += [("modulation", W.mod_w, W.mod_b), ("timestep_freqs", W.temb_freqs.float().reshape(128), None)]
        f.write(struct.pack("<i", len(recs)))
        for n, w, b in recs:
            _tensor(f, n, w, b)
        sd = ae.state_dict()
        names = gh.vae.weight_names()
        f.write(bytes(gh.vae.cfg) + struct.pack("<i", len(names)))
        for n in names:
            _tensor(f, n, sd[n + ".weight"], sd[n + ".bias"])
        for enc, hd in ((t5, gh.t5), (clip, gh.clip)):
            sd = enc.state_dict()
            f.write(bytes(hd.cfg) + struct.pack("<i", len(sd)))
            for k, v in sd.items():
                _tensor(f, k, v)
        f.write(struct.pack("<i", len(ROWS)))
        for (H, Wd), px, m in zip(ROWS, data["rows"], data["masks"]):
            f.write(struct.pack("<2i", H, Wd) + _raw(px) + _raw(m.reshape(H, Wd)) + struct.pack("<i", 1))
        for ids in (data["t5_ids"], data["clip_ids"]):
            a = ids[0].cpu().numpy().astype(np.int32)
            f.write(struct.pack("<i", a.size) + a.tobytes())
        f.write(struct.pack("<2Qf2id", SEED, 5, CFG, STEPS, 0, 1.0))


def _flux_config(fh):
    from visualcloze_amd import hip as H
    import ctypes as C
    p = fh.params
    D = p.hidden_size
    return H.FluxConfig(p.in_channels, p.out_channels, p.vec_in_dim, p.context_in_dim, D, p.num_heads, p.depth, p.depth_single_blocks,
                        int(D * p.mlp_ratio), int(bool(p.guidance_embed)), (C.c_int32 * 3)(*p.axes_dim), int(p.theta))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_host_program_generates_the_grid_bit_identically(hip, gh, mods, data, tmp_path):  # noqa: F811
    exe = build_grid_demo(tmp_path)
    write_demo_input(tmp_path / "in.bin", gh, mods, data)
    want, want_off = gh.generate(data["rows"], data["masks"], data["t5_ids"], data["clip_ids"], SEED, 5, cfg=CFG, steps=STEPS)
    torch.cuda.synchronize()
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint8)
    n = sum(3 * H * W for H, W in ROWS)
    assert raw.size == 4 * n + 8
    got = torch.from_numpy(raw[:4 * n].view(np.float32).copy())
    assert int(raw[4 * n:].view(np.uint64)[0]) == want_off
    o = 0
    for w in want:
        assert torch.equal(got[o:o + w.numel()].reshape(w.shape), w.cpu()) and float(w.std()) > 0
        o += w.numel()
