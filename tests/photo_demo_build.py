"""Builds tests/c_abi/photo_demo.c with gcc as C99 against libvcloze_hip.so (shared by the CPU and the GPU test of the demo)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def build_photo_demo(out_dir) -> str:
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    exe = os.path.join(str(out_dir), "photo_demo")
    libdir = os.path.dirname(hip.LIB_PATH)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(ROCM, "include"),
           os.path.join(REPO, "tests", "c_abi", "photo_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip", "-L" + os.path.join(ROCM, "lib"),
           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def write_handles(f, gh, mods) -> None:
    """the four handles as tests/c_abi/photo_demo.c reads them (the layout tests/c_abi/grid_demo.c reads too): configuration,
    options and weights of the Flux handle, then the autoencoder's, T5's and CLIP's configuration and state dict"""
    import struct
    from tests.test_grid_demo_gpu import _flux_config, _tensor
    _, ae, t5, clip = mods
    fh, W = gh.flux, gh.flux.W
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
