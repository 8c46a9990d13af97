"""Builds tests/c_abi/torch_noise_demo.c with gcc as C99 against libvcloze_hip.so (shared by the CPU and the GPU test of the demo)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def build_torch_noise_demo(out_dir) -> str:
    from visualcloze_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    exe = os.path.join(str(out_dir), "torch_noise_demo")
    libdir = os.path.dirname(hip.LIB_PATH)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-isystem", os.path.join(ROCM, "include"),
           os.path.join(REPO, "tests", "c_abi", "torch_noise_demo.c"), "-o", exe, "-L" + libdir, "-lvcloze_hip", "-L" + os.path.join(ROCM, "lib"),
           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe
