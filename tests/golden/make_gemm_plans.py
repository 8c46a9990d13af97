"""What the GEMM launch planner answers (vc_gemm_plan: CPU only, no launch) over a wide sweep of shapes, epilogues, scratch
states and tile_cfg words -> tests/golden/gemm_plans.json.gz (JSON, gzip: 0.9 MB of text is no diff to read), the table tests/test_host_cpu.py holds the library to
(test_gemm_plans_match_the_recorded_table).  The table pins the planner's behaviour across refactors: it is written ONCE, by the
library of the commit named in its header, and not regenerated when the planner is only rearranged.

    python tests/golden/make_gemm_plans.py            (VC_HIP_LIB=<library of another checkout> to record that one)

Layout (one group per line; tests/helpers.py:gemm_plan_case turns a group + case into VcGemmArgs):
    header   commit, counts, "ws" = the scratch states a case names by index
    groups   {"p": [[M, N, K, {other VcGemmProblem fields}?] ...], "epi", "args": {other VcGemmArgs fields}?,
              "cases": [[tile_cfg, ws, batch, the eight out integers | [return code, vc_last_error() text]] ...]}
The cross product of all axes is ~1e8 cases, so it is thinned: every shape (rows x N x K) appears with tile_cfg 0 with and without
a scratch plus seeded random picks of (tile_cfg word, scratch, batch); every (tile / illegal neighbour) x (flag) pair appears on
six representative shapes; epilogues, the qkv head forms, unequal K and the argument errors have sweeps of their own.
"""
import gzip
import itertools
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.helpers import GEMM_PLAN_WS, gemm_plan_answer, gemm_plan_case  # noqa: E402
from visualcloze_amd import hip  # noqa: E402

T = 512
N_IMG = [1152, 3456, 3240, 4096, 6144, 6912, 14400]      # BASELINE cfg 1, 2, the 3:4 portraits (L = 3752), SDEdit, cfg 3, cfg 5, 5x5
RAGGED = [1, 63, 64, 255, 256, 257, 300, 777, 4095, 4097]
NS = [64, 256, 264, 1024, 3072, 4096, 9216, 12288, 15360, 1056768]
KS = [64, 512, 3072, 4096, 6144, 12288, 15360]
BIAS, GELU, GATE_RES, SILU, QKV = range(5)
WS_NONE, WS_FULL, WS_SMALL = range(3)

TILES = [0, 1, 2, 3, 4, 5, 19, 20, 21, 34, 36] + [6, 17, 18, 33, 35, 37, 48, 49, 63]       # auto, the tests' fixed ones, illegal neighbours
FLAGS = ([0, hip.GEMM_NO_SPLIT, hip.GEMM_NO_SPLITK, hip.GEMM_PERSIST, hip.GEMM_STREAMK, hip.GEMM_PREFER_STREAMK, hip.GEMM_STREAMK_ANY_K]
         + [hip.GEMM_SPLITK(s) for s in range(2, 10)] + [k << 8 for k in (1, 3, 16, 200)])


def row_sets():
    rows = []
    for n in N_IMG:
        for s in (1, 2):                                   # one sample, two samples per GPU
            rows += [[s * (n + T)], [s * n, s * T]]
        rows.append([n, T, n, T])
    return rows + [[m] for m in RAGGED]


def qkv_fields(H, vt, kn, qn, pre=0, rpb=None):
    """the VC_EPI_QKV head-permuted forms (N = 384 H): V^T on / off, key / query norm fused or not"""
    f = {"kn_heads": H, "vt_rpb": rpb or 512, "vt_lpad": 16384}
    if vt:
        f.update(vt=0x1000, vt_col0=256 * H, vt_bstride=128 * H * 16384)
    if kn or qn:
        f.update(kn_rope=0x1000)
    if kn:
        f["kn_scale"] = 0x1000
    if qn:
        f.update(qn_scale=0x1000, qn_prescale=pre)
    return f


def groups():
    rng = random.Random(20261016)
    words = [t | f for t in TILES for f in FLAGS]
    pick = lambda k: [[rng.choice(words) | (rng.choice(FLAGS) if rng.random() < 0.2 else 0), rng.randrange(3), 2 if rng.random() < 0.15 else 0]   # noqa: E731
                      for _ in range(k)]
    # 1. every shape: auto with and without a scratch + random words; the epilogue rotates (the planner tells only QKV apart)
    for i, (Ms, N, K) in enumerate(itertools.product(row_sets(), NS, KS)):
        if len(Ms) == 4 and i % 3:                          # the four-problem row sets: every third (N, K)
            continue
        yield {"p": [[M, N, K] for M in Ms], "epi": i % 5}, [[0, WS_FULL, 0], [0, WS_NONE, 0]] + pick(3)
    # 2. every tile x flag word on six shapes, scratch on offer
    for Ms, N, K, epi in (([3456, T], 3072, 3072, GATE_RES), ([4608], 3072, 15360, GATE_RES), ([6144, T], 3072, 12288, GELU),
                          ([7424], 12288, 3072, GELU), ([300], 264, 4096, BIAS), ([1152, T], 9216, 3072, QKV)):
        yield {"p": [[M, N, K] for M in Ms], "epi": epi}, [[w, WS_FULL, 0] for w in words] + [[w, WS_SMALL, 0] for w in words[::7]]
    # 3. every epilogue, the qkv head forms included, on the FLUX widths
    heads = [dict(H=H, vt=vt, kn=kn, qn=qn, pre=pre) for H in (8, 24) for vt in (0, 1) for kn, qn, pre in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1))]
    for Ms in ([1152, T], [3456, T], [3968], [3752], [4096, T], [6656], [6912, T], [14912], [7936], [777]):
        for K in (3072, 4096):
            for epi in (BIAS, GELU, GATE_RES, SILU, QKV):
                yield {"p": [[M, 3072, K] for M in Ms], "epi": epi}, [[0, WS_FULL, 0], [36, WS_FULL, 0], [hip.GEMM_NO_SPLIT, WS_NONE, 0]] + pick(2)
            yield {"p": [[M, 9216, K, {"vt": 0x1000, "vt_col0": 6144, "vt_rpb": M, "vt_lpad": 16384, "vt_bstride": 3072 * 16384}] for M in Ms], "epi": QKV}, \
                [[0, WS_FULL, 0], [4, WS_NONE, 0]] + pick(2)
            for h in heads:
                yield {"p": [[M, 384 * h["H"], K, qkv_fields(rpb=M, **h)] for M in Ms], "epi": QKV}, \
                    [[0, WS_FULL, 0], [1, WS_FULL, 0], [20, WS_NONE, 0], [34, WS_NONE, 0], [3 << 8, WS_FULL, 0]] + pick(2)
    # 4. grouped problems with unequal K (the remainder schemes need one K)
    for (m0, m1), N, (k0, k1) in itertools.product(([3456, T], [4096, T], [6144, T], [1152, T], [300, 777]), (3072, 4096, 264),
                                                   ((15360, 12288), (3072, 4096), (12288, 64), (6144, 6144))):
        yield {"p": [[m0, N, k0], [m1, N, k1]], "epi": GELU}, \
            [[0, WS_FULL, 0], [0, WS_NONE, 0], [hip.GEMM_STREAMK, WS_FULL, 0], [hip.GEMM_SPLITK(4), WS_FULL, 0], [hip.GEMM_PREFER_STREAMK, WS_FULL, 0]] + pick(2)
    # 5. the argument errors, one case each (and batch > 1 done right)
    ok = [256, 256, 256]
    bad_problem = [
        [0, 256, 256], [256, 256, 60], [256, 12, 256], ok + [{"ldc": 260}], ok + [{"lda": 257}], ok + [{"A": 0}], ok + [{"W": 0}], ok + [{"C": 0}],
        ok + [{"a_rpb": -1}], ok + [{"a_bstride": 4}], ok + [{"c_rpb": 64, "c_bstride": 64 * 512, "ldres": 512}],
        ok + [{"a_rpb": 1, "a_bstride": 1 << 25}], [70000, 256, 256, {"lda": 65536}], [256, 70000, 65536], ok + [{"ldw": 128}], ok + [{"ldw": 260}],
        [65536, 256, 256, {"lda": 40000}], [256, 8, 256, {"ldw": 7500000}],
    ]
    for p in bad_problem:
        yield {"p": [p], "epi": BIAS}, [[0, WS_NONE, 0]]
    yield {"p": [ok, [256, 256, 60]], "epi": BIAS}, [[0, WS_NONE, 0]]
    for f in ({"res": 0}, {"gate": 0}, {"rows_per_batch": 0}, {"ldres": 260}, {"gate_bstride": 4}):
        yield {"p": [ok + [f]], "epi": GATE_RES}, [[0, WS_NONE, 0]]
    yield {"p": [ok], "epi": GATE_RES, "args": {"gate_step_stride": 4}}, [[0, WS_NONE, 0]]
    hp = lambda **over: [256, 384 * 8, 256, {**qkv_fields(8, 1, 1, 1), **over}]      # noqa: E731
    for p in (hp(kn_heads=-8), hp(kn_heads=4), hp(vt_col0=1024), hp(vt_rpb=0), hp(kn_rope=0), hp(vt_row0=-8), hp(kn_rope_bstride=-8),
              hp(qn_scale=0, qn_prescale=1), hp(vt_lpad=256), hp(vt_bstride=8), hp(),
              [256, 3072, 256, {"vt": 0x1000, "vt_rpb": 0}], [256, 3072, 256, {"vt": 0x1000, "vt_rpb": 256, "vt_lpad": 256, "vt_col0": 100}],
              [256, 3072, 256, {"vt": 0x1000, "vt_rpb": 256, "vt_lpad": 256, "vt_col0": 3072}],
              [256, 3072, 256, {"vt": 0x1000, "vt_rpb": 256, "vt_lpad": 256, "vt_col0": 2048, "vt_row0": -1}],
              [256, 3072, 256, {"kn_scale": 0x1000}], [256, 3072, 256, {"qn_prescale": 1}]):
        yield {"p": [p], "epi": QKV}, [[0, WS_NONE, 0]]
    yield {"p": [hp()], "epi": BIAS}, [[0, WS_NONE, 0]]
    for epi in (-1, 5):
        yield {"p": [ok], "epi": epi}, [[0, WS_NONE, 0]]
    for n in (0, 5):
        yield {"p": [ok], "epi": BIAS, "args": {"nprob": n}}, [[0, WS_NONE, 0]]
    yield {"p": [ok], "epi": BIAS}, [[0, WS_NONE, b] for b in (-1, 1, 65535, 65536)]
    yield {"p": [ok], "epi": GELU}, [[0, WS_NONE, 2]]
    for f in ({"a_zstride": 4}, {"w_zstride": -8}, {"c_zstride": 12}, {"a_rpb": 64, "a_bstride": 64 * 256}, {"a_zstride": 1 << 39}, {"w_zstride": 1 << 39},
              {"a_zstride": 65536, "w_zstride": 65536, "c_zstride": 65536}):
        yield {"p": [ok + [f]], "epi": BIAS}, [[t, WS_FULL, 2] for t in (0, 1, 4, 36, hip.GEMM_STREAMK)]


def main():
    lib = hip.lib()
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
    out, n_cases, n_err = [], 0, 0
    for g, cases in groups():
        seen, g["cases"] = set(), []
        for c in cases:
            if tuple(c) in seen:
                continue
            seen.add(tuple(c))
            a, tile_cfg, _ = gemm_plan_case(g, c + [None])
            ans = gemm_plan_answer(lib, a, tile_cfg)
            n_err += len(ans) == 2
            g["cases"].append(c + [ans])
        n_cases += len(g["cases"])
        out.append(g)
    header = {"what": "vc_gemm_plan answers; see tests/golden/make_gemm_plans.py", "commit": commit, "library": os.path.basename(hip.LIB_PATH),
              "abi": lib.vc_abi_version(), "cu_count": 256, "groups": len(out), "cases": n_cases, "error_cases": n_err, "ws": GEMM_PLAN_WS}
    dumps = lambda o: json.dumps(o, separators=(",", ":"))      # noqa: E731
    path = os.path.join(HERE, "gemm_plans.json.gz")
    text = '{"header":' + dumps(header) + ',\n"groups":[\n' + ",\n".join(dumps(g) for g in out) + "\n]}\n"
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:      # (no name, no time: same bytes every run)
        f.write(text.encode())
    print(f"wrote {path}: {len(out)} groups, {n_cases} cases ({n_err} errors), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
