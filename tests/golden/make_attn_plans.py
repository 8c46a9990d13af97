"""What the attention launch planner answers (vc_attention_plan: CPU only, no launch) over a sweep of geometries, CU counts,
variant words, masks, scratch states, query forms, logit bounds and strides -> tests/golden/attn_plans.json.gz (JSON, gzip), the
table tests/test_host_cpu.py holds the library to (test_attention_plans_match_the_recorded_table).  The table pins every launch
decision across refactors: it is written ONCE, by the library its header names, and not regenerated when the planner is only
rearranged.  This one was recorded from the commit BEFORE the planner existed, through a recording shim: the two launch functions
of that commit filled the sixteen integers from the values their own decision lines computed and returned before the first HIP call.

    python tests/golden/make_attn_plans.py            (VC_HIP_LIB=<library of another checkout> to record that one;
                                                       VC_PLAN_COMMIT / VC_PLAN_NOTE name it in the header)

Layout (one group per line; tests/helpers.py:attn_plan_case turns a group + case into a VcAttention):
    header   commit, how it was recorded, counts
    groups   {"B", "L", "H", "n_cu", "o": {other VcAttention fields}?,
              "cases": [[variant, mask, scratch state, query form, logit_bound, the sixteen out integers | [return code, vc_last_error() text]] ...]}
The cross product of all axes is ~1e9 cases, so it is thinned: every (L, H, B, n_cu) appears with every variant word in the form the
product launches it, plus seeded random picks of (variant, mask, scratch, query form, bound); every variant x scratch state x mask,
and every variant x query form x bound, appear on the BASELINE geometries; the strides and the argument errors have sweeps of their own.
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

from tests.helpers import attn_plan_answer, attn_plan_case  # noqa: E402
from visualcloze_amd import hip  # noqa: E402

LS = [1, 15, 16, 40, 63, 64, 65, 255, 256, 257, 333, 1664, 3752, 3968, 4608, 6656, 7424, 14912]
HS = [1, 2, 3, 8, 24]
BS = [1, 2, 4]
CUS = [256, 304, 64, 8, 7, 1]
VARIANTS = [0, 1, 2, 3, 7, 8, 12, 28] + [4, 5, 6, 20, 24]          # the ones in use, the illegal neighbours
MASKS = [0, 1, 3, 2]                                               # none, kv_len, kv_len + kv_gap, kv_gap alone (an error)
SCRATCH = range(6)                                                 # tests/helpers.py:attn_scratch_states
WHOLE = 4
QFORMS = range(16)                                                 # bits: q_scale, q_scale2, rope, q_prescaled
QPRE = 8
BOUNDS = [0.0, 0.5, 16.65, 100.0, 100.00000762939453, 1e30]        # (the float above 100)


def product_form(v):
    """the case the host engines launch variant v as: whole scratch, no mask, prescaled queries + the model's bound where attention64 runs"""
    return [v, 0, WHOLE, QPRE if v & 8 else 0, 16.65 if v & 8 else 0.0]


def groups():
    rng = random.Random(20261018)
    pick = lambda k: [[rng.choice(VARIANTS), rng.choice(MASKS[:3]) if rng.random() < 0.9 else 2, rng.choice(SCRATCH),       # noqa: E731
                       rng.choice((0, QPRE, QPRE, 5, 7)) if rng.random() < 0.9 else rng.choice(QFORMS), rng.choice(BOUNDS)] for _ in range(k)]
    # 1. every geometry x CU count: every variant word as the product launches it (the illegal neighbours at 256 CUs) + random picks
    for L, H, B, n_cu in itertools.product(LS, HS, BS, CUS):
        yield {"B": B, "L": L, "H": H, "n_cu": n_cu}, [product_form(v) for v in (VARIANTS if n_cu == 256 else VARIANTS[:8])] + pick(2)
    # 2. BASELINE geometries (cfg 1, 2, 3, 5, 5x5) and a ragged one: variant x scratch x mask; variant x query form; query form x bound
    for (B, L), n_cu in itertools.product(((1, 1664), (1, 3968), (2, 3968), (1, 6656), (1, 7424), (1, 14912), (4, 257)), (256, 7)):
        yield {"B": B, "L": L, "H": 24, "n_cu": n_cu}, [[v, m, s, QPRE if v & 8 else 0, 16.65] for v in VARIANTS for m in MASKS for s in SCRATCH]
    for B, L in ((1, 1664), (1, 3968), (1, 7424), (4, 257)):
        yield {"B": B, "L": L, "H": 24, "n_cu": 256}, ([[v, 0, WHOLE, q, 16.65] for v in VARIANTS for q in QFORMS] +
                                                       [[v, 0, WHOLE, q, b] for v in (3, 8, 12, 28) for q in QFORMS for b in BOUNDS])
    # 3. strides on both sides of each 32-bit condition (variants 12 / 28 prescaled: the stream form where the operands fit), alignment, Lpad
    forms = [[v, 0, WHOLE, q, 16.65] for v in (3, 7, 8, 12, 28) for q in (0, QPRE)]
    g = lambda B, L, H, **o: {"B": B, "L": L, "H": H, "n_cu": 256, "o": o}      # noqa: E731
    for grp in (g(1, 4608, 24, bstride=2105007096), g(1, 4608, 24, bstride=2105007104),                # fits32: the qkv rows
                g(4, 14912, 24, Lpad=174720), g(4, 14912, 24, Lpad=174784),                            # fits32: V^T
                g(1, 14912, 1, ld=143392), g(1, 14912, 1, ld=143400),                                  # K rows of one sample
                g(1, 333, 1, Lpad=(1 << 24) - 64, ld=120), g(1, 333, 1, Lpad=(1 << 24) - 64, ld=128), g(1, 333, 1, Lpad=1 << 24, ld=8),
                g(1, 3968, 24, ld=9220), g(1, 3968, 24, ldo=3074), g(1, 3968, 24, ldo=3076), g(1, 3968, 24, bstride=3968 * 9216 + 4),
                g(1, 3968, 24, ld=9224, bstride=3968 * 9224 + 8, ldo=15360, out_bstride=3968 * 15360),
                g(1, 333, 8, Lpad=320), g(1, 333, 8, Lpad=400), g(1, 333, 8, Lpad=448), g(1, 64, 8, Lpad=0),
                g(1, 3968, 24, qkv=0), g(1, 3968, 24, vt=0), g(1, 3968, 24, out=0),
                g(0, 3968, 24), g(1, 0, 24), g(1, 3968, 0), g(-1, 3968, 24), g(1, 3968, 24, qkv=0, Lpad=100)):
        yield grp, forms


def main():
    lib = hip.lib()
    commit = os.environ.get("VC_PLAN_COMMIT") or subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
    out, n_cases, n_err = [], 0, 0
    for g, cases in groups():
        seen, g["cases"] = set(), []
        for c in cases:
            if tuple(c) in seen:
                continue
            seen.add(tuple(c))
            a, n_cu, _ = attn_plan_case(g, c + [None])
            ans = attn_plan_answer(lib, a, n_cu)
            n_err += len(ans) == 2
            g["cases"].append(c + [ans])
        n_cases += len(g["cases"])
        out.append(g)
    header = {"what": "vc_attention_plan answers; see tests/golden/make_attn_plans.py", "commit": commit,
              "recorded_by": os.environ.get("VC_PLAN_NOTE", "the library of that commit"), "library": os.path.basename(hip.LIB_PATH),
              "abi": lib.vc_abi_version(), "groups": len(out), "cases": n_cases, "error_cases": n_err}
    dumps = lambda o: json.dumps(o, separators=(",", ":"))      # noqa: E731
    path = os.path.join(HERE, "attn_plans.json.gz")
    text = '{"header":' + dumps(header) + ',\n"groups":[\n' + ",\n".join(dumps(g) for g in out) + "\n]}\n"
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:      # (no name, no time: same bytes every run)
        f.write(text.encode())
    print(f"wrote {path}: {len(out)} groups, {n_cases} cases ({n_err} errors), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
