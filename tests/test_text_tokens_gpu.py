"""-m gpu: the T5 and CLIP encoders judged PER TOKEN (tests/tokenview.py) - the composition that `text.py::_run` / `_encode_one` and
csrc/text_engine.hip issue, against the CPU oracle's fp32 run with the oracle's own bf16 run as the yardstick, region by region: the
first and the last row of every 64-row tile, row 0 of the causal block, the rows beside CLIP's pad rows (L = 7 runs as 64 rows, 77 as
128), the distances past T5's last relative-position bucket (L = 192), the EOS row that becomes `pooled`.  Depth prefixes (the first
one / two layers of the same weights) localise a failure to a block.  The bound TOKEN_M comes from the oracle alone (tests/tokenview.py's
docstring; tests/test_tokenview_cpu.py shows what it catches).  Every case prints the worst ratio and its row for every region.
Measured on the MI355X (first run; records, they do not feed TOKEN_M).  T5, TOKEN_M 5: the interior's worst row 1.35 - 2.89 (t5_192
row 19 the largest; prompt-shaped 1.87 - 2.17, depth 1 / 2 2.15 / 2.09, outlier channel 2.34), the first / last rows of the tiles
0.31 - 1.72.  CLIP, TOKEN_M 3: row 0 0.62 - 1.21, the EOS row and `pooled` 0.80 - 1.14, the last live row 0.60 - 1.15, the rest
1.09 - 1.47 (outlier channel the largest).  The handle returns the module's bits.  Width (tests/test_text_gpu.py): XXL-width T5
0.67 - 1.16 at the tile edges and 1.43 inside, CLIP-L 0.96 - 1.21.  Nothing missed its bound; no kernel changed."""
import pytest
import torch

from tests import tokenview as TV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T5_CASES = [n for n in TV.CASES if n.startswith("t5")]
CLIP_CASES = [n for n in TV.CASES if n.startswith("clip")]


@pytest.fixture(scope="module")
def hip():
    from visualcloze_amd import hip as h
    h.require_gpu()
    return h


_MODELS = {}


def model_of(case: TV.Case):
    """the module for the case's configuration, at the case's depth: the first `depth` layers of the same weights (a shallower model
    built from the same state dict - production code is not touched)"""
    from visualcloze_amd.text import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    key = (case.kind, case.wide_positions, case.depth, case.outlier)
    if key not in _MODELS:
        if case.kind == "t5":
            m = T5EncoderModel(T5Config(**dict(case.cfg, **({} if case.depth is None else {"num_layers": case.depth}))))
        else:
            m = CLIPTextModel(CLIPTextConfig(**dict(case.cfg, **({} if case.depth is None else {"num_hidden_layers": case.depth}))))
        sd = TV.state_dict(case)
        m.load_state_dict({k: sd[k] for k in m.state_dict()})
        _MODELS[key] = m.to(DEV).to(torch.bfloat16)
    return _MODELS[key]


def encode(case, through_handle=False):
    """(hidden [L, D], pooled [D] | None) in bf16 on the device, by the module's Python-ordered plan or by the vc_text_* handle"""
    m = model_of(case)
    ids = torch.tensor(case.ids)[None].to(DEV)
    if through_handle:
        from visualcloze_amd.handle import TextHandle
        hs, pooled = TextHandle(m).encode(ids)
    elif case.kind == "t5":
        hs, pooled = m(ids), None
    else:
        pooled, hs = m(ids)
    torch.cuda.synchronize()
    assert hs.dtype == torch.bfloat16 and hs.shape == (1, case.L, hs.shape[-1])
    return hs[0], None if pooled is None else pooled[0]


def judge(name, hs, pooled, what):
    case, regs, runs = TV.oracle_runs(name)
    assert (pooled is None) == (case.kind == "t5")
    got_p = None if pooled is None else pooled.float().cpu()
    return TV.assert_tokens_within_bf16_noise(hs.float().cpu(), runs["o16"][0], runs["o32"][0], regs, f"{name}, {what}", TV.TOKEN_M[case.kind],
                                              pooled=TV.pooled_triple(runs, got_p))


@pytest.mark.parametrize("name", T5_CASES)
def test_t5_tokens(hip, name):
    """one, two and three tiles with random ids and with prompt-shaped ids (n live ids, EOS, pad id 0: hundreds of identical rows and
    tied logits), the two cases with transformers goldens, the depth prefixes and the outlier channel"""
    case = TV.CASES[name]()
    hs, _ = encode(case)
    judge(name, hs, None, "module")


@pytest.mark.parametrize("name", CLIP_CASES)
def test_clip_tokens(hip, name):
    """L = 7 / 24 / 64 / 77 with the EOS first, in the middle, last and followed by EOS padding; `pooled` is judged as a row and is the
    EOS row bit for bit"""
    case = TV.CASES[name]()
    hs, pooled = encode(case)
    assert torch.equal(pooled, hs[case.eos])
    judge(name, hs, pooled, "module")


@pytest.mark.parametrize("name", ["t5_192", "t5_128_prompt", "clip_77_eospad", "clip_7_last"])
def test_tokens_through_the_handle(hip, name):
    """the vc_text_* handle: judged by itself, and bit-identical to the module so that the two paths cannot drift apart unnoticed"""
    case = TV.CASES[name]()
    hs, pooled = encode(case, through_handle=True)
    judge(name, hs, pooled, "handle")
    want_h, want_p = encode(case)
    assert torch.equal(hs, want_h)
    if case.kind == "clip":
        assert torch.equal(pooled, want_p) and torch.equal(pooled, hs[case.eos])
