"""The host statement of the library's fixed-order sum (csrc/block_reduce.h is the device's): what vc_fm_loss, vc_rk_error_ratio,
vc_tensor_stats and vc_residual_change promise in include/vcloze_hip.h, restated in torch so that a CPU computation gives the
kernels' bits."""
import torch

THREADS = 256        # threads of a block = the most blocks of pass 1: pass 2 holds one block sum per thread


def _tree(v: torch.Tensor) -> torch.Tensor:
    """block_tree over the last dimension (THREADS entries): l[t] = l[t] + l[t + o] for t < o, o = 128, 64, .., 1 -> l[0]"""
    o = THREADS // 2
    while o >= 1:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def ordered_sum(terms: torch.Tensor, units_total=None, max_blocks: int = THREADS) -> torch.Tensor:
    """The sum of the already-formed addends `terms` [units, E] (CPU, f32 or f64) of ONE sample, in its dtype, in the kernels' order.
    A unit is what a thread takes at a time: E = 8 elements of a bf16 row, 4 of an f32 row, 1 for vc_rk_error_ratio.  The units are
    dealt round-robin to the nblk * 256 threads of nblk = min(ceil(units_total / 256), max_blocks) blocks - `units_total` where the
    grid is sized by more units than are summed (vc_fm_loss: all rows size it, the valid ones are summed) - and a thread adds the
    elements of its units in ascending order; the 256 sums of a block go down the tree, the nblk block sums down the same tree.
    A unit shorter than E is padded with zeros, as is a thread without a unit: x + 0 = x leaves every sum as it is."""
    assert terms.dim() == 2 and terms.dtype in (torch.float32, torch.float64) and max_blocks <= THREADS
    units, E = terms.shape
    nblk = min(((units if units_total is None else units_total) + THREADS - 1) // THREADS, max_blocks)
    T = nblk * THREADS
    rounds = max(-(-units // T), 1)
    pad = torch.zeros(rounds * T, E, dtype=terms.dtype)
    pad[:units] = terms.detach()
    pad = pad.view(rounds, T, E)
    s = torch.zeros(T, dtype=terms.dtype)
    for r in range(rounds):
        for e in range(E):
            s = s + pad[r, :, e]
    part = torch.zeros(THREADS, dtype=terms.dtype)
    part[:nblk] = _tree(s.view(nblk, THREADS))
    return _tree(part)
