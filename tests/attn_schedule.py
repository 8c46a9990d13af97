"""The work schedule of the attention tail split, restated in plain Python: integers only, no GPU and no library call.  This is the
single Python statement of the schedule; tests/test_attn_schedule_cpu.py holds it to the partition properties over CU counts no one
machine has, and tests/test_hotpath_gpu.py uses it to find the geometries of each edge class at the device's CU count.

What it mirrors (visualcloze_amd/csrc):
  sched64, chunk_begin     attn_plan.h `sched64`; attention64.hip `chunk_begin64`; attention.hip `chunk_begin`
  plan64, plan32           attn_plan.hip `plan_attention64` / `plan_attention32`: the split rule and the plan words
  whole64, writer64        attention64.hip, both kernels: the `if (split)` block in front of the item loop and the `tu` / `tu_end` walk
                           of the item loop / `next_seg` (piece = blockIdx.x * 2 + (it - it_first), blockIdx.x = slot * 8 + xcd)
  merge64_blocks           `attn64_merge_kernel`: block -> (xcd, it, qb), the search for the first chunk, `next_chunk`, `piece_ptr`
  combine64_tasks          the `if (a.inmerge)` block at the end of `attn64s_kernel`: T = slot; T < 2 * tail; T += W
  decode                   id -> (b, h, query block) as the writers and both merge paths compute it
  whole32, writer32        attention.hip `attn_fwd_kernel<4>` (variant 7): chunk = xcd_remap(blockIdx.x, G), item -> xcd_remap(item, items)
  merge32_blocks           `attn_merge_kernel`: the two `for (cc = c; ...)` loops with their `continue`

Every function takes `mut`, a set of names of deliberate mistakes (MUTATIONS); the test file shows that each one breaks a property.
"""
import functools
from collections import namedtuple

KVB = 64                       # keys per tile
QB64, QB32 = 256, 128          # queries per work item: attention64.hip, attention.hip with 4 waves

# piece_no_xcd       the piece index without its xcd term (writers and readers alike: XCDs then share pieces)
# chunk_ceil         chunk_begin rounding up in the readers (rounding up everywhere is a partition again: the readers must agree
#                    with the writers, not with a formula)
# no_skip_empty      a reader that takes an empty chunk for a piece
# start_even         sched64's `start` as if items were a multiple of 8
MUTATIONS = ("piece_no_xcd", "chunk_ceil", "no_skip_empty", "start_even")

Sched = namedtuple("Sched", "W start n rounds tail units")
Geom = namedtuple("Geom", "B L H n_cu qblocks items nkt G")


def geom(B, L, H, n_cu, family):
    """family 64: attention64.hip (variants 12 / 28), one workgroup per CU; family 32: attention.hip variant 7, two per CU"""
    qb = QB64 if family == 64 else QB32
    qblocks = (L + qb - 1) // qb
    return Geom(B, L, H, n_cu, qblocks, qblocks * H * B, (L + KVB - 1) // KVB, n_cu if family == 64 else 2 * n_cu)


def chunk_begin(c, units, chunks):
    return (c * units) // chunks


def _cb_read(c, units, chunks, mut):
    return -((-c * units) // chunks) if "chunk_ceil" in mut else chunk_begin(c, units, chunks)


def xcd_remap(bid, nb):
    q, r = nb >> 3, nb & 7
    xcd, idx = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


@functools.lru_cache(maxsize=1 << 14)
def sched64(x, G, items, nkt, mut=()):
    W = G >> 3
    q, r = items >> 3, items & 7
    n = q + (1 if x < r else 0)
    start = x * (q + 1) if x < r else r * (q + 1) + (x - r) * q
    if "start_even" in mut:
        start = x * q
    rounds = n // W
    tail = n - rounds * W
    return Sched(W, start, n, rounds, tail, tail * nkt)


def decode(id_, qblocks, H):
    """(b, h, query block) of a logical item"""
    bh = id_ // qblocks
    return bh // H, bh % H, id_ % qblocks


# ---------------------------------------------------------------- the planner's rule
def plan64(g):
    """None where plan_attention64 does not split (given the tail-split bit, no kv_len and the whole scratch), else the plan words it
    reports: full_rounds / tail_items / tail_units are whole-grid figures that the kernels do not read beyond full_rounds >= 0 (the
    schedule is per XCD); merge_grid is that of variant 12 (variant 28, stream form: 0, the pieces are combined in the launch)."""
    if g.G % 8:
        return None
    sc = [sched64(x, g.G, g.items, g.nkt) for x in range(8)]
    tail_slots = max(s.tail for s in sc)
    worst_split = max((s.tail * g.nkt + s.W - 1) // s.W for s in sc)
    if not (tail_slots > 0 and worst_split + 4 < g.nkt):
        return None
    full = g.items // g.G
    tail = g.items - full * g.G
    return {"full_rounds": full, "tail_items": tail, "tail_units": tail * g.nkt, "merge_grid": 16 * tail_slots, "worst_split": worst_split}


def plan32(g):
    rounds = g.items // g.G
    tail = g.items - rounds * g.G
    split_tiles = (tail * g.nkt + g.G - 1) // g.G
    if not (tail > 0 and split_tiles + 3 < g.nkt):
        return None
    return {"full_rounds": rounds, "tail_items": tail, "tail_units": tail * g.nkt, "merge_grid": tail, "worst_split": split_tiles}


# ---------------------------------------------------------------- writers
def _walk(tu, tu_end, nkt, piece0):
    """the segment walk both families share: [(tail item, first tile, tile past the last, piece index or -1 = written to out)]"""
    it_first = tu // nkt
    segs = []
    while tu < tu_end:
        it = tu // nkt
        kt0 = tu - it * nkt
        kt1 = min(nkt, kt0 + (tu_end - tu))
        tu += kt1 - kt0
        segs.append((it, kt0, kt1, piece0 + (it - it_first) if kt1 - kt0 != nkt else -1))
    return segs


def whole64(g, xcd, slot, mut=()):
    """ids of the whole items of workgroup slot * 8 + xcd"""
    sc = sched64(xcd, g.G, g.items, g.nkt, mut)
    return [sc.start + slot + r * sc.W for r in range(sc.rounds)]


def tail_id64(g, xcd, it, mut=()):
    sc = sched64(xcd, g.G, g.items, g.nkt, mut)
    return sc.start + sc.rounds * sc.W + it


def writer64(g, xcd, slot, mut=()):
    sc = sched64(xcd, g.G, g.items, g.nkt, mut)
    block = slot * 8 + (0 if "piece_no_xcd" in mut else xcd)
    return _walk(chunk_begin(slot, sc.units, sc.W), chunk_begin(slot + 1, sc.units, sc.W), g.nkt, block * 2)


def whole32(g, block):
    rounds = g.items // g.G
    return [xcd_remap(block + seg * g.G, g.items) for seg in range(rounds)]


def tail_id32(g, it):
    return xcd_remap((g.items // g.G) * g.G + it, g.items)


def writer32(g, block):
    units = (g.items - (g.items // g.G) * g.G) * g.nkt
    chunk = xcd_remap(block, g.G)
    return _walk(chunk_begin(chunk, units, g.G), chunk_begin(chunk + 1, units, g.G), g.nkt, chunk * 2)


# ---------------------------------------------------------------- readers
def _first_chunk(u0, units, chunks, mut):
    c = (u0 * chunks) // units
    while c > 0 and _cb_read(c, units, chunks, mut) > u0:
        c -= 1
    while c + 1 < chunks and _cb_read(c + 1, units, chunks, mut) <= u0:
        c += 1
    return c


@functools.lru_cache(maxsize=1 << 12)
def _pieces64(it, xcd, sc, nkt, mut):
    """the piece list of tail item `it` of an XCD, in the order the 64-query readers fold it; None = the early exit `the whole item
    ran inside one chunk`"""
    cb = lambda c: _cb_read(c, sc.units, sc.W, mut)  # noqa: E731
    u0 = it * nkt
    u1 = u0 + nkt
    c = _first_chunk(u0, sc.units, sc.W, mut)
    if cb(c + 1) >= u1:
        return None

    def next_chunk(cc):
        while "no_skip_empty" not in mut and cc < sc.W and cb(cc) < u1 and cb(cc + 1) == cb(cc):
            cc += 1
        return cc if cc < sc.W and cb(cc) < u1 else -1
    out = []
    cc = next_chunk(c)
    while cc >= 0:
        out.append((cc * 8 + (0 if "piece_no_xcd" in mut else xcd)) * 2 + (it - cb(cc) // nkt))
        cc = next_chunk(cc + 1)
    return tuple(out)


def merge64_blocks(g, merge_grid, mut=()):
    """attn64_merge_kernel: {block: (xcd, it, qb, piece list or None)} for the blocks that do not return at `it >= sc.tail`"""
    out = {}
    for blk in range(merge_grid):
        xcd, it, qb = blk & 7, blk >> 4, (blk >> 3) & 1
        sc = sched64(xcd, g.G, g.items, g.nkt, mut)
        if it < sc.tail:
            out[blk] = (xcd, it, qb, _pieces64(it, xcd, sc, g.nkt, mut))
    return out


def combine64_tasks(g, xcd, slot, mut=()):
    """the in-launch combine of workgroup slot * 8 + xcd: [(it, qb, piece list or None, flag words read and cleared)].  EVERY workgroup
    runs it (attn64s_combine), also one whose chunk is empty and that has no whole item: with units < W such a workgroup owns tasks."""
    sc = sched64(xcd, g.G, g.items, g.nkt, mut)
    out = []
    for T in range(slot, 2 * sc.tail, sc.W):
        it, qb = T >> 1, T & 1
        pcs = _pieces64(it, xcd, sc, g.nkt, mut)
        out.append((it, qb, pcs, None if pcs is None else tuple(p * 2 + qb for p in pcs)))
    return out


def flags_set64(segs):
    """the flag words a stream-form writer publishes: both query blocks of each piece"""
    return [p * 2 + qb for (_, _, _, p) in segs if p >= 0 for qb in (0, 1)]


def merge32_blocks(g, merge_grid, mut=()):
    """attn_merge_kernel: {block = tail item: piece list or None}"""
    units = (g.items - (g.items // g.G) * g.G) * g.nkt
    cb = lambda c: _cb_read(c, units, g.G, mut)  # noqa: E731
    out = {}
    for it in range(merge_grid):
        u0 = it * g.nkt
        u1 = u0 + g.nkt
        c = _first_chunk(u0, units, g.G, mut)
        if cb(c + 1) >= u1:
            out[it] = None
            continue
        pcs = []
        cc = c
        while cc < g.G and cb(cc) < u1:
            if "no_skip_empty" in mut or cb(cc + 1) != cb(cc):
                pcs.append(cc * 2 + (it - cb(cc) // g.nkt))
            cc += 1
        out[it] = tuple(pcs)
    return out


# ---------------------------------------------------------------- edge classes
def max_pieces(g, family):
    """the most pieces any tail item is cut into (the writers' count)"""
    n = {}
    if family == 64:
        for xcd in range(8):
            for slot in range(g.G >> 3):
                for it, _, _, p in writer64(g, xcd, slot):
                    n[(xcd, it)] = n.get((xcd, it), 0) + (p >= 0)
    else:
        for blk in range(g.G):
            for it, _, _, p in writer32(g, blk):
                n[it] = n.get(it, 0) + (p >= 0)
    return max(n.values())


def classes(B, L, H, n_cu, family):
    """The edge classes of a geometry's tail split (empty set: the planner does not split):
      uneven / even        items & 7 != 0: sched64's n, start, rounds and tail differ between XCDs / items & 7 == 0
      xcd_without_tail     some XCD has tail items and some XCD has none
      empty_chunks         fewer (item, tile) units than workgroups: family 64 per XCD (0 < units < W), family 32 over the grid
      tail_sample_ge1      a tail item belongs to sample b >= 1
      pieces_ge_9          an item is cut into 9 or more pieces (three batches of the in-launch combine's MAXP = 4)
      pieces_eq_W          an item is cut into W pieces, the most there can be (family 64)
      behind_whole_round   the tail follows at least one round of whole items (family 64: on an XCD that has a tail)
      batch                B > 1"""
    g = geom(B, L, H, n_cu, family)
    out = set()
    if family == 64:
        if plan64(g) is None:
            return out
        sc = [sched64(x, g.G, g.items, g.nkt) for x in range(8)]
        out.add("uneven" if g.items & 7 else "even")
        if any(s.tail == 0 for s in sc):
            out.add("xcd_without_tail")
        if any(0 < s.units < s.W for s in sc):
            out.add("empty_chunks")
        if any(s.tail and s.rounds for s in sc):
            out.add("behind_whole_round")
        ids = [tail_id64(g, x, it) for x in range(8) for it in range(sc[x].tail)]
        mp = max_pieces(g, 64)
        if mp == g.G >> 3:
            out.add("pieces_eq_W")
    else:
        p = plan32(g)
        if p is None:
            return out
        if p["tail_units"] < g.G:
            out.add("empty_chunks")
        if p["full_rounds"] > 0:
            out.add("behind_whole_round")
        ids = [tail_id32(g, it) for it in range(p["tail_items"])]
        mp = max_pieces(g, 32)
    if mp >= 9:
        out.add("pieces_ge_9")
    if any(decode(i, g.qblocks, H)[0] >= 1 for i in ids):
        out.add("tail_sample_ge1")
    if B > 1:
        out.add("batch")
    return out
