"""CPU: the attention tail-split schedule (tests/attn_schedule.py, restated from the kernels) as a partition, at CU counts from 8 to
320 - the GPU tests can only ever run one - and four deliberate mistakes that the properties catch."""
from collections import Counter

import pytest

from tests import attn_schedule as S

N_CUS = list(range(8, 321, 8))
BS = (1, 2, 3)
HS = (1, 2, 3, 5, 7, 8, 9, 11, 24)
# on and off the 64-key tile and the 256-query item; 321 / 257: the shortest rows the 64- / 32-query planner ever splits (6 / 5 tiles)
LS = (257, 320, 321, 513, 769, 1985, 2049, 3968, 8000)


def sweep():
    for n_cu in N_CUS:
        for B in BS:
            for H in HS:
                for L in LS:
                    yield B, L, H, n_cu


def tiles_once(segs, nkt):
    """[(kt0, kt1)] cover 0 .. nkt - 1 exactly once"""
    at = 0
    for kt0, kt1 in sorted(segs):
        if kt0 != at or kt1 <= kt0:
            return False
        at = kt1
    return at == nkt


def covers_once(ids, g):
    """the logical items are 0 .. items - 1, each once, and so are their (b, h, query block)"""
    if sorted(ids) != list(range(g.items)):
        return False
    dec = [S.decode(i, g.qblocks, g.H) for i in ids]
    return all(0 <= b < g.B and 0 <= h < g.H and 0 <= q < g.qblocks for b, h, q in dec) and len(set(dec)) == g.items


def violations64(g, mut=()):
    """the names of the properties a split geometry of the 64-query family breaks (none: [])"""
    bad = set()
    W = g.G >> 3
    sc = [S.sched64(x, g.G, g.items, g.nkt, mut) for x in range(8)]
    ids, segs_of, flags_set, piece_writers = [], {}, Counter(), Counter()
    for xcd in range(8):
        ids += [S.tail_id64(g, xcd, it, mut) for it in range(sc[xcd].tail)]
        for slot in range(W):
            ids += S.whole64(g, xcd, slot, mut)
            segs = S.writer64(g, xcd, slot, mut)
            if sum(p >= 0 for _, _, _, p in segs) > 2:
                bad.add("a workgroup writes more than two pieces")
            for it, kt0, kt1, p in segs:
                segs_of.setdefault((xcd, it), []).append((kt0, kt1, p))
                if p < 0:
                    bad.add("a whole tail item inside one chunk")
                elif not 0 <= p < 2 * g.n_cu:
                    bad.add("piece index outside the scratch")
                if p >= 0:
                    piece_writers[p] += 1
            flags_set.update(S.flags_set64(segs))
    if not covers_once(ids, g):
        bad.add("items not covered exactly once")
    want = {(x, it) for x in range(8) for it in range(sc[x].tail)}
    if set(segs_of) != want or not all(tiles_once([(a, b) for a, b, _ in v], g.nkt) for v in segs_of.values()):
        bad.add("a (tail item, key tile) not written exactly once")
    if any(n != 1 for n in piece_writers.values()) or any(n != 1 for n in flags_set.values()):
        bad.add("a piece or flag word with two writers")
    in_key_order = {k: tuple(p for _, _, p in sorted(v)) for k, v in segs_of.items()}
    # attn64_merge_kernel behind variant 12's launch
    blocks = S.merge64_blocks(g, S.plan64(g)["merge_grid"], mut)
    if sorted((x, it, qb) for x, it, qb, _ in blocks.values()) != sorted((x, it, qb) for x, it in want for qb in (0, 1)):
        bad.add("merge grid: a task without exactly one block")
    for x, it, qb, pcs in blocks.values():
        if pcs is None:
            bad.add("reader takes the early exit")
        elif pcs != in_key_order.get((x, it)):
            bad.add("merge kernel: piece list differs from the writers'")
    # the in-launch combine of variant 28
    owners, cleared = Counter(), Counter()
    for xcd in range(8):
        for slot in range(W):
            for it, qb, pcs, flags in S.combine64_tasks(g, xcd, slot, mut):
                owners[(xcd, it, qb)] += 1
                if pcs is None:
                    bad.add("reader takes the early exit")
                    continue
                if pcs != in_key_order.get((xcd, it)):
                    bad.add("in-launch combine: piece list differs from the writers'")
                cleared.update(flags)
    if owners != Counter({(x, it, qb): 1 for x, it in want for qb in (0, 1)}):
        bad.add("in-launch combine: a task without exactly one owner")
    if cleared != flags_set:
        bad.add("a flag word not set once and cleared once")
    return sorted(bad)


def violations32(g, mut=()):
    """the same for variant 7 (attention.hip, G = 2 n_cu workgroups, chunks over the whole grid, no flags)"""
    bad = set()
    p = S.plan32(g)
    ids, segs_of, piece_writers = [S.tail_id32(g, it) for it in range(p["tail_items"])], {}, Counter()
    for blk in range(g.G):
        ids += S.whole32(g, blk)
        segs = S.writer32(g, blk)
        if sum(pc >= 0 for _, _, _, pc in segs) > 2:
            bad.add("a workgroup writes more than two pieces")
        for it, kt0, kt1, pc in segs:
            segs_of.setdefault(it, []).append((kt0, kt1, pc))
            if pc < 0:
                bad.add("a whole tail item inside one chunk")
            elif not 0 <= pc < 4 * g.n_cu:         # 2 pieces per workgroup, 2 workgroups per CU (attention_flags_offset)
                bad.add("piece index outside the scratch")
            if pc >= 0:
                piece_writers[pc] += 1
    if not covers_once(ids, g):
        bad.add("items not covered exactly once")
    if sorted(segs_of) != list(range(p["tail_items"])) or not all(tiles_once([(a, b) for a, b, _ in v], g.nkt) for v in segs_of.values()):
        bad.add("a (tail item, key tile) not written exactly once")
    if any(n != 1 for n in piece_writers.values()):
        bad.add("a piece or flag word with two writers")
    blocks = S.merge32_blocks(g, p["merge_grid"], mut)
    if sorted(blocks) != list(range(p["tail_items"])):
        bad.add("merge grid: a task without exactly one block")
    for it, pcs in blocks.items():
        if pcs is None:
            bad.add("reader takes the early exit")
        elif pcs != tuple(pc for _, _, pc in sorted(segs_of.get(it, []))):
            bad.add("merge kernel: piece list differs from the writers'")
    return sorted(bad)


def library_plan(lib, B, L, H, n_cu, variant):
    from tests.helpers import attn_plan_answer, attn_plan_case
    WHOLE, QPRE = 4, 8               # scratch state / query form of tests/helpers.py:attn_plan_case
    a, n_cu, _ = attn_plan_case({"B": B, "L": L, "H": H, "n_cu": n_cu}, [variant, 0, WHOLE, QPRE if variant & 8 else 0, 16.0, None])
    return attn_plan_answer(lib, a, n_cu)


def test_tail_split_schedule_is_a_partition_at_every_cu_count():
    """Over n_cu = 8 .. 320 (multiples of 8), B = 1 .. 3, nine head counts and nine lengths, wherever vc_attention_plan splits: the
    plan words equal the restatement's; every (tail item, key tile) has one writer; a workgroup writes at most two pieces, each inside
    the scratch; attn64_merge_kernel's and the in-launch combine's piece lists are the writers' pieces in key order (variant 7:
    attn_merge_kernel's); every flag word is set once and cleared once, every task has one owner, one merge block; all items decode
    to every (b, h, query block) once.  The readers' early exit `the whole item ran inside one chunk` is UNREACHABLE from the planner:
    it splits only where the longest chunk, worst_split, is more than 4 tiles (variant 7: 3) shorter than an item, so no chunk holds a
    whole item - asserted here as `no writer segment is a whole item and no reader returns early`, in place of a GPU shape."""
    from visualcloze_amd import hip
    lib = hip.lib()
    n = {64: 0, 32: 0}
    seen, checked = set(), set()
    for B, L, H, n_cu in sweep():
        for family, variants in ((64, (12, 28)), (32, (7,))):
            g = S.geom(B, L, H, n_cu, family)
            p = (S.plan64 if family == 64 else S.plan32)(g)
            for v in variants:
                got = library_plan(lib, B, L, H, n_cu, v)
                assert len(got) == 16 and got[6:8] == [g.qblocks, g.items], (B, L, H, n_cu, v, got)
                if p is None:
                    assert got[8:13] == [-1, 0, 0, 0, 0], (B, L, H, n_cu, v, got)
                else:
                    assert got[3] == g.G and got[8:11] == [p["full_rounds"], p["tail_items"], p["tail_units"]], (B, L, H, n_cu, v, got, p)
                    assert got[11:13] == ([1, 0] if v == 28 else [0, p["merge_grid"]]), (B, L, H, n_cu, v, got, p)
            if p is None:
                continue
            assert p["worst_split"] < g.nkt
            n[family] += 1
            if (family, n_cu, g.items, g.nkt) in checked:      # the schedule reads B, L and H through items and nkt alone: (2, L, 3) is (3, L, 2)
                assert covers_once(range(g.items), g), (family, B, L, H, n_cu)
                continue
            checked.add((family, n_cu, g.items, g.nkt))
            bad = (violations64 if family == 64 else violations32)(g)
            assert not bad, (family, B, L, H, n_cu, bad)
            if n_cu in (64, 256):
                seen |= {(family, c) for c in S.classes(B, L, H, n_cu, family)}
    print(f"tail-split sweep: {n[64]} split geometries of the 64-query family, {n[32]} of variant 7, {len(checked)} distinct schedules")
    assert n[64] >= 1000 and n[32] >= 1000
    # the sweep reaches every edge class
    assert {(64, c) for c in ("uneven", "even", "xcd_without_tail", "empty_chunks", "tail_sample_ge1", "pieces_ge_9", "pieces_eq_W",
                              "behind_whole_round", "batch")} | {(32, c) for c in ("empty_chunks", "tail_sample_ge1", "pieces_ge_9",
                                                                                   "behind_whole_round", "batch")} <= seen


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_schedule_properties_catch_a_mutated_restatement(mutation):
    """The properties are not vacuous: the piece index without its xcd term, chunk_begin rounding up in the readers, a reader that
    does not skip empty chunks, and `start` computed as if items were a multiple of 8 each break at least one of them on the sweep."""
    broken = {}
    for B, L, H, n_cu in sweep():
        if n_cu not in (8, 64):
            continue
        for family in (64, 32):
            g = S.geom(B, L, H, n_cu, family)
            if (S.plan64 if family == 64 else S.plan32)(g) is None:
                continue
            for b in (violations64 if family == 64 else violations32)(g, (mutation,)):
                broken.setdefault(b, (family, B, L, H, n_cu))
    print(mutation, "breaks", broken)
    assert broken, mutation
    expected = {"piece_no_xcd": "a piece or flag word with two writers", "chunk_ceil": "merge kernel: piece list differs from the writers'",
                "no_skip_empty": "in-launch combine: piece list differs from the writers'", "start_even": "items not covered exactly once"}
    assert expected[mutation] in broken, broken


def test_classes_at_256_cus():
    """the geometries tests/test_hotpath_gpu.py resolves to on a 256-CU device, worked out from the schedule by hand: (1, 321, 1) is
    2 items of 6 tiles on XCDs 0 and 1, one tile per piece, 26 of 32 chunks empty; (1, 513, 1) is 3 items of 9 one-tile pieces;
    (1, 1985, 1) is one item of 32 tiles per XCD, a tile per workgroup; (3, 2049, 11) is 297 items = 38 on XCD 0 and 37 on the others,
    one round of 32 and 6 / 5 tail items; (3, 769, 24) is 288 = 36 per XCD; variant 7 at L = 257 has 3 B items of 5 tiles on 512 chunks"""
    assert {"uneven", "xcd_without_tail", "empty_chunks"} <= S.classes(1, 321, 1, 256, 64) and not S.classes(1, 320, 1, 256, 64)
    assert "tail_sample_ge1" in S.classes(2, 321, 1, 256, 64) and "tail_sample_ge1" not in S.classes(1, 321, 1, 256, 64)
    assert S.max_pieces(S.geom(1, 321, 1, 256, 64), 64) == 6 and S.max_pieces(S.geom(1, 513, 1, 256, 64), 64) == 9
    assert {"uneven", "pieces_ge_9"} <= S.classes(1, 513, 1, 256, 64) and "pieces_ge_9" not in S.classes(1, 512, 1, 256, 64)
    assert "pieces_eq_W" in S.classes(1, 1985, 1, 256, 64) and "pieces_eq_W" not in S.classes(1, 1984, 1, 256, 64)
    assert {"uneven", "behind_whole_round", "batch", "tail_sample_ge1"} <= S.classes(3, 2049, 11, 256, 64)
    assert [S.sched64(x, 256, 297, 33)[2:5] for x in (0, 1, 7)] == [(38, 1, 6), (37, 1, 5), (37, 1, 5)]
    assert {"even", "behind_whole_round", "batch"} <= S.classes(3, 769, 24, 256, 64)
    assert "empty_chunks" in S.classes(1, 257, 1, 256, 32) and not S.classes(1, 256, 1, 256, 32)
    assert {"empty_chunks", "batch", "tail_sample_ge1"} <= S.classes(2, 257, 1, 256, 32)
