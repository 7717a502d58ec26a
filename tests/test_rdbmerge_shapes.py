"""The batches of tests/rdbmerge_shapes.py held to account on the CPU: every builder reaches the edge of
rr_rdbmerge.hip it is named for, by the reference alone, and fast_merge gives what rdbloadall_reference.merge
gives on every one of them (at full size too: merge()'s loop needs a few seconds for the half million values of A
and G).  These are conditions on the inputs; tests/test_gpu_rdbmerge_edges.py runs the kernels on them."""
import numpy as np
import pytest

import rdbload_reference as ld
import rdbloadall_reference as la
import rdbmerge_shapes as sh
from rdbmerge_shapes import CAP, PIECE, ROW, S


def both(shape, cap=None):
    stages = shape.stages()
    fast, slow = shape.fast(cap, stages=stages), shape.slow(cap, stages=stages)
    assert sh.same(fast, slow)
    return fast


def test_forge_items():
    """A hole keeps its size at RR_E_CAPACITY, advances its stage's offsets, and its bytes are never the canary."""
    items = [(1, 4), (sh.H2, 300), (ld.E_TRUNC, 0), (sh.H3, 7), (3, 2), (sh.H1, 5), (2, 6)]
    st = sh.forge(items, seed=1, lead=(2, 0, 1), tail=(0, 3, 0))
    assert [s[2].tolist() for s in st] == [[0, sh.CONV, ld.E_TRUNC, sh.CONV, sh.CONV, CAP, sh.CONV],
                                           [sh.SKIP2, CAP, sh.SKIP2, sh.CONV, sh.CONV, sh.SKIP2, 0],
                                           [sh.SKIP3, sh.SKIP3, sh.SKIP3, CAP, 0, sh.SKIP3, sh.SKIP3]]
    assert st[0][1].tolist() == [2, 6, 6, 6, 6, 6, 11, 11] and st[1][1].tolist() == [0, 0, 300, 300, 300, 300, 300, 306]
    assert [s[3] for s in st] == [11, 309, 10] and st[1][0][306:].tolist() == [0xEE] * 3
    assert not (st[1][0][:300] == sh.CANARY).any() and len(set(st[1][0][:300].tolist())) > 100
    want = both(sh.Shape(items, 1, lead=(2, 0, 1), tail=(0, 3, 0)))
    assert want[3].tolist() == [0, CAP, ld.E_TRUNC, CAP, 0, CAP, 0] and want[1].tolist() == [0, 4, 304, 304, 311, 313, 318, 324]
    assert (want[5][4:311] == sh.CANARY).all() and want[4] == {"n_elems": 2, "bytes": 324, "n_bad": 4, "payload": 12}
    empty = sh.forge([(sh.H1, 1 << 40), (sh.H3, 5)], data=False)
    assert [s[3] for s in empty] == [0, 0, 0] and int(empty[0][1][-1]) == 1 << 40
    assert sh.fast_merge(empty, *sh.type_bytes(2), 0, 64)[3].tolist() == [CAP, CAP]


# ---- A ----------------------------------------------------------------------------------------------------
def deep_guard(shape, full):
    f, n = shape.facts, shape.n
    want = shape.fast()
    offs, st = want[1].astype(np.int64), want[3]
    total = int(offs[-1])
    empty = offs[1:] == offs[:-1]
    for name, unit, rem in (("long", S, 0), ("row", S, 3 * ROW), ("piece", PIECE, 5)):
        (first, at), count = f[name + "_at"], f[name + "_run"]
        assert empty[first:first + count].all() and not empty[first - 1] and not empty[first + count]
        assert at % unit == rem and (offs[first:first + count + 1] == at).all()
        assert {0, ld.E_TRUNC, ld.E_LEN} <= set(st[first:first + count].tolist())   # bad statuses and held empty blobs mixed
    first, at = f["long_at"]
    nxt = first + f["long_run"]
    assert st[nxt] == CAP and st[nxt + 1] == 0                                     # the hole, then the next written value
    written = int(np.nonzero((st[nxt:] == 0) & ~empty[nxt:])[0][0]) + nxt
    assert offs[written] % ROW != 0 and offs[written] % PIECE != 0 and offs[written] // ROW == at // ROW
    assert empty[:f["lead_run"]].all() and not empty[f["lead_run"]] and offs[f["lead_run"]] == 0
    assert empty[n - f["trail_run"]:].all() and not empty[n - f["trail_run"] - 1] and f["trail_at"][1] == total
    log = sh.span_searches(want[1], total)
    steps = [e[0] for e in log]
    assert any(e[2] == 0 for e in log if e[0] > 1) and any(e[3] for e in log if e[0] > 1)
    second = (n - 65) // 64 + 1                                                     # the step behind the 64 empty values at 0
    assert f["lead_run"] >= 64 and (nxt - 65) % second == 0                         # so the search for that span start has f == 0
    if full:
        deep = [e for e in log if e[0] >= 65]                                      # b == 0, f == 0 and top < hi past the second level
        assert any(e[1] for e in deep) and any(e[2] == 0 for e in deep) and any(e[3] for e in deep)
        assert n == sh.MAX_WAVES * 64 + 300 and f["long_run"] == 70000 and f["row_run"] == 5000 and f["piece_run"] > 4096
        assert f["lead_run"] == 300 and f["trail_run"] == 4200
        assert max(steps) >= 4097 and any(65 <= s < 4097 for s in steps)
        assert n > sh.MAX_WAVES * 64 and (st[sh.MAX_WAVES * 64:] != 0).any()     # the prologue's second stride counts bad values
        assert -(-n // sh.SCAN_TILE) > 2 * sh.LB_GROUP                              # three look-back groups
        assert 5_000_000 < total < 7_000_000 and total // S > 500
    return want


def test_deep_search_reduced():
    shape = sh.deep_search(n=9000, long_run=700, row_run=200, piece_run=150, lead_run=70, trail_run=420)
    deep_guard(shape, False)
    both(shape)


def test_deep_search_full():
    shape = sh.deep_search()
    deep_guard(shape, True)
    both(shape)


# ---- B ----------------------------------------------------------------------------------------------------
def test_mid_caps():
    shape = sh.mid_caps()
    full = both(shape)
    offs = full[1].astype(np.int64)
    total = int(offs[-1])
    assert 590 <= shape.n <= 610 and total > 4 * S and len(set(shape.caps)) == len(shape.caps) == 35
    j1, j2, j3 = shape.facts["chosen"]
    assert offs[j1] // PIECE != (offs[j1 + 1] - 1) // PIECE and offs[j1] // ROW == (offs[j1 + 1] - 1) // ROW
    assert offs[j2] // ROW != (offs[j2 + 1] - 1) // ROW and offs[j2] // S == (offs[j2 + 1] - 1) // S
    assert offs[j3] // S != (offs[j3 + 1] - 1) // S
    shared = set()
    for cap in shape.caps:
        want = both(shape, cap)
        refused = int(np.nonzero(offs[1:] > cap)[0][0])                             # the first value that ends past the cap
        assert 0 < refused < shape.n and (want[3][:refused] == 0).all() and (want[3][refused:] == CAP).all()
        assert np.array_equal(want[1], full[1]) and want[4]["payload"] == offs[refused] <= cap < total
        assert np.array_equal(want[5][:offs[refused]], full[5][:offs[refused]]) and (want[5][offs[refused]:] == sh.CANARY).all()
        if (offs[refused] - 1) // PIECE == offs[refused] // PIECE and offs[refused] % PIECE:
            shared.add(cap)                                                         # a written and a refused value in one piece
    assert {1, 15} <= shared and len(shared) > 10
    for j in (j1, j2, j3):                                                          # the cap on, before and behind a value's end
        at = shape.caps.index(int(offs[j + 1]))
        assert [int(np.nonzero(offs[1:] > c)[0][0]) for c in shape.caps[at - 1:at + 2]] == [j, j + 1, j + 1]


# ---- C ----------------------------------------------------------------------------------------------------
def test_empty_at_cap():
    shape = sh.empty_at_cap()
    cap, f = shape.caps[0], shape.facts
    want = both(shape, cap)
    offs, st = want[1], want[3]
    assert all(int(offs[i]) == int(offs[i + 1]) == cap for i in f["at_cap"]) and st[f["at_cap"]].tolist() == [0, ld.E_TRUNC, 0, 0]
    assert st[f["refused"]] == CAP and int(offs[f["refused"]]) == cap
    assert all(int(offs[i]) == int(offs[i + 1]) > cap for i in f["past"]) and st[f["past"]].tolist() == [CAP, ld.E_LEN, CAP, CAP]
    held = [int(shape.items[i, 0]) for i in f["at_cap"] + f["past"]]
    assert sorted(held[:4]) == sorted([1, 2, 3, ld.E_TRUNC]) and sorted(held[4:]) == sorted([1, 2, 3, ld.E_LEN])


# ---- D ----------------------------------------------------------------------------------------------------
def test_packed():
    shape = sh.packed()
    want = both(shape)
    offs, st = want[1].astype(np.int64), want[3]
    sizes = shape.items[:4096, 1]
    assert set(sh.PATTERN) <= set(sizes.tolist()) and all((shape.items[i, 0] in sh.BAD) == sh._is_prime(i) for i in range(4096))
    combos = {(int(k), int(s)) for k, s in shape.items[:4096] if k in (1, 2, 3)}
    assert len(combos) == 3 * len(set(sh.PATTERN))                                  # every size from every stage
    t = sh.piece_table(want)
    count = np.bincount(t[:, 0])
    assert count.max() == 16
    for shift, at in enumerate(shape.facts["blocks"]):
        assert at % PIECE == shift
        seg = t[(t[:, 0] * PIECE + t[:, 3] >= at) & (t[:, 0] * PIECE + t[:, 3] < at + 16)]
        assert len(seg) == 16 and (seg[:, 2] == 1).all() and (np.diff(seg[:, 1]) == (2 if shift % 2 else 1)).all()
        assert [int(shape.items[v, 0]) for v in seg[:, 1]] == [1 + j % 3 for j in range(16)]
        if shift % 2:                                                               # held and bad empty values between the bytes
            assert {int(st[v + 1]) for v in seg[:, 1]} == {0, ld.E_TRUNC, ld.E_LEN}
    assert count[shape.facts["blocks"][0] // PIECE] == 16
    size = offs[1:] - offs[:-1]
    whole = set((offs[:-1][(size == 16) & (offs[:-1] % 16 == 0) & (st == 0)] // ROW).tolist())   # len 16, sh 0
    tip = set((offs[:-1][(size == 1) & (offs[:-1] % 16 == 15) & (st == 0)] // ROW).tolist())     # len 1, sh 15
    assert whole and tip and whole & tip                                            # and both in one row
    assert {(16, 0), (1, 15)} <= {(int(r[2]), int(r[3])) for r in t}


# ---- E ----------------------------------------------------------------------------------------------------
def test_holes():
    shape = sh.holes()
    want = both(shape)
    f = shape.facts
    offs, st = want[1].astype(np.int64), want[3]
    size = offs[1:] - offs[:-1]
    hole = shape.items[:, 0] < 0
    assert (st[hole] == CAP).all() and (st[~hole] == 0).all() and np.array_equal(size, shape.items[:, 1])
    assert hole[0] and hole[-1] and not hole[1] and not hole[-2]
    assert size[f["five"]] == 5 and not hole[f["five"] - 1] and not hole[f["five"] + 1]
    run = slice(f["run"], f["run"] + 40)
    assert hole[run].all() and not hole[f["run"] - 1] and not hole[f["run"] + 40] and 1 <= size[run].min() and size[run].max() <= 30
    assert {int(k) for k in shape.items[run, 0]} == {sh.H1, sh.H2, sh.H3} == {int(k) for k in shape.items[hole, 0]}
    assert size[f["aligned"]] == 16 and offs[f["aligned"]] % PIECE == 0
    assert size[f["row"]] == ROW + 7 and size[f["span"]] == S + 100 and offs[f["span"]] % PIECE == 5
    assert 0 < -offs[f["span"]] % S <= 100                                          # so a whole span lies inside it
    w = sh.written_mask(want)
    total = len(w) // PIECE * PIECE
    per = lambda unit: w[:len(w) // unit * unit].reshape(-1, unit).sum(1)
    pieces = per(PIECE)
    mixed = slice(f["mixed"], f["mixed"] + 40)
    assert hole[mixed][0::2].all() and not hole[mixed][1::2].any() and size[mixed].max() <= 9
    assert ((pieces > 0) & (pieces < PIECE)).sum() > 15 and (pieces == 0).sum() > (S + ROW) // PIECE
    assert (per(ROW) == 0).any() and (per(S) == 0).any() and total > 2 * S
    assert pieces[offs[f["aligned"]] // PIECE] == 0 and pieces[offs[f["aligned"]] // PIECE - 1] > 0


# ---- F, J -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [3, 1])
@pytest.mark.parametrize("total", sorted(sh.SMALL_PARTS))
def test_small_stage(total, small):
    shape = sh.small_stage(total, small)
    stages = shape.stages()
    assert [s[3] for s in stages][small - 1] == total == int(stages[small - 1][1][-1]) and shape.lead == (0, 0, 0)
    assert min(s[3] for k, s in enumerate(stages) if k != small - 1) > 5000
    parts = shape.items[shape.items[:, 0] == small, 1].tolist()
    assert len(parts) in (2, 3) and sum(parts) == total
    want = both(shape)
    assert (want[3] == 0).all()


@pytest.mark.parametrize("tail", [0, 1, 15, 16, 17])
def test_last_bytes(tail):
    shape = sh.last_bytes(tail)
    stages = shape.stages()
    for k, (data, offs, _, cap) in enumerate(stages):
        assert cap == len(data) == int(offs[-1]) + tail and (data[int(offs[-1]):] == 0xEE).all()
        last = int(np.nonzero(shape.items[:, 0] == k + 1)[0][-1])
        assert int(offs[last + 1]) == int(offs[-1]) and 0 < int(offs[last + 1] - offs[last]) < 16   # a segment in the last 15 bytes
    assert int(stages[2][1][-1]) == 5 and (stages[2][3] < 16) == (tail in (0, 1))
    for t in (0, tail):                                                             # and the small stage on its own tail
        s = sh.small_stage(5, 3, t)
        assert s.stages()[2][3] == 5 + t
    both(shape)


# ---- G ----------------------------------------------------------------------------------------------------
def sizing_guard(shape):
    sizes = shape.items[:, 1]
    waves, tiles, groups = sh.scan_facts(sizes)
    slow = (waves >= 1 << 26).any(1)
    real = slow[:-(-shape.n // 1024)]                                               # the waves that hold values
    assert real.mean() > 0.9 and (~real).sum() >= 8                                 # both forms of the wave sums in one launch
    ntiles = -(-shape.n // sh.SCAN_TILE)
    slow_tile = slow.reshape(-1, 4).all(1)[:ntiles]
    fast_tile = (~slow).reshape(-1, 4).all(1)[:ntiles]
    assert fast_tile[sh.LB_GROUP - 1] and fast_tile[sh.LB_GROUP] and slow_tile[sh.LB_GROUP - 2] and slow_tile[sh.LB_GROUP + 2]
    assert len(groups) >= 3 and groups.max() < 1 << 48 and int(sizes.sum()) < 1 << 62   # GRP_VAL, LB_VAL
    assert int(np.cumsum(sizes)[sh.SCAN_TILE * sh.LB_GROUP - 1]) > 1 << 32           # past 2^32 within the first group
    assert (shape.items[:, 0] < 0).all() and sizes.max() > (1 << 27) - (1 << 20)


def test_sizing_past_4gib():
    shape = sh.sizing_past_4gib()
    assert shape.n == 2 * 262144 + 5000
    sizing_guard(shape)
    stages = shape.stages()
    fast, slow = shape.fast(0, 64, stages), shape.slow(0, stages)
    assert sh.same(fast, slow) and (fast[3] == CAP).all() and (fast[5] == sh.CANARY).all()
    assert fast[4] == {"n_elems": 0, "bytes": int(shape.items[:, 1].sum()), "n_bad": shape.n, "payload": 0}
    assert sum(int(s[1][-1]) for s in stages) == fast[4]["bytes"] > 1 << 44


def test_sizing_second_stride():
    """The same shape with more values than merge_size_kernel's 16384 x 256 threads: still inside the look-back fields."""
    shape = sh.sizing_past_4gib(16384 * 256 + 300)
    sizing_guard(shape)
    assert shape.n > 16384 * 256 and int(shape.items[:, 1].sum()) > 1 << 47


def test_sizing_reduced():
    shape = sh.sizing_past_4gib(n=9000, small_at=3000, small_len=2100)
    fast, slow = shape.fast(0, 64), shape.slow(0)
    assert sh.same(fast, slow)


# ---- H ----------------------------------------------------------------------------------------------------
def test_one_call_packed():
    types, data, offs = sh.one_call_packed()
    full = la.expected_batch(types, data, offs, sh.OPTS)
    caps = (full[6][0], full[6][1] // 2, full[6][2])
    short = la.expected_batch(types, data, offs, sh.OPTS, stage_cap=caps)
    assert len(types) == 3000 and np.array_equal(short[1], full[1]) and short[6] == full[6]
    s1 = ld.load_batch(types, data, offs, sh.OPTS)[2]
    s2 = sh.cv.convert_batch(types, data, offs, s1, sh.OPTS)[3]
    s3 = sh.zr.zset_batch(types, data, offs, s2, sh.OPTS)[2]
    held = [(s1 == 0).sum(), (s2 == 0).sum(), (s3 == 0).sum()]
    assert held[0] >= 700 and held[1] >= 700 and held[2] >= 700 and full[4]["n_bad"] > 300
    size = (full[1][1:] - full[1][:-1]).astype(np.int64)
    assert 0 < size[s1 == 0].max() < PIECE and (size[full[3] == 0] > 0).all()        # blobs of under one piece
    holes = np.nonzero((short[3] == CAP) & (full[3] == 0))[0]
    assert 300 < len(holes) < held[1] and (s2[holes] == 0).all() and np.array_equal(np.delete(short[3], holes), np.delete(full[3], holes))
    first = int(holes[0])
    assert (short[3][first:][s2[first:] == 0] == CAP).all() and (short[3][:first][s2[:first] == 0] == 0).all()   # a run to the end
    w = sh.written_mask(short)
    pieces = w[:len(w) // PIECE * PIECE].reshape(-1, PIECE).sum(1)
    assert ((pieces > 0) & (pieces < PIECE)).sum() > 100                             # kept and written bytes share pieces
    assert np.bincount(sh.piece_table(full)[:, 0]).max() >= 3                        # and several values a piece
