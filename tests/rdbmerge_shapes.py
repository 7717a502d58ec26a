"""Stage batches aimed at the seams of rr_rdbmerge.hip's own code, and a vectorised expectation for them.

  forge(items, seed, lead, tail, data)   items (k, size) -> the three (data, offsets, status, data_cap) stage batches.
                                         k 1..3: held by stage k; H1, H2, H3: held at RR_E_CAPACITY by stage 1..3 (a hole:
                                         the size is kept, the stage's bytes there are random and never the canary, and
                                         nothing may be written); any other k: that first-stage status, size 0.
  fast_merge(stages, types, conv, ...)   rdbloadall_reference.merge without the per-value loop: (None, offsets, out_types,
                                         status, totals, image); image is the whole output room, CANARY where nothing
                                         is written, and stands where merge() has its list of blobs.
  deep_search ... last_bytes             the builders A..J: each returns a Shape (the items, how to forge them, the
                                         capacities to run, the facts its guard in tests/test_rdbmerge_shapes.py asserts).

S is the span of out->data a wave owns, ROW what it stores an instruction, PIECE what a lane does.  trace_find and
piece_table restate wave_find and the per-piece walk of merge_emit_kernel, for the guards alone: which search steps
and which (len, sh) segments a batch reaches is a fact about the batch, computed without the kernel.

one_call_packed: n = 3000 payloads; expected_batch (the three stage references and merge) took under 0.5 s for them on
the machine these tests were written on."""
import numpy as np

import redrock_old_amd as rr

import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbloadall_reference as la
import rdbzset_reference as zr
from test_rdbzset import ZSET, raw, zset

CANARY = 0xA5
S, ROW, PIECE = rr.RDBMERGE_SPAN, 1024, 16
MAX_WAVES = rr.RDBMERGE_MAX_WAVES
CAP, CONV, SLICE = la.E_CAPACITY, la.E_CONVERT, la.E_SLICE
SKIP2, SKIP3 = cv.SKIP, zr.SKIP
H1, H2, H3 = -1, -2, -3
BAD = (ld.E_TRUNC, ld.E_LEN)
SCAN_TILE, LB_GROUP = 4096, 64                                                  # rr_util.hip, rr_device.h
OPTS = ld.options(set_max_intset_entries=1000, zset_max_ziplist_entries=1000, zset_max_ziplist_value=300)

_HELD = np.array([(0, SKIP2, SKIP3), (CONV, 0, SKIP3), (CONV, CONV, 0)], np.uint8)
_HOLE = np.array([(CAP, SKIP2, SKIP3), (CONV, CAP, SKIP3), (CONV, CONV, CAP)], np.uint8)


def forge(items, seed=0, lead=(0, 0, 0), tail=(0, 0, 0), data=True):
    """lead[k] unused bytes in front of stage k's data, tail[k] behind it (0xEE; data_cap counts them).  data False:
    every data_cap is 0 and no byte exists, only the offsets (every item a hole)."""
    rng = np.random.default_rng(seed)
    it = np.asarray(items, np.int64).reshape(-1, 2)
    ks, sz = it[:, 0], it[:, 1]
    n = len(ks)
    st = np.zeros((3, n), np.uint8)
    st[1], st[2] = SKIP2, SKIP3
    st[0] = np.where((ks >= -3) & (ks <= 3), 0, ks).astype(np.uint8)
    sizes = np.zeros((3, n), np.int64)
    for k in (1, 2, 3):
        for sel, table in ((ks == k, _HELD), (ks == -k, _HOLE)):
            st[:, sel] = table[k - 1][:, None]
            sizes[k - 1, sel] = sz[sel]
    assert not sz[(ks < -3) | (ks > 3) | (ks == 0)].any()
    stages = []
    for k in range(3):
        offs = np.zeros(n + 1, np.uint64)
        np.cumsum(sizes[k], out=offs[1:])
        offs += np.uint64(lead[k])
        if not data:
            assert (ks < 0).all()
            stages.append((np.zeros(0, np.uint8), offs, st[k].copy(), 0))
            continue
        d = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
        for i in np.nonzero(ks == -(k + 1))[0]:                                  # a copied hole never looks like the canary
            h = d[int(offs[i]):int(offs[i + 1])]
            h[h == CANARY] = CANARY ^ 0xFF
        d = np.concatenate([d, np.full(tail[k], 0xEE, np.uint8)])
        stages.append((d, offs, st[k].copy(), len(d)))
    return stages


def type_bytes(n):
    return (np.arange(n) % 251).astype(np.uint8), ((np.arange(n) + 7) % 251).astype(np.uint8)


def room_of(total, data_cap):
    """(out_cap, bytes of output room) as test_gpu_rdbloadall.merge_device lays them out."""
    cap = total + 40 if data_cap is None else data_cap
    return cap, max(cap, total) + 64


def fast_merge(stages, types, conv_types, data_cap=None, room=None):
    n = len(stages[0][1]) - 1
    s1, s2, s3 = (np.asarray(s[2]) for s in stages)
    holds = lambda s: (s == 0) | (s == CAP)
    k = np.where(holds(s1), 1, np.where((s1 == CONV) & holds(s2), 2, np.where((s1 == CONV) & (s2 == CONV) & holds(s3), 3, 0)))
    st = np.select([k == 1, k == 2, k == 3, s1 != CONV], [s1, s2, s3, s1], CONV).astype(np.uint8)
    o0, o1, hcap = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(3):
        sel = k == j + 1
        o0[sel], o1[sel], hcap[sel] = stages[j][1][:-1][sel], stages[j][1][1:][sel], stages[j][3]
    bad_slice = (k > 0) & ((o0 > o1) | ((st == 0) & (o1 > hcap)))
    st[bad_slice] = SLICE
    held = (k > 0) & ~bad_slice
    sizes = np.where(held, o1 - o0, 0).astype(np.uint64)
    out_types = np.where(held, np.select([k == 1, k == 2], [types, conv_types], la.ZSET_ZIPLIST), la.NO_TYPE).astype(np.uint8)
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(sizes, out=offsets[1:])
    total = int(offsets[n])
    cap, default_room = room_of(total, data_cap)
    room = default_room if room is None else room
    st[(st == 0) & (offsets[1:] > np.uint64(cap))] = CAP
    wr = (st == 0) & (sizes > 0)
    image = np.full(room, CANARY, np.uint8)
    for j in range(3):
        sel = np.nonzero(wr & (k == j + 1))[0]
        ln = sizes[sel].astype(np.int64)
        if not len(sel):
            continue
        inside = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        image[np.repeat(offsets[sel].astype(np.int64), ln) + inside] = stages[j][0][np.repeat(o0[sel].astype(np.int64), ln) + inside]
    totals = {"n_elems": int(((st == 0) & (k >= 2)).sum()), "bytes": total, "n_bad": int((st != 0).sum()),
              "payload": int(sizes[st == 0].sum())}
    return None, offsets, out_types, st, totals, image


def image_of(want, room):
    """The output room of a merge() result, as fast_merge gives it."""
    img = np.full(room, CANARY, np.uint8)
    for i, b in enumerate(want[5]):
        if b:
            img[int(want[1][i]):int(want[1][i]) + len(b)] = np.frombuffer(b, np.uint8)
    return img


def same(fast, slow):
    """fast_merge's answer against merge()'s."""
    return (np.array_equal(fast[1], slow[1]) and np.array_equal(fast[2], slow[2]) and np.array_equal(fast[3], slow[3])
            and fast[4] == slow[4] and np.array_equal(fast[5], image_of(slow, len(fast[5]))))


def written_mask(want):
    """Per byte of [0, offsets[n]): written by a value."""
    offs, st = want[1].astype(np.int64), want[3]
    d = np.zeros(int(offs[-1]) + 1, np.int64)
    np.add.at(d, offs[:-1][st == 0], 1)
    np.add.at(d, offs[1:][st == 0], -1)
    return np.cumsum(d)[:-1] > 0


# ---- the kernel's searches, restated for the guards ---------------------------------------------------------------
def trace_find(offs, lo, hi, t, log):
    """wave_find: the first v in [lo, hi] with offs[v + 1] > t; log gets (step, no probe past t, first probe past t)."""
    lanes = np.arange(64)
    step = 1
    while lo < hi:
        p = lo + lanes * step
        past = (p >= hi) | (offs[np.minimum(p, hi) + 1] > t)
        if not past.any():
            log.append((step, True, -1, False))
            lo += 63 * step + 1
        else:
            f = int(np.argmax(past))
            top = lo + f * step
            log.append((step, False, f, top < hi))
            if top < hi:
                hi = top
            if f:
                lo += (f - 1) * step + 1
        step = (hi - lo) // 64 + 1
    return lo


def span_searches(offsets, end):
    """Every span's first search of merge_emit_kernel over a batch: the log of trace_find."""
    n, log = len(offsets) - 1, []
    offs = offsets.astype(np.int64)
    for s0 in range(0, end, S):
        v = trace_find(offs, 0, n - 1, s0, log)
        assert offs[v] <= s0 < offs[v + 1]
    return log


def piece_table(want):
    """(piece, value, len, sh) of every segment a lane assembles from a written value."""
    offs, st = want[1].astype(np.int64), want[3]
    rows = []
    for i in np.nonzero((st == 0) & (offs[1:] > offs[:-1]))[0]:
        b0, b1 = int(offs[i]), int(offs[i + 1])
        for p in range(b0 // PIECE, (b1 - 1) // PIECE + 1):
            a, e = max(b0, p * PIECE), min(b1, (p + 1) * PIECE)
            rows.append((p, i, e - a, a - p * PIECE))
    return np.array(rows, np.int64).reshape(-1, 4)


# ---- the builders ------------------------------------------------------------------------------------------------
class Shape:
    """items and how forge takes them; caps: the out_caps to run (None: room for everything); facts: for the guard."""

    def __init__(self, items, seed, caps=(None,), lead=(0, 0, 0), tail=(0, 0, 0), data=True, **facts):
        self.items, self.seed, self.caps, self.lead, self.tail, self.data = np.asarray(items, np.int64).reshape(-1, 2), seed, list(caps), lead, tail, data
        self.facts = facts
        self.n = len(self.items)

    def stages(self):
        return forge(self.items, self.seed, self.lead, self.tail, self.data)

    def fast(self, data_cap=None, room=None, stages=None):
        return fast_merge(stages or self.stages(), *type_bytes(self.n), data_cap, room)

    def slow(self, data_cap=None, stages=None):
        return la.merge(*(stages or self.stages()), *type_bytes(self.n), data_cap)


class _Items:
    """Items with the merged offset they have reached."""

    def __init__(self, seed):
        self.items, self.at, self.rng = [], 0, np.random.default_rng(seed)

    def add(self, k, size=0):
        self.items.append((k, size))
        self.at += size
        return len(self.items) - 1

    def empties(self, count):
        """A run of size-0 values: bad statuses and held empty blobs of the three stages mixed."""
        first = len(self.items)
        for j in range(count):
            self.add((BAD[0], 1, BAD[1], 2, 3)[j % 5])
        return first

    def fill(self, count, lo, hi):
        ks = self.rng.integers(1, 4, count)
        sz = self.rng.integers(lo, hi + 1, count)
        self.items += list(zip(ks.tolist(), sz.tolist()))
        self.at += int(sz.sum())

    def pad_to(self, mod, rem, k=1):
        """One value of stage k (never empty) after which the offset is rem mod `mod`."""
        self.add(k, (rem - self.at) % mod or mod)
        assert self.at % mod == rem


def deep_search(n=MAX_WAVES * 64 + 300, long_run=70000, row_run=5000, piece_run=4500, lead_run=300, trail_run=4200):
    """A.  Sizes 0..24 from the three stages, with runs of empty values: in front of byte 0, from a span start
    (the value behind it a 37-byte hole, so the next written value begins mid-row and mid-piece: a run of empty
    values has one offset, which cannot be a span start and mid-row at once), from a row start inside a span, from the
    middle of a piece (the one a lane's own search has to skip), and up to n - 1."""
    b = _Items(20)
    fixed = lead_run + long_run + row_run + piece_run + trail_run + 4
    part = (n - fixed) // 4
    b.empties(lead_run)
    second = (n - 65) // 64 + 1                                                  # wave_find's step behind the 64 empty values at 0
    hole = lead_run + part + 1 + long_run                                        # the index of the value under that span start:
    b.fill(part + (65 - hole) % second, 0, 24)                                   # on the search's new lo, so f == 0 at the third step
    b.pad_to(S, 0)
    long_at = (b.empties(long_run), b.at)
    b.add(H2, 37)
    b.fill(part, 0, 24)
    b.pad_to(S, 3 * ROW, 2)
    row_at = (b.empties(row_run), b.at)
    b.add(3, 7)
    b.fill(part, 0, 24)
    b.pad_to(PIECE, 5, 3)
    piece_at = (b.empties(piece_run), b.at)
    b.add(1, 30)
    b.fill(n - trail_run - len(b.items) - 1, 0, 24)
    b.add(1, 9)
    trail_at = (b.empties(trail_run), b.at)
    assert len(b.items) == n
    return Shape(b.items, 20, lead_run=lead_run, long_at=long_at, long_run=long_run, row_at=row_at, row_run=row_run,
                 piece_at=piece_at, piece_run=piece_run, trail_at=trail_at, trail_run=trail_run)


def mid_caps():
    """B.  About 600 values of 1..300 bytes; the out_caps inside a piece, a row and a span and around three values that
    cross a piece, a row and a span seam.  The first values (1, 3, 5, 4, 2, 7 bytes) put a written and a refused
    value into piece 0 for the caps 1 and 15."""
    b = _Items(21)
    for j, size in enumerate((1, 3, 5, 4, 2, 7)):
        b.add(1 + j % 3, size)
    b.fill(594, 1, 300)
    offs = np.zeros(len(b.items) + 1, np.int64)
    np.cumsum([s for _, s in b.items], out=offs[1:])
    first, last = offs[:-1], offs[1:] - 1
    crosses = lambda unit, inside: next(int(j) for j in range(100, len(b.items)) if first[j] // unit != last[j] // unit
                                        and (inside is None or first[j] // inside == last[j] // inside) and offs[j + 1] > 3 * S + 16)
    chosen = [crosses(PIECE, ROW), crosses(ROW, S), crosses(S, None)]
    caps = [1, 15, 16, 17, ROW - 1, ROW, ROW + 1, S - 1, S, S + 1] + [3 * S + k for k in range(16)]
    for j in chosen:
        caps += [int(offs[j + 1]) - 1, int(offs[j + 1]), int(offs[j + 1]) + 1]
    return Shape(b.items, 21, caps=caps, chosen=chosen)


def empty_at_cap():
    """C.  Held empty blobs of each stage and a bad empty value at offsets == out_cap (status 0, and the bad one its
    own), a refused value, and the same four behind it (RR_E_CAPACITY, and the bad one its own)."""
    b = _Items(22)
    b.fill(5, 3, 40)
    cap = b.at
    at_cap = [b.add(1), b.add(BAD[0]), b.add(2), b.add(3)]
    refused = b.add(2, 21)
    past = [b.add(3), b.add(BAD[1]), b.add(1), b.add(2)]
    b.add(1, 8)
    return Shape(b.items, 22, caps=[cap], at_cap=at_cap, refused=refused, past=past)


PATTERN = (1, 0, 2, 1, 0, 0, 3, 1, 16, 1, 15, 17)


def _is_prime(i):
    return i > 1 and all(i % d for d in range(2, int(i ** 0.5) + 1))


def packed():
    """D.  4096 values of PATTERN's sizes, the holding stage rotating with period 5, a bad empty value at every prime
    index; then sixteen one-byte values of stages 1, 2, 3, 1, ... filling one aligned piece, and the same sixteen
    begun 1..15 bytes into a piece, with an empty value (held or bad) behind each byte at the odd shifts."""
    b = _Items(23)
    for i in range(4096):
        if _is_prime(i):
            b.add(BAD[i % 2])
        else:
            b.add(1 + (i % 5) % 3, PATTERN[i % len(PATTERN)])
    blocks = []
    for shift in range(16):
        b.pad_to(PIECE, shift, 1 + shift % 3)
        blocks.append(b.at)
        for j in range(16):
            b.add(1 + j % 3, 1)
            if shift % 2:
                b.add((2, BAD[0], 3, BAD[1])[j % 4])
    b.add(2, 6)
    return Shape(b.items, 23, blocks=blocks)


def holes():
    """E.  Holes of each stage between written values: the first value, 5 bytes, a run of 40 of 1..30 bytes, 20 of 1..9
    bytes with written values of 1..6 bytes between them, 16 aligned bytes, ROW + 7, S + 100 from byte 5 of a piece 59 bytes before a span start (a whole span inside it), the last
    value."""
    b = _Items(24)
    marks = {}
    b.add(H1, 9)
    b.fill(6, 1, 40)
    marks["five"] = b.add(H2, 5)
    b.fill(6, 1, 40)
    marks["run"] = len(b.items)
    for j in range(40):
        b.add((H1, H2, H3)[j % 3], 1 + (7 * j) % 30)
    b.fill(6, 1, 40)
    marks["mixed"] = len(b.items)
    for j in range(20):                                                          # holes and written values of a few bytes, turn by turn
        b.add((H3, H1, H2)[j % 3], 1 + (5 * j) % 9)
        b.add(1 + j % 3, 1 + (3 * j) % 6)
    b.pad_to(PIECE, 0, 2)
    marks["aligned"] = b.add(H3, 16)
    b.fill(6, 1, 40)
    marks["row"] = b.add(H1, ROW + 7)
    b.fill(40, 1, 40)
    b.pad_to(S, S - 59, 3)
    assert b.at % PIECE == 5
    marks["span"] = b.add(H2, S + 100)
    b.fill(30, 1, 40)
    marks["last"] = b.add(H3, 11)
    return Shape(b.items, 24, **marks)


SMALL_PARTS = {1: (1, 0), 5: (2, 3), 15: (7, 8), 16: (5, 5, 6), 17: (16, 1), 31: (10, 5, 16)}


def small_stage(total, small=3, tail=0):
    """F.  The small stage's whole batch is `total` bytes in two or three values among 200 values of the other two;
    its data_cap is total + tail."""
    b = _Items(25 + total)
    others = [k for k in (1, 2, 3) if k != small]
    parts = dict(zip((40, 110, 170), SMALL_PARTS[total]))
    for i in range(200 + len(parts)):
        if i in parts:
            b.add(small, parts.pop(i))
        else:
            b.add(others[i % 2], int(b.rng.integers(6, 200)))
    assert not parts
    t = [0, 0, 0]
    t[small - 1] = tail
    return Shape(b.items, 25 + total, tail=tuple(t), small=small, total=total)


def last_bytes(tail):
    """J.  Every stage's data_cap exceeds its last offset by `tail` bytes (0xEE there).  300 values of 1..40 bytes,
    the third stage's whole batch 5 bytes, so its data_cap passes 16 with the tail; the last value of each stage ends
    on that stage's last used byte."""
    b = _Items(26)
    for i in range(300):
        b.add(3, (2, 3)[i // 200]) if i in (100, 200) else b.add(1 + i % 2, int(b.rng.integers(1, 41)))
    b.add(2, 3), b.add(1, 1), b.add(2, 14)
    return Shape(b.items, 26, tail=(tail,) * 3)


def sizing_past_4gib(n=2 * SCAN_TILE * LB_GROUP + 5000, small_at=SCAN_TILE * LB_GROUP - SCAN_TILE, small_len=3 * SCAN_TILE):
    """G.  Holes only, sizes up to 2^27 and a stretch of sizes under 1000 across the first look-back group's end:
    no data, every data_cap and out_cap 0."""
    rng = np.random.default_rng(27)
    sz = rng.integers(0, (1 << 27) + 1, n)
    sz[small_at:small_at + small_len] = rng.integers(0, 1000, small_len)
    ks = -(1 + np.arange(n) % 3)
    return Shape(np.stack([ks, sz], 1), 27, caps=[0], data=False, small_at=small_at, small_len=small_len)


def scan_facts(sizes):
    """What rr_launch_scan_u64's kernel sees: the sums of a thread's 16 values per wave (1024 values), per tile, per group."""
    pad = np.zeros(-len(sizes) % (SCAN_TILE * LB_GROUP) + len(sizes), np.int64)
    pad[:len(sizes)] = sizes
    thread = pad.reshape(-1, 16).sum(1)
    return thread.reshape(-1, 64), pad.reshape(-1, SCAN_TILE).sum(1), pad.reshape(-1, SCAN_TILE * LB_GROUP).sum(1)


def one_call_packed(n=3000):
    """H.  Payloads for the one call: integer Strings (stage 1), integer Sets of one and two members (stage 2), ZSets of
    one fractional member (stage 3), with empty, truncated and bad-type payloads between them.  (types, data, offsets)."""
    rng = np.random.default_rng(28)
    types, pays = [], []
    for i in range(n):
        k = i % 8
        if k in (0, 3):
            types.append(rr.T_STRING), pays.append(b"\xC0" + bytes([int(rng.integers(0, 128))]))
        elif k in (1, 6):
            m = [raw(b"%d" % int(x)) for x in rng.integers(-30000, 30000, 1 + (i // 8) % 2)]
            types.append(rr.T_SET_HT), pays.append(bytes([len(m)]) + b"".join(m))
        elif k in (2, 5):
            types.append(ZSET), pays.append(zset([(b"m", int(rng.integers(1, 999)) / 8 + 0.0625)]))
        elif k == 4:
            types.append(rr.T_STRING), pays.append((b"", b"\xC0", raw(b"abc")[:-1], raw(b""))[(i // 8) % 4])
        else:
            types.append((3, rr.T_SET_HT, ZSET)[(i // 8) % 3]), pays.append((b"\x00", b"\x00", b"\x01" + raw(b"m"))[(i // 8) % 3])
    return (np.asarray(types, np.uint8),) + ld.pack(pays)
