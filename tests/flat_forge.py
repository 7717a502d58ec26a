"""Forged flat batches for the encoders: records, descriptors and an arena built from scratch, no
decoder involved (include/rr_serdes.h: rr_encode_batch takes whatever flat batch its caller
builds).  Four kinds of builders, all returning (values, elems, arena) as VALUE_DT / ELEM_DT /
uint8 arrays:

  well_formed / decimal_lists   encodable values of every type, the empty ones included;
  forge_mutations               structured mutants of a well-formed batch, one field of one value
                                at a time (also returns the mutation class of every value);
  placement helpers             rejected values put where the kernels' walks change path: a run
                                across a 256-value block edge, a run in front of a value at a
                                16 KiB output-window edge, the first / last / every value, a
                                block of more than 4,096 descriptors;
  tiling helpers                a 61-value base batch whose value records are repeated over the
                                same descriptors and arena, and the expected rdbsave output of
                                the repeat from the reference's answer for the base alone.

Nothing here decides what is encodable: tests/encode_expect.py states that rule.
"""
import struct

import numpy as np

import redrock_old_amd as rr
from oracle import pyoracle

E1_BLOCK = 256        # values per enc_size_kernel workgroup
ENC_WINDOW = 16384    # output bytes per enc_emit_kernel workgroup
ENC_MAPCAP = 4096     # descriptors of one E1 block above which it searches instead of mapping
ZL_TYPES = (rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST)


class Flat:
    """A flat batch under construction: values own consecutive descriptor ranges, payloads go to
    the arena with 0-3 bytes of slack before each (no alignment to rely on)."""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.values, self.elems, self.arena = [], [], bytearray()

    def put(self, payload):
        self.arena += bytes(int(self.rng.integers(0, 4)))
        at = len(self.arena)
        self.arena += payload
        return at

    def add(self, typ, enc, items, lru=None, status=0):
        """items: bytes -> STR, int -> INT, ("score", bits) -> SCORE, ("zl", bytes) -> ZLRAW,
        ("raw", kind, data, len, zenc, rsv) -> the descriptor as given."""
        base = len(self.elems)
        for it in items:
            if isinstance(it, (bytes, bytearray)):
                self.elems.append((self.put(it), len(it), rr.K_STR, 0, 0))
            elif isinstance(it, int):
                self.elems.append((it & 0xFFFFFFFFFFFFFFFF, 0, rr.K_INT, 0, 0))
            elif it[0] == "score":
                self.elems.append((it[1], 0, rr.K_SCORE, 0, 0))
            elif it[0] == "zl":
                self.elems.append((self.put(it[1]), len(it[1]), rr.K_ZLRAW, 0, 0))
            else:
                _, kind, data, ln, zenc, rsv = it
                self.elems.append((data, ln, kind, zenc, rsv))
        if lru is None:
            lru = int(self.rng.integers(0, 1 << 24))
        self.values.append((typ, enc, status, lru, len(items), base))
        return len(self.values) - 1

    def done(self):
        v = np.array(self.values, dtype=rr.VALUE_DT) if self.values else np.zeros(0, rr.VALUE_DT)
        e = np.array(self.elems, dtype=rr.ELEM_DT) if self.elems else np.zeros(0, rr.ELEM_DT)
        # (never an empty descriptor array or arena: the bindings pass those as NULL)
        if len(e) == 0:
            e = np.zeros(1, rr.ELEM_DT)
        a = np.frombuffer(bytes(self.arena) or b"\0", np.uint8).copy()
        return v, e, a


def _word(rng, lo, hi):
    """A payload that is never a decimal integer (a List STR element that string2ll accepts would
    decode as INT, and the well-formed batch round-trips through the decoder)."""
    return b"k" + bytes(rng.integers(0, 256, int(rng.integers(lo, hi)), dtype=np.uint8))


def _score_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _add_well_formed(f, k, scale):
    """One encodable value of shape k (0..19): every type, and every empty form."""
    rng = f.rng
    big = max(1, scale)
    if k == 0:
        f.add(rr.T_STRING, 0, [_word(rng, 0, 40 * big)])
    elif k == 1:
        f.add(rr.T_STRING, 8, [_word(rng, 0, 43)])
    elif k == 2:
        f.add(rr.T_STRING, 1, [int(rng.integers(-2**63, 2**63 - 1))])
    elif k == 3:
        f.add(rr.T_STRING, 0, [b""])                                   # RAW of length 0
    elif k == 4:
        f.add(rr.T_STRING, 8, [b""])                                   # EMBSTR of length 0
    elif k == 5:
        items = []
        for _ in range(int(rng.integers(1, 6 * big + 2))):
            items.append(_word(rng, 0, 12) if rng.integers(0, 2) else
                         int(rng.integers(-2**63, 2**63 - 1)) >> int(rng.integers(0, 64)))
        f.add(rr.T_LIST_QUICKLIST, 0, items)
    elif k == 6:
        f.add(rr.T_LIST_QUICKLIST, 0, [])                              # 5-byte blob
    elif k == 7:
        w = (2, 4, 8)[int(rng.integers(0, 3))]
        lim = 1 << (8 * w - 1)
        f.add(rr.T_SET_INTSET, w, sorted({int(x) for x in rng.integers(-lim, lim - 1, int(rng.integers(1, 5 * big + 2)))}))
    elif k == 8:
        f.add(rr.T_SET_INTSET, (2, 4, 8)[int(rng.integers(0, 3))], [])
    elif k == 9:
        f.add(rr.T_SET_HT, 0, [b"%d" % j + _word(rng, 0, 10) for j in range(int(rng.integers(1, 4 * big + 2)))])
    elif k == 10:
        f.add(rr.T_SET_HT, 0, [])
    elif k == 11:
        items = []
        for j in range(int(rng.integers(1, 3 * big + 2))):
            items += [b"f%d" % j + _word(rng, 0, 6), _word(rng, 0, 12)]
        f.add(rr.T_HASH_HT, 0, items)
    elif k == 12:
        f.add(rr.T_HASH_HT, 0, [])
    elif k == 13:
        pairs = [(float(int(x)) / 4, b"m%d" % j + _word(rng, 0, 8))
                 for j, x in enumerate(rng.integers(-50, 50, int(rng.integers(1, 3 * big + 2))))]
        pairs.sort(reverse=True)                                       # serZset's order
        items = []
        for sc, m in pairs:
            items += [m, ("score", _score_bits(sc))]
        f.add(rr.T_ZSET_SKIPLIST, 0, items)
    elif k == 14:
        f.add(rr.T_ZSET_SKIPLIST, 0, [])
    elif k in (15, 16):
        # a ziplist value as the decoder leaves it: ZLRAW then one descriptor per entry
        typ = ZL_TYPES[k - 15]
        ents = []
        for j in range(int(rng.integers(1, 2 * big + 2))):
            ents += [b"e%d" % j + _word(rng, 0, 6), int(rng.integers(-70000, 70000))]
        zl = pyoracle.build_ziplist(ents)
        items = [("zl", zl)]
        for kind, data, ln, zenc in pyoracle.parse_ziplist(zl, 0):
            items.append(("raw", kind, data & 0xFFFFFFFFFFFFFFFF, ln, zenc, 0))
        i = f.add(typ, 0, items)
        # (entry descriptors point into the ZLRAW payload, wherever that went)
        zat = f.elems[f.values[i][5]][0]
        for j in range(1, len(items)):
            d, ln, kind, zenc, rsv = f.elems[f.values[i][5] + j]
            if kind == rr.K_STR:
                f.elems[f.values[i][5] + j] = (d + zat, ln, kind, zenc, rsv)
    elif k == 17:
        # ZLRAW alone (what RR_CTX_ZL_RAW decodes to), any bytes
        f.add(ZL_TYPES[int(rng.integers(0, 2))], 0, [("zl", bytes(rng.integers(0, 256, int(rng.integers(1, 30 * big)), dtype=np.uint8)))])
    elif k == 18:
        f.add(ZL_TYPES[int(rng.integers(0, 2))], 0, [("zl", b"")])     # ZLRAW of length 0
    else:
        # ZLRAW then descriptors of any kind: only descriptor 0 is written
        items = [("zl", bytes(rng.integers(0, 256, 12, dtype=np.uint8)))]
        for _ in range(int(rng.integers(1, 5))):
            items.append(("raw", int(rng.integers(0, 4)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 99)), 7, 0))
        f.add(ZL_TYPES[int(rng.integers(0, 2))], 0, items)


N_SHAPES = 20


def well_formed(seed, n, scale=1):
    """n encodable values cycling through every shape (types, encodings, the empty forms)."""
    f = Flat(seed)
    order = f.rng.permutation(N_SHAPES)
    for i in range(n):
        _add_well_formed(f, int(order[i % N_SHAPES]), scale)
    return f.done()


def decimal_integers():
    """The integers whose decimal length sits at a digit-count or bit-count edge."""
    xs = []
    for k in range(1, 19):
        for m in (10**k - 1, 10**k, 10**k + 1):
            xs += [m, -m]
    for k in range(1, 63):
        for m in (2**k - 1, 2**k):
            xs += [m, -m]
    xs += [2**63 - 1, -2**63]
    return xs


def decimal_lists(dense, seed=7):
    """The decimal integers in Lists.  dense: all-integer Lists (every task of an emit wave an
    integer: more than 21 a wave); else every integer followed by three short strings (16 a wave).
    Returns ((values, elems, arena), per-value item lists) — items are ints and bytes."""
    f = Flat(seed)
    xs = decimal_integers()
    lists = []
    per = 50 if dense else 16
    for i in range(0, len(xs), per):
        items = []
        for x in xs[i:i + per]:
            items.append(x)
            if not dense:
                items += [_word(f.rng, 0, 5) for _ in range(3)]
        f.add(rr.T_LIST_QUICKLIST, 0, items)
        lists.append(items)
    return f.done(), lists


# ---- mutations ------------------------------------------------------------------------------
COLLECTIONS = (rr.T_LIST_QUICKLIST, rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST, rr.T_SET_INTSET)
STR_KINDS = (rr.K_STR, rr.K_ZLRAW)
# mutation class -> (the rule can reject such a mutant, the rule can accept one)
MUTATION_CLASSES = {
    "type": (True, False), "enc": (True, True), "status": (True, False), "lru": (False, True),
    "n_elems": (True, True), "elem_base": (True, True), "kind": (True, True), "arena": (True, True),
    "intset": (True, True), "odd": (True, False), "swap": (True, False), "zenc_rsv": (False, True),
    "string_n": (True, False),
}


def forge_mutations(values, elems, arena, seed, share=0.6):
    """Mutants of a well-formed batch, one field of one value at a time; about `share` of the
    values are mutated.  Returns (values, elems, arena, classes): classes[i] is the mutation class
    of value i (MUTATION_CLASSES) or None.  The descriptor array and the arena grow by one tail
    each, so that one value's range ends exactly at elem_cap and one payload exactly at
    arena_cap."""
    rng = np.random.default_rng(seed)
    v, e, a = values.copy(), elems.copy(), arena.copy()
    n = len(v)
    classes = [None] * n

    def has_str(i):
        b, c = int(v["elem_base"][i]), int(v["n_elems"][i])
        if c == 0 or v["type"][i] == rr.T_SET_INTSET:
            return False
        return bool(v["type"][i] in ZL_TYPES or (e["kind"][b:b + c] == rr.K_STR).any())

    # a class that applies to the value; half the time one only its type can take (they are rare)
    picked = {}
    for i in rng.permutation(n)[:int(n * share)]:
        i = int(i)
        t, c = int(v["type"][i]), int(v["n_elems"][i])
        common = ["type", "enc", "status", "lru", "n_elems", "elem_base"]
        if c:
            common += ["kind", "zenc_rsv"]
        if has_str(i):
            common.append("arena")
        own = []
        if t == rr.T_SET_INTSET and c:
            own.append("intset")
        if t in (rr.T_HASH_HT, rr.T_ZSET_SKIPLIST) and c >= 2:
            own.append("odd")
        if t == rr.T_ZSET_SKIPLIST and c >= 2:
            own.append("swap")
        if t == rr.T_STRING:
            own.append("string_n")
        pool = own if own and rng.integers(0, 2) else common
        picked[i] = pool[int(rng.integers(0, len(pool)))]

    # the two tails first: they fix elem_cap and arena_cap for every other mutant
    tail_e = next((i for i in picked if picked[i] == "elem_base" and v["n_elems"][i] >= 2), None)
    tail_a = next((i for i in picked if picked[i] == "arena" and has_str(i) and i != tail_e), None)
    if tail_a is not None:
        b, c = int(v["elem_base"][tail_a]), int(v["n_elems"][tail_a])
        k = next(b + j for j in range(c) if e["kind"][b + j] in STR_KINDS and
                 (j == 0 or v["type"][tail_a] not in ZL_TYPES))
        d, ln = int(e["data"][k]), int(e["len"][k])
        payload = a[d:d + ln].copy()
        if ln == 0:
            payload = np.zeros(0, np.uint8)
        e["data"][k] = len(a)
        a = np.concatenate([a, payload])                # data + len == arena_cap
        classes[tail_a] = "arena"
    if tail_e is not None:
        b, c = int(v["elem_base"][tail_e]), int(v["n_elems"][tail_e])
        v["elem_base"][tail_e] = len(e)
        e = np.concatenate([e, e[b:b + c]])             # elem_base + n_elems == elem_cap
        classes[tail_e] = "elem_base"
    ecap, acap = len(e), len(a)

    for i, cls in picked.items():
        if i in (tail_e, tail_a):
            continue
        t, b, c = int(v["type"][i]), int(v["elem_base"][i]), int(v["n_elems"][i])
        r = int(rng.integers(0, 1 << 30))
        if cls == "type":
            v["type"][i] = (1, 3, 6, 10, 15, 255)[r % 6]
        elif cls == "enc":
            v["enc"][i] = (0, 1, 2, 3, 4, 8, 255)[r % 7]
        elif cls == "status":
            v["status"][i] = 1 + r % 14
        elif cls == "lru":
            v["lru"][i] = int(v["lru"][i]) | ((1 + r % 255) << 24)
        elif cls == "n_elems":
            v["n_elems"][i] = (c + 1, max(c - 1, 0), 0, 0xFFFFFFFF)[r % 4]
        elif cls == "elem_base":
            # the range ends at elem_cap (other values' descriptors), one past it, or past 2^32
            # (a 32-bit sum would wrap to 0)
            if c == 0:
                v["elem_base"][i] = (ecap, ecap + 1, 0xFFFFFFFF)[r % 3]
            else:
                v["elem_base"][i] = (ecap - c, ecap + 1 - c, (1 << 32) - c)[r % 3]
        elif cls == "kind":
            if c == 0:
                continue
            at = [j for j in (0, 3, 4, 5, c - 1) if j < c]
            e["kind"][b + at[r % len(at)]] = (0, 1, 2, 3, 4, 200)[(r >> 8) % 6]
        elif cls == "arena":
            ks = [b + j for j in range(c) if e["kind"][b + j] in STR_KINDS and (j == 0 or t not in ZL_TYPES)]
            if not ks or t == rr.T_SET_INTSET:
                continue
            k = ks[r % len(ks)]
            ln = int(e["len"][k])
            how = (r >> 8) % 5
            if how == 0:
                e["data"][k] = acap - ln                 # ends exactly at arena_cap (other bytes)
            elif how == 1:
                e["data"][k] = acap + 1 - ln             # one byte past
            elif how == 2:
                e["data"][k], e["len"][k] = 0xFFFFFFFFFFFFFFFF, 1   # data + len wraps to 0
            elif how == 3:
                e["len"][k] = 0xFFFFFFFF
            else:
                e["data"][k] = acap                      # at the end: fine only for len 0
        elif cls == "intset":
            if t != rr.T_SET_INTSET or c == 0:
                continue
            w = (2, 4, 8)[r % 3]
            v["enc"][i] = w
            for j in range(c):                           # make the rest fit any width
                e["data"][b + j] = (int(rng.integers(-30000, 30000))) & 0xFFFFFFFFFFFFFFFF
            edge = ((-(1 << 15) - 1, -(1 << 15), (1 << 15) - 1, 1 << 15,
                     -(1 << 31) - 1, -(1 << 31), (1 << 31) - 1, 1 << 31))[(r >> 8) % 8]
            e["data"][b + (r >> 16) % c] = edge & 0xFFFFFFFFFFFFFFFF
        elif cls == "odd":
            if t not in (rr.T_HASH_HT, rr.T_ZSET_SKIPLIST) or c < 2:
                continue
            v["n_elems"][i] = c - 1
        elif cls == "swap":
            if t != rr.T_ZSET_SKIPLIST or c < 2:
                continue
            j = b + 2 * ((r >> 8) % (c // 2))
            e[[j, j + 1]] = e[[j + 1, j]]
        elif cls == "zenc_rsv":
            if c == 0:
                continue
            j = b + r % c
            e["zenc"][j] = 1 + (r >> 8) % 255
            e["rsv"][j] = (r >> 16) & 0xFFFF
        elif cls == "string_n":
            if t != rr.T_STRING:
                continue
            v["n_elems"][i] = (0, 2)[r % 2]
        classes[i] = cls
    return v, e, a, classes


# ---- placement --------------------------------------------------------------------------------
def add_rejected(f, k):
    """k unencodable values of assorted causes, each owning one descriptor."""
    for j in range(k):
        c = j % 6
        if c == 0:
            f.add(rr.T_STRING, 0, [b"status"], status=1 + j % 14)
        elif c == 1:
            f.add((1, 3, 6, 10, 15, 255)[j % 6], 0, [b"type"])
        elif c == 2:
            f.add(rr.T_STRING, 0, [("raw", rr.K_SCORE, 0, 0, 0, 0)])
        elif c == 3:
            f.add(rr.T_SET_HT, 0, [("raw", rr.K_STR, 1 << 40, 5, 0, 0)])     # payload past the arena
        elif c == 4:
            f.add(rr.T_SET_INTSET, 3, [5])
        else:
            f.add(rr.T_HASH_HT, 0, [b"odd"])


def add_accepted(f, k, scale=1):
    for _ in range(k):
        _add_well_formed(f, int(f.rng.integers(0, N_SHAPES)), scale)


def block_edge_run(seed=1, run=320):
    """200 encodable values, `run` rejected ones (values 200..519: across the E1 block edges at
    256 and 512), then encodable ones to 700.  Returns the batch and the run's (first, last+1)."""
    f = Flat(seed)
    add_accepted(f, 200)
    add_rejected(f, run)
    add_accepted(f, 700 - 200 - run)
    return f.done(), (200, 200 + run)


def window_edge_run(delta, seed=2, run=300):
    """Strings filling the output up to byte ENC_WINDOW + delta, `run` rejected values (across the
    E1 block edge at 256), then encodable values, the first starting at ENC_WINDOW + delta: the
    window's first value is found past a run of size-0 values.  Returns the batch, the run's
    (first, last+1) and the byte the run sits at."""
    f = Flat(seed)
    for _ in range(150):
        f.add(rr.T_STRING, 0, [_word(f.rng, 9, 10)])          # 6 + 10 bytes each
    at, target = 150 * 16, ENC_WINDOW + delta
    while target - at > 900:
        f.add(rr.T_STRING, 0, [_word(f.rng, 593, 594)])       # 600 bytes each
        at += 600
    f.add(rr.T_STRING, 0, [_word(f.rng, target - at - 7, target - at - 6)])
    first = len(f.values)
    add_rejected(f, run)
    add_accepted(f, 400, scale=4)
    return f.done(), (first, first + run), target


def edges_rejected(which, seed=3, n=600):
    """`which`: "first", "last" or "all" — the value(s) rejected in a batch of n."""
    f = Flat(seed)
    if which == "all":
        add_rejected(f, n)
    else:
        if which == "first":
            add_rejected(f, 1)
        add_accepted(f, n - 1)
        if which == "last":
            add_rejected(f, 1)
    return f.done()


def big_task_block(seed=4):
    """The first E1 block holds more than ENC_MAPCAP descriptors (the task search instead of the
    task map): 20 Lists of 300 elements among short values; the Lists at tasks past 4,096 carry
    the defects (a SCORE among a List's elements; a skiplist pair swapped; a payload past the
    arena), one descriptor each.  Returns the batch and the indices of the defective values."""
    f = Flat(seed)
    rng = f.rng
    bad = []
    for j in range(20):
        items = [(_word(rng, 0, 6) if q % 3 else int(rng.integers(-10**12, 10**12))) for q in range(300)]
        if j in (15, 18):
            items[150 if j == 15 else 299] = ("raw", rr.K_SCORE, 1, 0, 0, 0)
            bad.append(len(f.values))
        f.add(rr.T_LIST_QUICKLIST, 0, items)
        add_accepted(f, 4)
    pairs = []
    for q in range(40):
        pairs += [b"m%02d" % q, ("score", _score_bits(40.0 - q))]
    pairs[60], pairs[61] = pairs[61], pairs[60]
    bad.append(f.add(rr.T_ZSET_SKIPLIST, 0, pairs))
    bad.append(f.add(rr.T_SET_HT, 0, [b"a", b"b", b"c", b"d", b"e", ("raw", rr.K_STR, 1 << 33, 1, 0, 0)]))
    add_accepted(f, 300)
    return f.done(), bad


def cap_settings(offsets, accepted, total):
    """The data_cap settings of one batch: the full output, a cap at a rejected value inside the
    batch (a run of them where there is one: the run holds no bytes, so the cap sits at the end of
    the value before it), a cap at an accepted value's end and one byte before it."""
    n = len(accepted)
    caps = [total + 16]
    rej = [i for i in range(n // 3, n) if not accepted[i]]
    if rej:
        caps.append(int(offsets[rej[len(rej) // 2]]))
    acc = [i for i in range(n // 2, n) if accepted[i]]
    if acc:
        end = int(offsets[acc[0] + 1])
        caps += [end, end - 1]
    return caps


# ---- tiling: large batches from a small base, for the grid-stride tests -------------------------
TILE_BASE = 61      # odd: a List at base index j sits at lane (j + 61 t) % 8 of its group in tile t
TILE_FILL = 2       # list_fill of the tiled batches: a List of three entries is two nodes


def _letters(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))    # never a decimal integer


def tiling_base(seed=11):
    """TILE_BASE values, short payloads: all eight types, a two-node List (under TILE_FILL), a List
    of one 13-byte node, a rejected value (status != 0), a STRING in the integer form, a body
    longer than a lane copies alone."""
    f = Flat(seed)
    rng = f.rng
    L = rr.T_LIST_QUICKLIST
    zl = pyoracle.build_ziplist([b"f", 3])
    f.add(L, 0, [_letters(rng, 3), 7, _letters(rng, 5)])                # two nodes
    f.add(rr.T_STRING, 0, [b"12345"])                                   # INT16
    f.add(L, 0, [5])                                                    # one node of 13 bytes
    f.add(rr.T_STRING, 0, [_letters(rng, 9)], status=3)                 # rejected
    f.add(rr.T_SET_HT, 0, [_letters(rng, 4), b"77", _letters(rng, 2)])
    f.add(rr.T_HASH_HT, 0, [_letters(rng, 3), _letters(rng, 6)])
    f.add(rr.T_ZSET_SKIPLIST, 0, [_letters(rng, 3), ("score", _score_bits(1.5))])
    f.add(rr.T_SET_INTSET, 2, [-3, 4, 500])
    f.add(rr.T_HASH_ZIPLIST, 0, [("zl", zl)])
    f.add(rr.T_ZSET_ZIPLIST, 0, [("zl", zl), 9])
    f.add(rr.T_STRING, 1, [-(2**40)])
    f.add(rr.T_STRING, 8, [_letters(rng, 70)])                          # copied by the whole wave
    f.add(L, 0, [])
    while len(f.values) < TILE_BASE:
        k = len(f.values) % 6
        if k == 0:
            f.add(L, 0, [(_letters(rng, int(rng.integers(0, 9))) if q % 2 else int(rng.integers(-900, 900)))
                         for q in range(int(rng.integers(1, 6)))])
        elif k == 1:
            f.add(rr.T_STRING, 0, [_letters(rng, int(rng.integers(0, 60)))])
        elif k == 2:
            f.add(rr.T_SET_HT, 0, [_letters(rng, int(rng.integers(1, 12))) for _ in range(int(rng.integers(0, 4)))])
        elif k == 3:
            f.add(rr.T_STRING, 1, [int(rng.integers(-2**33, 2**33))])
        elif k == 4:
            f.add(L, 0, [_letters(rng, 40), _letters(rng, 2)])
        else:
            f.add(rr.T_SET_INTSET, 4, [int(x) for x in rng.integers(-10**6, 10**6, int(rng.integers(0, 4)))])
    return f.done()


def tile_records(values, n):
    """n value records: the base's repeated over the same descriptors and arena, the last tile cut."""
    return np.tile(values, (n + len(values) - 1) // len(values))[:n].copy()


def tiling_reference(values, elems, arena, fill=TILE_FILL):
    """(base_ref, base_pays) for tile_expect: the reference on the base batch, and on each of its
    values alone for that value's share of totals.payload."""
    import rdb_reference as ref
    base_ref = ref.save_batch(values, elems, arena, fill)
    pays = [ref.save_batch(values[i:i + 1], elems, arena, fill)[4]["payload"] for i in range(len(values))]
    return base_ref, pays


def tile_expect(base_values,base_ref, base_pays, n, data_cap=None):
    """What rr_rdbsave_batch gives for tile_records(base_values, n), from the reference's answer
    for the base alone (base_ref: rdb_reference.save_batch without a data_cap) and base_pays, each
    base value's totals.payload when saved alone: (types, data, offsets, status, totals).  data
    holds offsets[n] bytes whatever data_cap is: offsets never decrease, so the values written are
    those before the first saveable one that ends past data_cap, and a test compares
    data[:offsets[j]] for that j.  tests/test_rdbsave.py holds this shortcut to save_batch on the
    tiled records themselves."""
    types, bdata, boffs, bstatus, _, _ = base_ref
    m = len(types)
    reps = (n + m - 1) // m
    sizes = np.tile(np.diff(boffs.astype(np.int64)), reps)[:n]
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes)
    total = int(offsets[n])
    status = np.tile(bstatus, reps)[:n].copy()
    pays = np.tile(np.asarray(base_pays, np.int64), reps)[:n]
    if data_cap is not None:
        status[(status == 0) & (offsets[1:] > np.uint64(data_cap))] = rr.E_CAPACITY
    data = np.tile(bdata, reps)[:total].copy()
    n_elems = int(np.tile(base_values["n_elems"].astype(np.int64), reps)[:n].sum())
    totals = {"n_elems": n_elems, "bytes": total,
              "n_bad": int((status != 0).sum()), "payload": int(pays[status == 0].sum())}
    return np.tile(types, reps)[:n].copy(), data, offsets, status, totals
