"""Inputs aimed at the snappy compressor's own paths (snz_comp_kernel / snz_pack_kernel in
redrock_old_amd/csrc/rr_snappy.hip) and a plain-Python model of compress_fragment as the kernel
runs it.  No tests here: tests/test_snappy_comp_streams.py pins the model to the CPU oracle and
proves the coverage conditions (CPU), tests/test_gpu_snappy_comp.py runs the inputs on the GPU.

The model (trace()) restates the kernel, not the serial loop:
  step 1   rounds of K = 16 probes.  Lane j holds the j-th probe of the skip schedule from the
           round's (P0, S0): position P, skip S, stride B = S >> 5, next position Pn = P + B; when
           S0 + K <= 64 every stride is 1 ('one'), else the per-lane schedule ('uniform' when all 16
           strides are equal, 'mixed' when the stride changes inside the round).  A lane is valid
           when Pn <= ip_limit.  Its candidate is the nearest earlier lane of the round with the same
           hash ('prev') or the table entry ('table').  The first lane that is invalid or matches
           is the stop lane sl; lanes below sl commit, and sl too when it matched; of the
           committing lanes only the last of each hash writes the table.
  step 2   Out::literal: the tag, then the bytes a byte a lane (len <= 64) or as destination-aligned
           dwords with a head and a tail, 4 x 64 dwords a loop trip.
  step 3   match_len in 64-lane steps, Out::copy's split at 68 / 64 / 60, the inserts at ip - 1
           and ip, repeated while the next four bytes match their table entry.
A scan only ever runs 'uniform' in its third round (S0 = 64: strides of 2 up to S = 94) and
'mixed' from the fourth on (from S = 96 a lane's stride grows within 16 probes).

trace(block, c0, mis, mut) -> (bytes, events); mut: a string of mutation letters, each a plausible
kernel defect (MUTATIONS).  Events are dicts: kind 'round' / 'lit' / 'copy' / 'exit'.
"""
import functools

import numpy as np

K = 16                    # RR_SNZ_K
MARGIN = 15               # kInputMarginBytes
TAB_MIN, TAB_MAX = 1 << 8, 1 << 14
FRAG = 1 << 16
WAVE = 64
GRID_CAP = 1 << 20        # grid_for's cap of snz_comp_kernel and snz_pack_kernel
PACK_WPB, PACK_U = 4, 4

MUTATIONS = {
    "a": "the candidate always comes from the table",
    "b": "the first lane of a hash writes the table, not the last",
    "c": "lanes past sl also commit",
    "d": "the hit lane does not commit",
    "e": "the whole round uses the stride of its first lane",
    "f": "Pn < ip_limit instead of <=",
    "g": "step 3 omits the insert at ip - 1",
    "h": "the same-round candidate is the farthest equal-hash lane, not the nearest",
    "i": "copy splits at len > 64 where the kernel has len >= 68",
    "j": "the short-copy test uses offset <= 2048",
    "J": "the short-copy test uses len <= 12",
    "k": "the literal tag switches at n1 <= 60",
}


def table_size(fn):
    return TAB_MAX if fn > TAB_MAX else TAB_MIN if fn < TAB_MIN else 2 << ((fn - 1).bit_length() - 1)


def hash32(v, shift):
    return ((v * 0x1e35a7bd) & 0xFFFFFFFF) >> shift


def varint32(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def schedule(P0, S0, mut=""):
    """(P, S, regime) of a round's 16 lanes."""
    if S0 + K <= 64:
        return [P0 + j for j in range(K)], [S0 + j for j in range(K)], "one"
    P, S = [P0], [S0]
    for _ in range(K - 1):
        B = (S0 if "e" in mut else S[-1]) >> 5
        P.append(P[-1] + B)
        S.append(S[-1] + B)
    strides = {s >> 5 for s in S}
    return P, S, "uniform" if len(strides) == 1 else "mixed"


class _Out:
    def __init__(self, mis, ev, mut):
        self.b = bytearray()
        self.mis, self.ev, self.mut = mis, ev, mut

    def put(self, n, v):
        self.b += (v & ((1 << (8 * n)) - 1)).to_bytes(n, "little")

    def literal(self, d, addr, frm, ln):
        """d[frm : frm + ln]; addr: the source address of d[frm] mod 4."""
        n1 = ln - 1
        if n1 < 60 or ("k" in self.mut and n1 <= 60):
            self.put(1, n1 << 2)
        else:
            count = ((n1.bit_length() - 1) >> 3) + 1
            self.put(1 + count, ((59 + count) << 2) | (n1 << 8))
        op = len(self.b)
        h = (4 - ((self.mis + op) & 3)) & 3
        nd = (ln - h) >> 2 if ln > WAVE else 0
        self.ev.append(dict(kind="lit", len=ln, path="byte" if ln <= WAVE else "dword", dst=(self.mis + op) & 3,
                            src=addr & 3, tail=ln & 3, trips=(nd + 4 * WAVE - 1) // (4 * WAVE)))
        self.b += d[frm:frm + ln]

    def copy64(self, offset, ln, allow_short, pieces):
        pieces.append((offset, ln))
        short_off = offset <= 2048 if "j" in self.mut else offset < 2048
        short_len = ln <= 12 if "J" in self.mut else ln < 12
        if allow_short and short_len and short_off:
            self.put(2, (1 + (((ln - 4) & 0xFF) << 2) + ((offset >> 3) & 0xe0)) | ((offset & 0xFF) << 8))
        else:
            self.put(3, ((2 + (((ln - 1) & 0xFF) << 2)) & 0xFF) | ((offset & 0xFFFF) << 8))

    def copy(self, offset, ln):
        pieces = []
        if ln < 12:
            self.copy64(offset, ln, True, pieces)
            return pieces
        if "i" in self.mut:
            while ln > 64:
                self.copy64(offset, 64, False, pieces)
                ln -= 64
        else:
            while ln >= 68:
                self.copy64(offset, 64, False, pieces)
                ln -= 64
            if ln > 64:
                self.copy64(offset, 60, False, pieces)
                ln -= 60
        self.copy64(offset, ln, True, pieces)
        return pieces


def _match_len(d, a, b, lim):
    """Bytes equal at d[a + i] and d[b + i] for b + i < lim."""
    n, m, c = lim - b, 0, 64
    while m < n:
        c = min(c, n - m)
        x, y = d[a + m:a + m + c], d[b + m:b + m + c]
        if x != y:
            return m + next(i for i in range(c) if x[i] != y[i])
        m += c
        c = 4096
    return n


def _fragment(blk, f, fn, addr, O, ev, mut, fi):
    """The fragment blk[f : f + fn] (addr: its first byte's address mod 4)."""
    ts = table_size(fn)
    shift = 32 - (ts.bit_length() - 1)
    table = [0] * ts
    end = f + fn

    def ld(k):      # (a lane past the fragment reads what follows it; past the data, zeros)
        return int.from_bytes(blk[f + k:f + k + 4], "little") if k < len(blk) - f else 0

    ip = next_emit = 0
    exit_ = "short"
    if fn >= MARGIN:
        ip_limit = fn - MARGIN
        ip = 1
        while exit_ == "short":
            P0, S0, rnd = ip, 32, 0
            while True:
                P, S, regime = schedule(P0, S0, mut)
                B = [s >> 5 for s in S]
                if "e" in mut and regime != "one":
                    B = [S0 >> 5] * K
                Pn = [P[j] + B[j] for j in range(K)]
                valid = [Pn[j] < ip_limit if "f" in mut else Pn[j] <= ip_limit for j in range(K)]
                x = [ld(p) for p in P]
                H = [hash32(v, shift) for v in x]
                near, far = [-1] * K, [-1] * K
                for j in range(K):
                    for i in range(j):
                        if H[i] == H[j]:
                            near[j] = i
                            far[j] = i if far[j] < 0 else far[j]
                pick = far if "h" in mut else near
                c = [table[H[j]] if pick[j] < 0 or "a" in mut else P[pick[j]] for j in range(K)]
                m = [valid[j] and x[j] == ld(c[j]) for j in range(K)]
                sl = next((j for j in range(K) if not valid[j] or m[j]), K)
                hit = sl < K and m[sl]
                commit = [j < sl or (hit and j == sl and "d" not in mut) or "c" in mut for j in range(K)]
                coll = [(j, ts, x[j] == ld(table[H[j]])) for j in range(min(sl, K - 1) + 1)
                        if valid[j] and near[j] >= 0 and x[j] != x[near[j]]]
                if sl < K:
                    ev.append(dict(kind="round", frag=fi, rnd=rnd, sl=sl, reason="hit" if hit else "limit",
                                   source=("prev" if near[sl] >= 0 else "table") if hit else None, regime=regime,
                                   collisions=coll, ts=ts))
                elif coll:
                    ev.append(dict(kind="round", frag=fi, rnd=rnd, sl=K, reason="none", source=None, regime=regime,
                                   collisions=coll, ts=ts))
                for j in range(K):
                    if not commit[j]:
                        continue
                    if "b" in mut:
                        writes = not any(commit[i] and H[i] == H[j] for i in range(j))
                    else:
                        writes = not any(commit[i] and near[i] == j for i in range(j + 1, K))
                    if writes:
                        table[H[j]] = P[j] & 0xFFFF
                if sl < K:
                    break
                P0, S0, rnd = Pn[K - 1], S[K - 1] + B[K - 1], rnd + 1
            if not hit:
                exit_ = "limit1"
                break
            ip, cand = P[sl], c[sl]
            O.literal(blk, addr + next_emit, f + next_emit, ip - next_emit)
            depth = 0
            while True:
                b0 = ip
                extra = _match_len(blk, f + cand + 4, f + ip + 4, end)
                ip += 4 + extra
                pieces = O.copy(b0 - cand, 4 + extra)
                next_emit = ip
                depth += 1
                e = dict(kind="copy", frag=fi, offset=b0 - cand, len=4 + extra, pieces=pieces, extra=extra,
                         end="fn" if ip == fn else "mismatch", steps=extra // WAVE + 1, depth=depth, rel=ip - ip_limit,
                         at=b0, cand=cand)
                ev.append(e)
                if ip >= ip_limit:
                    exit_ = "limit3"
                    break
                if "g" not in mut:
                    table[hash32(ld(ip - 1), shift)] = (ip - 1) & 0xFFFF
                cur = ld(ip)
                ch = hash32(cur, shift)
                cand = table[ch]
                table[ch] = ip & 0xFFFF
                if cur != ld(cand):
                    break
            if exit_ == "limit3":
                break
            ip += 1
    ev.append(dict(kind="exit", frag=fi, exit=exit_, fn=fn))
    if next_emit < fn:
        O.literal(blk, addr + next_emit, f + next_emit, fn - next_emit)


def trace(block, c0=0, mis=0, mut=""):
    """(the compressed bytes, the events) of a block at input address c0 whose slot starts at an
    address = mis mod 4."""
    block = bytes(block)
    ev = []
    O = _Out(mis & 3, ev, mut)
    O.b += varint32(len(block))
    for fi, f in enumerate(range(0, len(block), FRAG)):
        _fragment(block, f, min(FRAG, len(block) - f), (c0 + f) & 3, O, ev, mut, fi)
    return bytes(O.b), ev


# ---- alignment: blocks behind fillers ---------------------------------------------------------------
def slot_size(n):
    return 32 + n + n // 6       # snz_bound_kernel (MaxCompressedLength)


def distinct(n, base=100):
    """n bytes in which no four consecutive bytes occur twice: the 16-bit values (i + base) * 513,
    low byte first (as tests/test_gpu_lz4_window.py's _distinct); base + n / 2 < 65536."""
    v = ((np.arange((n + 1) // 2 + 1, dtype=np.uint32) + base) * 513).astype("<u2")
    return v.view(np.uint8)[:n].tobytes()


@functools.lru_cache(None)
def _filler_table():
    """(c0 step & 15, slot step & 3) -> the shortest one or two filler lengths that give it."""
    best = {}
    lens = range(48)
    for a in lens:
        for b in [None] + list(lens):
            ls = (a,) if b is None else (a, b)
            key = (sum(ls) & 15, sum(slot_size(x) for x in ls) & 3)
            if key not in best or (len(ls), sum(ls)) < (len(best[key]), sum(best[key])):
                best[key] = ls
    assert len(best) == 64
    return best


def place(blocks, aligns):
    """The blocks with fillers of 0..47 distinct bytes in front of each, so that block i starts at an
    input address = aligns[i][0] mod 16 in a slot at aligns[i][1] mod 4 (the slots start 8-aligned:
    rr_launch_snappy_compress).  Returns (all blocks, the indices of the given ones)."""
    out, real, c0, so = [], [], 0, 0
    for b, (a, m) in zip(blocks, aligns):
        key = ((a - c0) & 15, (m - so) & 3)
        if key != (0, 0):
            for n in _filler_table()[key]:
                out.append(distinct(n, 40000 + 7 * len(out)))
                c0, so = c0 + n, so + slot_size(n)
        assert (c0 & 15, so & 3) == (a & 15, m & 3)
        real.append(len(out))
        out.append(b)
        c0, so = c0 + len(b), so + slot_size(len(b))
    return out, real


def starts(blocks):
    """(c0, slot offset) of every block of a batch."""
    c0 = so = 0
    out = []
    for b in blocks:
        out.append((c0, so))
        c0, so = c0 + len(b), so + slot_size(len(b))
    return out


def pack(blocks):
    """(data, offsets) of a batch, data zero-padded to a multiple of 16 bytes."""
    offs = np.zeros(len(blocks) + 1, np.uint64)
    offs[1:] = np.cumsum([len(b) for b in blocks])
    raw = b"".join(blocks)
    data = np.zeros(((len(raw) + 15) & ~15) or 16, np.uint8)
    data[:len(raw)] = np.frombuffer(raw, np.uint8)
    return data, offs


# ---- rounds -------------------------------------------------------------------------------------------
def gen_round(seed):
    """15..700 random bytes with up to three planted repeats at distances 1..59."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(15, 701))
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    for _ in range(int(rng.integers(0, 4))):
        dist, ln = int(rng.integers(1, 60)), int(rng.integers(4, 13))
        if n > dist + ln:
            at = int(rng.integers(dist, n - ln))
            for i in range(ln):
                d[at + i] = d[at - dist + i]
    return bytes(d)


def limit_block(regime, sl):
    """Distinct bytes (no match anywhere) of the length at which the first scan runs into ip_limit
    at lane sl of its first ('one'), third ('uniform') or fourth ('mixed') round."""
    P0, S0 = 1, 32
    for _ in range({"one": 0, "uniform": 2, "mixed": 3}[regime]):
        P, S, _ = schedule(P0, S0)
        P0, S0 = P[-1] + (S[-1] >> 5), S[-1] + (S[-1] >> 5)
    P, S, r = schedule(P0, S0)
    assert r == regime
    return distinct(P[sl] + (S[sl] >> 5) - 1 + MARGIN, 300)      # Pn = ip_limit + 1 at lane sl


# seeds of gen_round() whose traces cover, with limit_block(), every reachable (sl, source, regime)
# hit cell (a greedy cover of a search over 20000 seeds; test_snappy_comp_streams.py holds the cells)
ROUND_SEEDS = (70, 129, 172, 197, 236, 361, 365, 399, 451, 501, 538, 636, 930, 977, 1009, 1121, 1232, 1326, 1464, 1600,
               1603, 1708, 1854, 1888, 2159, 2270, 2681, 3090, 3940, 4236, 4698, 5421, 6278, 6905, 9625, 11082, 12262,
               13670, 16348, 18186)
# seeds of gen_round() with a same-round collision at every lane 1..15 of a 256-entry table, the
# pair's table entry matching and not
COLLISION_SEEDS = (54, 251, 551, 1121, 1383, 1927, 2156, 3277, 3953, 4149, 5940, 8363, 14227, 18901)


def hit_at_limit_block():
    """A match at position 13 = ip_limit - 1: the last position whose lane is still valid (Pn = ip_limit)."""
    X = distinct(8, 500)
    b = b"z" + X + distinct(4, 600) + X + distinct(8, 650)[::-1]
    assert len(b) - MARGIN - 1 == 13
    return b


def family_rounds():
    out = [(f"seed{s}", gen_round(s)) for s in ROUND_SEEDS] + [("hit_at_limit", hit_at_limit_block())]
    out += [(f"limit_{r}_{sl}", limit_block(r, sl)) for r in ("one", "uniform", "mixed") for sl in range(K)]
    return out


# ---- collisions ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def equal_hash_strings(shift=18):
    """{d: 4 + d bytes whose dwords at 0 and at d differ and have equal hash32} for d = 1..3, and
    (A, B) two such dwords apart (d = 4), by a seeded search."""
    rng = np.random.default_rng(2024)
    out = {}
    for d in (1, 2, 3, 4):
        while d not in out:
            s = rng.integers(1, 256, (4096, 4 + d), dtype=np.uint8)
            a = np.ascontiguousarray(s[:, :4]).view("<u4")[:, 0]
            b = np.ascontiguousarray(s[:, d:d + 4]).view("<u4")[:, 0]
            ha, hb = (a * np.uint32(0x1e35a7bd)) >> np.uint32(shift), (b * np.uint32(0x1e35a7bd)) >> np.uint32(shift)
            k = np.flatnonzero((ha == hb) & (a != b))
            if k.size:
                out[d] = s[k[0]].tobytes()
    return out


def collision_block(lane, entry_matches, n, third=False):
    """n bytes (a 16384-entry table: n > 8192) whose second round (positions 17..32, stride 1) has
    dwords A at lane 0 and B at `lane` with equal hash and different bytes.  entry_matches: the block
    starts with B, which an empty table entry points at, so taking the candidate from the table would
    match; else B stands again at position 41 (the third round's lane 4), where the table must hold
    lane `lane`'s position, not lane 0's.  third: B also at a lane between, so the nearest equal-hash
    lane matches and the farthest does not."""
    eq = equal_hash_strings()
    d = min(lane, 4)
    s = eq[d]
    A, B = s[:4], s[d:d + 4]
    buf = bytearray(distinct(n, 9000 + 97 * lane))
    if entry_matches:
        buf[0:4] = B
    if lane < 4:
        buf[17:17 + len(s)] = s
    else:
        buf[17:21] = A
        buf[17 + lane:21 + lane] = B
    if third:
        assert lane >= 8
        buf[17 + 4:17 + 8] = B          # lane 4: B, between A (lane 0) and B (`lane`)
    if not entry_matches:
        buf[41:45] = B
    return bytes(buf)


def family_collisions():
    out = [(f"seed{s}", gen_round(s)) for s in COLLISION_SEEDS]
    for lane in range(1, K):
        for em in (False, True):
            out.append((f"t16k_lane{lane}_{'match' if em else 'nomatch'}", collision_block(lane, em, 16384)))
    for lane in (8, 15):
        out.append((f"t16k_lane{lane}_third", collision_block(lane, False, 16384, third=True)))
    for lane in (1, 5, 15):
        for em in (False, True):
            out.append((f"t64k_lane{lane}_{'match' if em else 'nomatch'}", collision_block(lane, em, 65536)))
    return out


def family_collisions_small():
    """The collision inputs the Python model runs mutations on: all but most of the 16 / 64 KiB ones."""
    return [(n, b) for n, b in family_collisions() if len(b) < 8192 or "third" in n or "lane5" in n or "lane15" in n]


# ---- step 3 -------------------------------------------------------------------------------------------
ML_EXTRA = (0, 1, 59, 60, 63, 64, 65, 127, 128, 129)


def words(n, base):
    """n four-byte words with distinct first bytes and no four consecutive bytes twice."""
    return [bytes([16 + i + base, 200 - i, 3 * i + 1, 255 - 5 * i & 0xFF]) for i in range(n)]


def chain_block(depth):
    """Eight words at positions 1..32 (every one inserted by the first scan's two rounds), then from
    position 33 (the third round's lane 0) depth words in an order in which none follows its
    neighbour: depth back-to-back copies of four bytes, then distinct bytes."""
    w = words(8, 0)
    order = [0, 2, 4, 6, 1, 3, 5, 7, 2, 5, 0, 3, 6, 2, 7, 1]      # (no pair twice, none (i, i + 1) or (7, 0))
    assert depth <= len(order)
    return b"z" + b"".join(w) + b"".join(w[k] for k in order[:depth]) + distinct(24, 5000)


def insert_block(with_later=True):
    """A copy of six bytes ends at 19; four bytes that start at its last byte stand again at 30: a
    match only the insert at ip - 1 = 18 finds."""
    X, q = distinct(8, 700), distinct(11, 900)
    b = b"z" + X + distinct(4, 800) + X[:6] + q
    assert len(b) == 30
    return b + (X[5:6] + q[:3] if with_later else b"") + distinct(24, 1000)


def exit_block(rel):
    """A copy of 8 bytes that ends at ip_limit + rel (rel -1, 0, 1), or runs to fn (rel 15: 20 bytes)."""
    X = distinct(20, 1200)
    if rel == MARGIN:
        return b"z" + X + distinct(4, 1300) + X
    return b"z" + X[:8] + distinct(4, 1300) + X[:8] + distinct(MARGIN - rel, 1400)[::-1]


def matchlen_block(extra, end):
    """A match of 4 + extra bytes that ends by a mismatch, or by reaching fn (extra >= 12: a match
    starts below ip_limit = fn - 15, so one that reaches fn has at least 16 bytes)."""
    return copy_block(4 + extra, 300, tail=end == "mismatch")


def family_step3():
    out = [(f"chain{d}", chain_block(d)) for d in (1, 2, 16)]
    out += [("insert", insert_block()), ("insert_without", insert_block(False))]
    out += [(f"exit{rel:+d}", exit_block(rel)) for rel in (-1, 0, 1, MARGIN)]
    out += [(f"ml{e}_{end}", matchlen_block(e, end)) for e in ML_EXTRA for end in ("mismatch", "fn")
            if end == "mismatch" or e >= 12]
    return out


# ---- copies -------------------------------------------------------------------------------------------
COPY_LENS = tuple(range(4, 13)) + tuple(range(63, 71)) + (124, 127, 128, 131, 132, 4000)
COPY_OFFS = (1, 4, 2047, 2048, 2049, 65535 - 16, 65536)      # (65536: the largest the fragment allows)


def copy_offset(L, D):
    """The offset a copy of L bytes gets for the nominal offset D: a match starts at or below
    fn - 16 and ends at or below fn, and its source at or after 0."""
    return min(D, FRAG - 16, FRAG - L)


def copy_block(L, D, tail=True):
    """One copy of exactly L bytes at offset D = copy_offset(L, D), the last of the block's copies.
    Period D: eight distinct bytes H, then (D >= 40) a run of one 8-byte unit up to D bytes, which
    the compressor covers with one long copy that ends where H stands again; step 3 looks H up
    there and finds its first position.  The period's first L bytes follow, then (tail) a byte that
    breaks the match and distinct bytes (none when the match ends at the fragment's end)."""
    D = copy_offset(L, D)
    first = 0 if D + L + 16 > FRAG else 1                # (position 0: found through an empty table entry)
    if D < 40:
        period = distinct(D, 2100)
    else:
        unit = bytes([7, 9, 11, 13, 15, 17, 19, 21])
        period = distinct(8, 2100) + (unit * (D // 8 + 1))[:D - 8]
    rep = (period * (L // D + 2))[:L + 1]
    body = b"z" * first + period + rep[:L]
    if len(body) >= FRAG or not tail:
        return body[:FRAG]
    return (body + bytes([rep[L] ^ 0x80]) + distinct(24, 2300)[::-1])[:FRAG]


def family_copies():
    seen, out = set(), []
    for L in COPY_LENS:
        for D in COPY_OFFS:
            key = (L, copy_offset(L, D))
            if key not in seen:
                seen.add(key)
                out.append((f"copy_L{L}_D{key[1]}", copy_block(L, D)))
    return out


def family_copies_small():
    return [(n, b) for n, b in family_copies() if len(b) < 8192]


# ---- literals -----------------------------------------------------------------------------------------
LIT_LENS = (1, 59, 60, 61, 63, 64, 65, 66, 67, 68, 255, 256, 257, 1027, 1028, 1029, 1030, 1031, 2100)
LIT_PREFIX = 33


def literal_block(n):
    """A literal of 17, a copy of 16 that ends at byte 33 (found at 17 <= fn - 16 for any n >= 0), then
    n distinct bytes: the block's last literal has exactly n bytes."""
    X = distinct(16, 2500)
    return b"z" + X + X + distinct(n, 2600 + n)[::-1]


def family_literals():
    """(name, block, (c0 & 15, slot & 3)): every length at 16 placements that give every
    (destination & 3, source & 3) pair, and a whole incompressible fragment (one literal of 65536)
    at four of them."""
    out = []
    for n in LIT_LENS:
        for a in range(16):
            out.append((f"lit{n}_c{a}_m{a >> 2}", literal_block(n), (a, (a >> 2) & 3)))
    whole = distinct(FRAG, 11)
    for a in (0, 5, 10, 15):
        out.append((f"lit65536_c{a}_m{a >> 2}", whole, (a, (a >> 2) & 3)))
    return out


# ---- sizes --------------------------------------------------------------------------------------------
SIZES = tuple(range(81)) + (255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 65535, 65536, 65537,
                           2 * 65536 - 1, 2 * 65536, 2 * 65536 + 1, 200001)


def family_sizes():
    """Random bytes of every size (strides above 1), and bytes of a four-letter alphabet (copies up
    to the block's end) of the sizes up to 4097; the last block is 200001 random bytes, behind a
    block of 0..15 bytes that makes the batch's bytes a multiple of 16: the last block ends exactly
    at a data_cap that include/rr_snappy.h allows."""
    rng = np.random.default_rng(77)
    out = []
    for n in SIZES:
        if n <= 4097:
            out.append((f"low{n}", rng.integers(0, 4, n, dtype=np.uint8).tobytes()))
        if n == SIZES[-1]:
            out.append(("pad", rng.integers(0, 256, -(sum(len(b) for _, b in out) + n) & 15, dtype=np.uint8).tobytes()))
        out.append((f"rand{n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    assert sum(len(b) for _, b in out) % 16 == 0
    return out


def family_sizes_small():
    return [(n, b) for n, b in family_sizes() if len(b) <= 4097]


# ---- the pack kernel ----------------------------------------------------------------------------------
PACK_LENS = (1, 3, 15, 16, 17, 31, 32, 33, 4111, 4112, 4113, 9005)


def pack_input(clen):
    """Distinct bytes that compress to exactly clen bytes (a preamble, one literal tag, the bytes)."""
    if clen == 1:
        return b""
    n = clen - 2 if clen <= 62 else clen - 5        # (1 + 1 + n; 2 + 3 + n for 256 < n < 16384)
    return distinct(n, 3100)


def family_pack():
    """Every compressed length of PACK_LENS at every out_offs & 15, set by empty blocks (a byte
    each) in front."""
    out, at = [], 0
    for clen in PACK_LENS:
        for a in range(16):
            while at & 15 != a:
                out.append(("empty", b""))
                at += 1
            out.append((f"pack{clen}_o{a}", pack_input(clen)))
            at += clen
    return out


# ---- grid strides, 4 GiB ------------------------------------------------------------------------------
GRID_N = 4 * GRID_CAP + 3001
GRID_BASE = 61


def grid_base():
    """61 blocks of 0..3 bytes."""
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 4, GRID_BASE)]


def tile_offsets(base_offs, n):
    """The offsets of n blocks that repeat the base's blocks (base_offs: len(base) + 1 values)."""
    nb = len(base_offs) - 1
    t = -(-n // nb)
    sizes = np.tile(np.diff(base_offs.astype(np.int64)), t)[:n]
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(sizes, out=offs[1:])
    return offs
