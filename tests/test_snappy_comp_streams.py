"""The inputs of tests/snappy_comp_streams.py and its model of the compressor's rounds against the
CPU oracle, before any GPU sees them: the model without a mutation writes the oracle's bytes on every
family input and on a seeded fuzz; the families' traces hold every cell tests/test_gpu_snappy_comp.py
relies on (asserted as sets, the missing cells printed); every mutation of the model (a plausible
kernel defect each) changes the output of a named input of the family meant to catch it; and the
model's constants are the source's.

Cells that no input can reach, by the kernel's own conditions:
  - a hit at lane 0 from an earlier lane (there is none);
  - a match that ends at fn with fewer than 12 bytes past its first four: a match starts at
    ip < ip_limit = fn - 15, so one that reaches fn has at least 16 bytes;
  - a compressed length of 2 (an empty block gives 1 byte, a block of one byte 3): the pack family
    has 3 in its place;
  - offsets past 65520 (a match starts at or below fn - 16 of a 64 KiB fragment) and, for a
    length L, past 65536 - L: copy_offset() caps the nominal offsets.
The 200001-byte block has four fragments (3 x 65536 + 3393), the last with a 4096-entry table."""
import collections
import os
import re

import numpy as np
import pytest

import snappy_comp_streams as cs
from oracle import cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = ("one", "uniform", "mixed")


def _named(fam):
    return [(n, b, (0, 0)) for n, b in fam] if len(fam[0]) == 2 else fam


FAMILIES = {
    "rounds": cs.family_rounds, "collisions": cs.family_collisions, "step3": cs.family_step3,
    "copies": cs.family_copies, "literals": cs.family_literals, "sizes": cs.family_sizes, "pack": cs.family_pack,
}


@pytest.fixture(scope="module")
def traces():
    """{family: [(name, block, events)]}, the model's bytes compared with the oracle's on the way."""
    out = {}
    for fam, make in FAMILIES.items():
        out[fam] = []
        for name, b, (a, m) in _named(make()):
            got, ev = cs.trace(b, a, m)
            assert got == cpu.snappy_compress(b), f"{fam}/{name}: the model differs from the oracle"
            out[fam].append((name, b, ev))
    return out


def _exit(ev):
    return [e for e in ev if e["kind"] == "exit"][-1]


def _missing(want, have, what):
    miss = sorted(set(want) - set(have), key=repr)
    assert not miss, f"{what}: {len(miss)} cells missing: {miss[:40]}"


def test_constants_are_the_source():
    src = open(os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_snappy.hip")).read()
    assert int(re.search(r"^#define RR_SNZ_K (\d+)$", src, re.M).group(1)) == cs.K
    assert int(re.search(r"^#define RR_SNZ_SPARSE (\d+)$", src, re.M).group(1)) == 0
    assert int(re.search(r"^#define RR_SNZ_FRAG (\d+)$", src, re.M).group(1)) == 0
    assert int(re.search(r"constexpr uint32_t MARGIN = (\d+);", src).group(1)) == cs.MARGIN
    assert int(re.search(r"constexpr uint32_t WAVE = (\d+);", src).group(1)) == cs.WAVE
    assert 1 << int(re.search(r"constexpr uint32_t FRAG = 1u << (\d+);", src).group(1)) == cs.FRAG
    assert 1 << int(re.search(r"constexpr uint32_t TAB_MIN = 1u << (\d+);", src).group(1)) == cs.TAB_MIN
    assert 1 << int(re.search(r"constexpr uint32_t TAB_MAX = 1u << (\d+);", src).group(1)) == cs.TAB_MAX
    m = re.search(r"constexpr uint32_t PACK_WPB = (\d+), PACK_U = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (cs.PACK_WPB, cs.PACK_U)
    # the dense pass's grid and the pack kernel's, in rr_launch_snappy_compress
    body = src[src.index('extern "C" hipError_t rr_launch_snappy_compress'):]
    assert re.search(r"snz_comp_kernel<false>, dim3\(grid_for\(n, 1u << 20\)\), dim3\(WAVE\), smem,", body)
    assert re.search(r"snz_pack_kernel, dim3\(grid_for\(\(n \+ PACK_WPB - 1\) / PACK_WPB, 1u << 20\)\)", body)
    assert cs.GRID_CAP == 1 << 20 and cs.GRID_N > cs.PACK_WPB * cs.GRID_CAP
    assert re.search(r"slot_offs\[i\] = 32 \+ len \+ len / 6;", src) and cs.slot_size(13) == 47
    for fn, ts in ((0, 256), (256, 256), (257, 512), (4096, 4096), (4097, 8192), (16384, 16384), (65536, 16384), (3393, 4096)):
        assert cs.table_size(fn) == ts


def test_model_equals_oracle_on_a_fuzz():
    """Seeded: gen_round's inputs, low-entropy bytes, text-like periods, at any c0 / slot alignment."""
    rng = np.random.default_rng(99)
    for s in range(20000, 20400):
        b = cs.gen_round(s)
        assert cs.trace(b, s & 15, s >> 4 & 3)[0] == cpu.snappy_compress(b), s
    for k in range(120):
        n = int(rng.integers(0, 3000))
        b = rng.integers(0, int(rng.integers(2, 40)), n, dtype=np.uint8).tobytes()
        assert cs.trace(b)[0] == cpu.snappy_compress(b), ("low", k)
    for k in range(6):
        n = int(rng.integers(66000, 140000))
        unit = rng.integers(0, 256, int(rng.integers(20, 3000)), dtype=np.uint8).tobytes()
        b = bytearray((unit * (n // len(unit) + 1))[:n])
        for at in rng.integers(0, n, 200):
            b[int(at)] ^= 1
        assert cs.trace(bytes(b))[0] == cpu.snappy_compress(bytes(b)), ("period", k)


def test_placement():
    """place() puts block i at its (c0 & 15, slot & 3) with fillers that are blocks themselves."""
    fam = cs.family_literals()[:80]
    blocks, real = cs.place([b for _, b, _ in fam], [al for _, _, al in fam])
    st = cs.starts(blocks)
    for r, (_, b, (a, m)) in zip(real, fam):
        assert blocks[r] == b and (st[r][0] & 15, st[r][1] & 3) == (a, m)
    assert all(len(b) < 48 for i, b in enumerate(blocks) if i not in set(real))
    data, offs = cs.pack(blocks)
    assert data.size % 16 == 0 and 0 <= data.size - int(offs[-1]) < 16


def test_rounds_cells(traces):
    hits, limits = set(), set()
    for name, _, ev in traces["rounds"]:
        for e in ev:
            if e["kind"] == "round" and e["reason"] == "hit":
                hits.add((e["sl"], e["source"], e["regime"]))
            if e["kind"] == "round" and e["reason"] == "limit":
                limits.add((e["sl"], e["regime"]))
    want = {(sl, s, r) for sl in range(cs.K) for s in ("prev", "table") for r in REGIMES} - {(0, "prev", r) for r in REGIMES}
    _missing(want, hits, "rounds: (sl, source, regime) of a hit")
    assert not {h for h in hits if h[0] == 0 and h[1] == "prev"}
    _missing({(sl, r) for sl in range(cs.K) for r in REGIMES}, limits, "rounds: (sl, regime) of a limit stop")
    # the hit whose lane is the last valid one (Pn == ip_limit)
    ev = dict((n, e) for n, _, e in traces["rounds"])["hit_at_limit"]
    assert [e["at"] for e in ev if e["kind"] == "copy"] == [13] and _exit(ev)["fn"] - cs.MARGIN == 14


def test_collision_cells(traces):
    have = set()
    for name, b, ev in traces["collisions"]:
        for e in ev:
            if e["kind"] == "round":
                have |= set(e["collisions"])
    want = {(lane, ts, em) for lane in range(1, cs.K) for ts in (256, 16384) for em in (False, True)}
    _missing(want, have, "collisions: (lane, table size, the pair's table entry matches)")
    frag64 = set()
    for name, b, ev in traces["collisions"]:
        if len(b) == 65536:
            frag64 |= {c for e in ev if e["kind"] == "round" for c in e["collisions"]}
    _missing({(lane, 16384, em) for lane in (1, 5, 15) for em in (False, True)}, frag64, "collisions in a 64 KiB fragment")
    # the planted blocks do what collision_block() says: without a table match, the second B is found
    # at lane `lane`'s position (a copy from 41 to 17 + lane); with three equal hashes, at the nearest
    for name, b, ev in traces["collisions"]:
        if name.startswith("t16k") or name.startswith("t64k"):
            lane = int(re.search(r"lane(\d+)", name).group(1))
            copies = [(e["at"], e["cand"]) for e in ev if e["kind"] == "copy"]
            if name.endswith("nomatch"):
                assert (41, 17 + lane) in copies, (name, copies[:4])
            elif name.endswith("third"):
                assert (17 + lane, 21) in copies, (name, copies[:4])
            else:
                assert not [c for c in copies if c[0] < 40], (name, copies[:4])


def _runs(ev):
    """The depths of the step-3 loops: copies back to back."""
    out = []
    for e in ev:
        if e["kind"] == "copy":
            if e["depth"] == 1:
                out.append(1)
            else:
                out[-1] = e["depth"]
    return out


def test_step3_cells(traces):
    by = {n: ev for n, _, ev in traces["step3"]}
    depths = {d for ev in by.values() for d in _runs(ev)}
    _missing({1, 2, 16}, depths, "step 3: copies back to back")
    assert _runs(by["chain16"]) == [16] and _runs(by["chain2"]) == [2] and _runs(by["chain1"]) == [1]
    # the match only the insert at ip - 1 finds
    c = [(e["at"], e["cand"]) for e in by["insert"] if e["kind"] == "copy"]
    assert c == [(13, 1), (30, 18)], c
    assert [(e["at"], e["cand"]) for e in by["insert_without"] if e["kind"] == "copy"] == [(13, 1)]
    rel = {e["rel"] for ev in by.values() for e in ev if e["kind"] == "copy"}
    _missing({-1, 0, 1, cs.MARGIN}, rel, "step 3: ip - ip_limit after a copy")
    assert [e["rel"] for e in by["exit-1"] if e["kind"] == "copy"] == [-1] and _exit(by["exit-1"])["exit"] == "limit1"
    for r in (0, 1, cs.MARGIN):
        assert _exit(by[f"exit{r:+d}"])["exit"] == "limit3", r
    exits = {e["exit"] for fam in traces.values() for _, _, ev in fam for e in ev if e["kind"] == "exit"}
    _missing({"short", "limit1", "limit3"}, exits, "exits")
    ml = {(e["extra"], e["end"]) for ev in by.values() for e in ev if e["kind"] == "copy"}
    want = {(x, "mismatch") for x in cs.ML_EXTRA} | {(x, "fn") for x in cs.ML_EXTRA if x >= 12}
    _missing(want, ml, "match_len: (bytes past the first four, how it ends)")
    steps = {e["steps"] for ev in by.values() for e in ev if e["kind"] == "copy"}
    _missing({1, 2, 3}, steps, "match_len: 64-lane steps")


def test_copy_cells(traces):
    have = {}
    for name, b, ev in traces["copies"]:
        for e in ev:
            if e["kind"] == "copy":
                have[(e["len"], e["offset"])] = e["pieces"]
    want = {(L, cs.copy_offset(L, D)) for L in cs.COPY_LENS for D in cs.COPY_OFFS}
    _missing(want, have, "copies: (length, offset)")
    offs = {o for _, o in want}
    assert offs >= {1, 4, 2047, 2048, 2049, 65519, 65520} and (4000, 65536 - 4000) in want
    # Out::copy's pieces at its thresholds
    assert [l for _, l in have[(64, 2048)]] == [64] and [l for _, l in have[(65, 2048)]] == [60, 5]
    assert [l for _, l in have[(67, 4)]] == [60, 7] and [l for _, l in have[(68, 4)]] == [64, 4]
    assert [l for _, l in have[(132, 1)]] == [64, 64, 4] and [l for _, l in have[(131, 1)]] == [64, 60, 7]
    assert len(have[(4000, 2049)]) == 63
    # every copy family block has its copy as the last one
    for name, b, ev in traces["copies"]:
        L, D = (int(x) for x in re.match(r"copy_L(\d+)_D(\d+)", name).groups())
        last = [e for e in ev if e["kind"] == "copy"][-1]
        assert (last["len"], last["offset"]) == (L, D), (name, last)


def test_literal_cells(traces):
    have = collections.defaultdict(set)
    trips = set()
    for name, b, ev in traces["literals"]:
        e = [e for e in ev if e["kind"] == "lit"][-1]
        have[e["len"]].add((e["dst"], e["src"]))
        trips.add(e["trips"])
        assert e["path"] == ("byte" if e["len"] <= 64 else "dword") and e["tail"] == e["len"] & 3
    pairs = {(d, s) for d in range(4) for s in range(4)}
    for n in cs.LIT_LENS:
        _missing(pairs, have[n], f"literal of {n}: (destination & 3, source & 3)")
    assert len(have[65536]) == 4
    _missing({0, 1, 2, 3, 64}, trips, "literals: trips of the 4 x 64-dword loop")
    # the tag forms: the length in the tag byte up to 60, then in one byte up to 256, then in two (a
    # fragment's longest literal, 65536, still has two)
    assert {60, 61, 256, 257, 65536} <= set(have)


def test_size_and_pack_cells(traces):
    sizes = {len(b) for _, b, _ in traces["sizes"]}
    _missing(set(range(81)) | {255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 65535, 65536, 65537,
                               131071, 131072, 131073, 200001}, sizes, "sizes")
    name, b, ev = traces["sizes"][-1]
    assert len(b) == 200001 and sum(len(b) for _, b, _ in traces["sizes"]) % 16 == 0      # (the last block ends at data_cap)
    assert [e["fn"] for e in ev if e["kind"] == "exit"] == [65536, 65536, 65536, 3393] and cs.table_size(3393) == 4096
    strides = {e["regime"] for _, _, ev in traces["sizes"] for e in ev if e["kind"] == "round"}
    assert "mixed" in strides
    at, have = 0, set()
    for name, b, _ in traces["pack"]:
        n = len(cpu.snappy_compress(b))
        if name != "empty":
            have.add((n, at & 15))
        at += n
    _missing({(n, a) for n in cs.PACK_LENS for a in range(16)}, have, "pack: (compressed length, out_offs & 15)")
    assert max(cs.PACK_LENS) > 16 * (2 * cs.PACK_U * cs.WAVE)        # a third trip of the PACK_U * WAVE loop


def test_grid_tiling_holds_to_the_oracle():
    """The expected output of the grid-stride test is the oracle's on 61 blocks, tiled: 3 x 61 blocks
    compressed by the oracle give the same bytes and offsets."""
    base = cs.grid_base()
    assert len(base) == cs.GRID_BASE and {len(b) for b in base} == {0, 1, 2, 3}
    want = [cpu.snappy_compress(b) for b in base]
    boffs = np.zeros(len(base) + 1, np.uint64)
    boffs[1:] = np.cumsum([len(w) for w in want])
    three = [cpu.snappy_compress(b) for b in base * 3]
    n = 3 * len(base) - 7
    offs = cs.tile_offsets(boffs, n)
    assert [int(x) for x in np.diff(offs)] == [len(w) for w in three[:n]]
    assert (b"".join(want) * 3)[:int(offs[-1])] == b"".join(three[:n])
    assert cs.GRID_N == 4 * (1 << 20) + 3001


# ---- mutations -----------------------------------------------------------------------------------------
# mutation -> (the family meant to catch it, the cell)
CATCHES = {
    "a": ("collisions", "a same-round collision whose table entry matches"),
    "b": ("collisions", "a same-round collision, its hash probed again later"),
    "c": ("rounds", "a hit below lane 15 with a later lane's position probed again"),
    "d": ("rounds", "a hit whose position a later probe matches"),
    "e": ("rounds", "a hit or a limit stop in a 'mixed' round"),
    "f": ("rounds", "the hit at the last valid lane (Pn == ip_limit)"),
    "g": ("step3", "the match only the insert at ip - 1 finds"),
    "h": ("collisions", "three lanes of one hash, the nearest equal to the probe"),
    "i": ("copies", "copy lengths 65..67"),
    "j": ("copies", "offset 2048 with a length below 12"),
    "J": ("copies", "length 12 with an offset below 2048"),
    "k": ("literals", "a literal of 61 bytes"),
}
SMALL = {"collisions": cs.family_collisions_small, "copies": cs.family_copies_small, "sizes": cs.family_sizes_small}


@pytest.mark.parametrize("mut", sorted(cs.MUTATIONS))
def test_mutation_is_caught(mut):
    assert set(CATCHES) == set(cs.MUTATIONS)
    fam, cell = CATCHES[mut]
    moved = []
    for name, b, (a, m) in _named(SMALL.get(fam, FAMILIES[fam])()):
        if fam == "literals" and a != 0:
            continue
        if cs.trace(b, a, m, mut)[0] != cs.trace(b, a, m)[0]:
            moved.append(name)
    print(f"\nmutation {mut} ({cs.MUTATIONS[mut]}): moves {len(moved)} inputs of '{fam}', first {moved[:6]}")
    assert moved, f"mutation {mut} ({cs.MUTATIONS[mut]}) moves no input of family '{fam}' (cell: {cell})"
    named = {"a": "t16k_lane5_match", "b": "t16k_lane5_nomatch", "f": "hit_at_limit", "g": "insert", "h": "t16k_lane8_third",
             "i": "copy_L65_D4", "j": "copy_L8_D2048", "J": "copy_L12_D4", "k": "lit61_c0_m0"}
    if mut in named:
        assert named[mut] in moved, f"mutation {mut}: {named[mut]} (cell: {cell}) does not move"
