"""rr_rdbload_batch where it parses bytes the project did not write, and at the kernels' own seams
(redrock_old_amd/csrc/rr_rdbload.hip), against tests/rdbload_reference.py: every status, offset,
blob byte and total, canaries behind every buffer (run_device / compare / check of
tests/test_gpu_rdbload.py).  Every rejection is made by rdbload_size_kernel and rdbload_emit_kernel
repeats the walk unchecked, so a wrong status is also a wrong write.

  1 the mutation corpus (tests/rdbload_mutants.py), forwards, reversed, and through the host entry
  2 a truncated value with the bytes it is missing directly behind it: nothing outside a slice is read
  3 input offsets that decrease or reach past data_cap: RR_RDBLOAD_E_TRUNC, the neighbours untouched
  4 LZF sequences at every stream offset round the 64-byte reload of lzf_check / LzfIt::next
  5 ziplist entries at every node offset round walk_node's reload
  6 the LDS window at RR_RDBLOAD_LZF_NODE_MAX, and lzf_to_window's cut below a sequence's end
"""
import struct

import numpy as np
import pytest
import torch

import lzf_reference as lzf
import rdb_reference as ref
import rdbload_mutants as mu
import rdbload_reference as ld
from test_gpu_rdbload import check, compare, lits, lzf_str, match, node_of, run_device
from test_rdbload import HZL, ISET, L, S, SET, ZERO, ZZL, intset_of, zl_of

pytestmark = pytest.mark.gpu

KEEP = ld.options(set_max_intset_entries=512, hash_max_ziplist_entries=512, zset_max_ziplist_entries=128)


def raw(b):
    return ref.save_len(len(b)) + b


def lz(b):
    """b as an LZF string: the CPU compressor's stream, literal runs where it does not compress."""
    return lzf_str(lzf.compress(b, len(b) - 4) or lits(b), len(b))


def lst(nodes):
    """A List payload of node strings (each already in its raw or LZF form)."""
    return ref.save_len(len(nodes)) + b"".join(nodes)


def word(rng, k):
    return bytes(rng.integers(97, 123, k, dtype=np.uint8))


# ---- 1. the mutation corpus ---------------------------------------------------------------------------
def test_mutation_sweep(engine):
    types, pays, _ = mu.corpus()
    assert len(types) >= 10000
    fwd, _ = check(engine, types, pays, mu.OPTS)
    assert set(fwd.tolist()) == {0, 32, 33, 34, 35, 36, 37, 38}
    # reversed: other neighbours, another wave and workgroup, another 16-byte alignment of every body
    rev, _ = check(engine, types[::-1], pays[::-1], mu.OPTS)
    assert rev.tolist() == fwd.tolist()[::-1]
    st, _ = check(engine, types[:2000], pays[:2000], mu.OPTS, host=True)
    assert st.tolist() == fwd.tolist()[:2000]


# ---- 2. the missing bytes lie directly behind the value -----------------------------------------------
def split_bait():
    types, pays = [], []
    for t, p in mu.seeds():
        for k in range(1, len(p)):
            types += [t, t]
            pays += [p[:k], p[k:]]                          # contiguous in data, as the intact seed would be
    return types, pays


def test_split_bait(engine):
    types, pays = split_bait()
    st, _ = check(engine, types, pays, mu.OPTS)
    heads = st[0::2]
    assert len(heads) >= 500 and (heads == ld.E_TRUNC).all()


# ---- 3. the input offsets -----------------------------------------------------------------------------
def offsets_batch():
    """About 20 valid values of every type; statuses 0 and CONVERT under mu.OPTS."""
    types = [t for t, _ in mu.seeds()] + [S, S]
    pays = [p for _, p in mu.seeds()] + [raw(b"last but one"), raw(b"the last value")]
    return types, pays


def offsets_variants(offsets, in_cap):
    """(name, offsets, data_cap of the call)."""
    n = len(offsets) - 1
    i = n // 2
    out = []
    o = offsets.copy(); o[i + 1] = o[i] - 3
    out.append(("decreasing", o, in_cap))
    o = offsets.copy(); o[n] = in_cap + 1
    out.append(("end+1", o, in_cap))
    o = offsets.copy(); o[n] = in_cap + 4000
    out.append(("end+4000", o, in_cap))
    o = offsets.copy(); o[i] = 2**40
    out.append(("2^40", o, in_cap))
    out.append(("cap inside a value", offsets.copy(), (int(offsets[i]) + int(offsets[i + 1])) // 2))
    return out


def test_offsets_guard(engine):
    types, pays = offsets_batch()
    data, offsets = ld.pack(pays)
    n, in_cap = len(types), len(data)
    base = ld.load_batch(types, data, offsets, mu.OPTS)[2]
    assert set(base.tolist()) == {0, ld.E_CONVERT}
    # the call's data is a slice of a longer tensor: what lies behind data_cap is mapped, and holds the
    # batch once more, so a slice that reached past data_cap would find bytes that parse
    big = torch.from_numpy(np.concatenate([data, data, data, np.zeros(8192, np.uint8)])).cuda()
    for name, offs, cap_in in offsets_variants(offsets, in_cap):
        want = ld.load_batch(types, data[:cap_in], offs, mu.OPTS)
        total = int(want[1][-1])
        room = total + 40 + 64
        _, bufs = run_device(engine, types, data, offs, mu.OPTS, total + 40, room, d_data=big[:cap_in])
        torch.cuda.synchronize()
        try:
            compare(bufs, n, want, room)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        st = want[2]
        i = n // 2
        if name == "decreasing":
            assert st[i] == ld.E_TRUNC and np.array_equal(st[:i], base[:i]) and np.array_equal(st[i + 2:], base[i + 2:])
        elif name.startswith("end+"):
            assert st[n - 1] == ld.E_TRUNC and np.array_equal(st[:n - 1], base[:n - 1])
        elif name == "2^40":
            assert st[i - 1] == st[i] == ld.E_TRUNC
            assert np.array_equal(st[:i - 1], base[:i - 1]) and np.array_equal(st[i + 1:], base[i + 1:])
        else:
            assert (st[i:] == ld.E_TRUNC).all() and np.array_equal(st[:i], base[:i])
        assert want[3]["n_bad"] == int((st != 0).sum()) and (st == 0).any()


# ---- 4. LZF sequences round the 64-byte reload --------------------------------------------------------
SEAM = range(56, 71)          # stream offsets of the sequence's control byte; the reload is at 62


def lit_pad(b, k):
    """b as k literal runs of nearly equal length: len(b) + k stream bytes."""
    q, r = divmod(len(b), k)
    out, at = b"", 0
    for j in range(k):
        ln = q + (1 if j < r else 0)
        assert 1 <= ln <= 32
        out += bytes([ln - 1]) + b[at:at + ln]
        at += ln
    return out


def pad_to(rng, x):
    """Literal runs that fill exactly x stream bytes, every control byte below offset 62 (no reload
    before x): (stream, the literals)."""
    k = 2 if x - 2 <= 64 else 3
    b = word(rng, x - k)
    s = lit_pad(b, k)
    assert len(s) == x
    return s, b


def seam_streams():
    """[(stream, its output, corrupt sibling)] per offset and form."""
    rng = np.random.default_rng(11)
    out = []
    for x in SEAM:
        pad, b = pad_to(rng, x)
        n = len(b)
        follow = match(4, 9) + lits(b"tail!")               # read from the reloaded register
        forms = [(match(20, 7), match(20, n + 1)),          # the long form: 3 stream bytes
                 (match(5, 30), match(5, n + 1)),           # the short form: 2
                 (match(264, n), match(264, n + 1)),        # the longest, at the largest valid distance
                 (lits(word(rng, 32)) + match(9, 3), lits(word(rng, 32)) + match(9, n + 33))]   # a literal run's control byte
        for good, bad in forms:
            s = pad + good + follow
            text = lzf.decompress(s, 1 << 20)
            assert text is not None and len(text) > 20
            sb = pad + bad + follow
            assert lzf.decompress(sb, 1 << 20) is None
            out.append((s, text, sb))
    return out


def sequences(stream):
    """[(stream offset of the control byte, stream bytes, match length or 0)] of a valid stream."""
    out, ip = [], 0
    while ip < len(stream):
        c = stream[ip]
        if c < 32:
            out.append((ip, 2 + c, 0)); ip += 2 + c
        elif c >> 5 == 7:
            out.append((ip, 3, 9 + stream[ip + 1])); ip += 3
        else:
            out.append((ip, 2, (c >> 5) + 2)); ip += 2
    return out


def seam_nodes():
    """List nodes whose compressed form (the CPU compressor's) has a long-form match at a stream
    offset in SEAM, found by a search over the first entry's length: {offset: node}."""
    rng = np.random.default_rng(12)
    found = {}
    text = word(rng, 90)
    for a in range(20, 90):
        for rep in (b"z" * 40, b"xy" * 30):
            node = node_of([bytes([a]) + text[:a] if a < 64 else bytes([0x40, a]) + text[:a], bytes([len(rep)]) + rep, b"\xF5"])
            comp = lzf.compress(node, len(node) - 4)
            if comp is None:
                continue
            for at, nb, ml in sequences(comp):
                if nb == 3 and ml and at in SEAM:
                    found.setdefault(at, node)
    return found


def hand_node(rng, x):
    """A valid node and a hand-written stream of it with a long-form match at stream offset x:
    (node, stream, corrupt stream)."""
    k = 2 if x - 2 <= 64 else 3
    n = x - k                                                # literal bytes in front of the match
    a = n - 10 - 2 - 2 - 1                                   # header, entry 1's two bytes, entry 2's two, one 'z'
    node = node_of([bytes([a]) + word(rng, a), bytes([40]) + b"z" * 40, b"\xF5"])
    s = lit_pad(node[:n], k) + match(39, 1) + lits(node[n + 39:])
    assert lzf.decompress(s, len(node)) == node and s[x] == 0xE0
    bad = lit_pad(node[:n], k) + match(39, n + 1) + lits(node[n + 39:])
    return node, s, bad


def lzf_seam_cases():
    rng = np.random.default_rng(13)
    types, pays, want = [], [], []
    streams = seam_streams()
    for s, text, sb in streams:                              # a String of more than 20 bytes: lzf_to_global
        types += [S, S]; pays += [lzf_str(s, len(text)), lzf_str(sb, len(text))]; want += [0, ld.E_LZF]
    for k in range(0, len(streams), 4):                      # Set members, four a Set
        grp = streams[k:k + 4]
        types.append(SET); pays.append(ref.save_len(len(grp)) + b"".join(lzf_str(s, len(t)) for s, t, _ in grp)); want.append(0)
        types.append(SET); want.append(ld.E_LZF)
        pays.append(ref.save_len(len(grp)) + b"".join(lzf_str(sb if j == len(grp) - 1 else s, len(t)) for j, (s, t, sb) in enumerate(grp)))
    for x in SEAM:                                           # a List node through lzf_to_window and walk_node on LDS
        node, s, bad = hand_node(rng, x)
        types += [L, L]; want += [0, ld.E_LZF]
        pays += [lst([raw(zl_of(1)), lzf_str(s, len(node))]), lst([raw(zl_of(1)), lzf_str(bad, len(node))])]
    found = seam_nodes()
    for at in sorted(found):
        types.append(L); pays.append(lst([lz(found[at])])); want.append(0)
    return types, pays, want, found


def test_lzf_reload_seams(engine):
    types, pays, want, found = lzf_seam_cases()
    assert len(found) >= 8, sorted(found)                    # of the 15 offsets, by the CPU compressor
    st, tot = check(engine, types, pays, ZERO, host=True)
    assert st.tolist() == want


# ---- 5. ziplist entries round walk_node's reload ------------------------------------------------------
ZL_SEAM = range(44, 67)       # node offsets of the entry; the first reload is at 51 or 52


def seam_node(t, form, rng):
    """(entries, index of the entry at node offset t)."""
    pad = t - 10
    ents = []
    if pad % 2:
        ents.append(b"\xFE\x85")                             # a three-byte entry for parity
        pad -= 3
    ents += [bytes([0xF1 + k % 13]) for k in range(pad // 2)]   # two bytes each
    at = len(ents)
    if form == "int64":
        ents.append(b"\xE0" + struct.pack("<q", int(rng.integers(-2**63, 2**63 - 1))))   # 10 bytes with its prevlen
    elif form == "str32":
        ents.append(b"\x80" + struct.pack(">I", 3) + word(rng, 3))                       # 6-byte header, 3-byte body
    else:
        ents.append(bytes([0x40, 5]) + word(rng, 5))
    ents += [b"\xF3", b"\xFC"]
    return ents, at


def entry_offset(ents, at):
    """Node offsets (start, end) of entry `at` of node_of(ents) (every prevlen here is one byte)."""
    p = 10
    for e in ents[:at]:
        p += 1 + len(e)
    return p, p + 1 + len(ents[at])


def ziplist_seam_cases():
    rng = np.random.default_rng(14)
    types, pays, want = [], [], []

    def add(node, st):
        for form in (raw, lz):
            types.append(L); pays.append(lst([form(node)])); want.append(st)

    for t in ZL_SEAM:
        for form in ("int64", "str32", "str14"):
            ents, at = seam_node(t, form, rng)
            node = node_of(ents)
            p, end = entry_offset(ents, at)
            assert p == t and ld.walk_node(node) is not None
            add(node, 0)
            z = bytearray(node); z[p] += 1                   # the entry's prevlen off by one
            add(bytes(z), ld.E_ZIPLIST)
            z = bytearray(node); z[p + 1] = 0xC1             # no such encoding
            add(bytes(z), ld.E_ZIPLIST)
            # the node cut so that the entry's body ends one byte past L - 1: zlbytes, zltail and zllen
            # say so too, the body's end is the only defect
            cut = struct.pack("<IIH", end, p, at + 1) + node[10:end]
            assert len(cut) == end
            add(cut, ld.E_ZIPLIST)
    big = node_of([bytes([0x41, 0x2C]) + word(rng, 300), b"\xE0" + struct.pack("<q", -2**62 - 12345), b"\xF7"])
    add(big, 0)                                              # a 5-byte prevlen: a 14-byte header
    return types, pays, want


def test_ziplist_reload_seams(engine):
    types, pays, want = ziplist_seam_cases()
    st, tot = check(engine, types, pays, host=True)
    assert st.tolist() == want and tot["n_elems"] > 1000


# ---- 6. the window's limits ---------------------------------------------------------------------------
def sized_node(total, salt):
    """A node of exactly `total` bytes: entries of 60 repeated letters, the last one sized to fit."""
    n = (total - 11) // 62 - 1
    rest = total - 11 - 62 * n
    if rest == 66:                                           # 1 + 1 + 63 = 65 and 1 + 2 + 64 = 67: no entry of 66
        n, rest = n - 1, rest + 62
    body = rest - 2 if rest - 2 <= 63 else rest - 3
    ents = [bytes([60]) + bytes([97 + (k + salt) % 26]) * 60 for k in range(n)]
    ents.append((bytes([body]) if body <= 63 else bytes([0x40 | body >> 8, body & 0xFF])) + bytes([65 + salt % 26]) * body)
    node = node_of(ents)
    assert len(node) == total and ld.walk_node(node) is not None
    return node


def window_cases():
    """[(types, payloads, options, statuses)], a call each."""
    calls = []
    M = ld.LZF_NODE_MAX
    nodes = [sized_node(M + d, d + 1) for d in (-1, 0, 1)]
    calls.append(([L] * 6, [lst([lz(z)]) for z in nodes] + [lst([raw(z)]) for z in nodes], None,
                  [0, 0, ld.E_CONVERT, 0, 0, 0]))
    # four full windows in a workgroup, each node different, and again in another order in the next
    four = [sized_node(M, 3 + k) for k in range(4)]
    assert len(set(four)) == 4
    order = four + four[3:] + four[:3]
    calls.append(([L] * 8, [lst([lz(z)]) for z in order], None, [0] * 8))
    # lzf_to_window's cut: a String's first 20 bytes
    ty, pa, st = [], [], []
    for n in range(1, 22):                                   # '1' * n: enc INT up to 19, text at 20 and 21
        s = lits(b"1" * n) if n < 4 else lits(b"1") + match(n - 1, 1)
        assert lzf.decompress(s, n) == b"1" * n
        ty.append(S); pa.append(lzf_str(s, n)); st.append(0)
    neg = lits(b"-1") + match(18, 1)
    assert lzf.decompress(neg, 20) == b"-" + b"1" * 19
    ty.append(S); pa.append(lzf_str(neg, 20)); st.append(0)
    calls.append((ty, pa, None, st))
    # the same strings as Set members: all integers up to 19 digits (CONVERT where n fits), not with 20
    mem19, mem20 = pa[:19], pa[:20]
    for members in (mem19, mem20):
        p = ref.save_len(len(members)) + b"".join(members)
        calls.append(([SET], [p], KEEP, [ld.E_CONVERT if members is mem19 else 0]))
        calls.append(([SET], [p], ZERO, [0]))
    # a ziplist header (10 bytes) whose last byte is the first of a back reference
    z1 = zl_of(1)
    s1 = lits(z1[:9]) + match(3, 3) + lits(b"a\xff")
    assert lzf.decompress(s1, len(z1)) == z1
    z2 = node_of([b"\x00", b"\x00"])                         # two empty strings: zllen 2
    s2 = lits(z2[:9]) + match(3, 4) + lits(z2[12:])
    assert lzf.decompress(s2, len(z2)) == z2
    z3 = struct.pack("<IIH", 257, 10, 257) + b"\x00\x40\xF3" + b"q" * 243 + b"\xff"   # zllen 257: both its bytes come from the match
    s3 = lits(z3[:8]) + match(3, 8) + lits(z3[11:])
    assert lzf.decompress(s3, len(z3)) == z3
    zls = [lzf_str(s1, len(z1)), lzf_str(s2, len(z2)), lzf_str(s3, len(z3))]
    one = ld.options(hash_max_ziplist_entries=1, zset_max_ziplist_entries=1)
    calls.append(([HZL, ZZL] * 3, [p for p in zls for _ in (0, 1)], KEEP, [0] * 6))
    calls.append(([HZL, ZZL] * 3, [p for p in zls for _ in (0, 1)], one, [0, 0, 0, 0, ld.E_CONVERT, ld.E_CONVERT]))
    calls.append(([HZL, ZZL] * 3, [p for p in zls for _ in (0, 1)], ZERO, [0, 0] + [ld.E_CONVERT] * 4))
    # an intset whose eight header bytes end inside a literal run of 32
    iset = intset_of(4, [3, -70000, 5, 2**31 - 1, 9, 10, 11, 12, 13, 14])
    si = lits(iset)
    assert si[0] == 31
    two = ld.options(set_max_intset_entries=2)
    calls.append(([ISET, ISET], [lzf_str(si, len(iset))] * 2, KEEP, [0, 0]))
    calls.append(([ISET, ISET], [lzf_str(si, len(iset))] * 2, two, [ld.E_CONVERT] * 2))
    return calls


def test_window_limits(engine):
    for types, pays, opts, want in window_cases():
        st, _ = check(engine, types, pays, opts, host=True)
        assert st.tolist() == want, (types, want)
