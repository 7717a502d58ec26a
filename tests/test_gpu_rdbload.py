"""rr_rdbload_batch on the GPU against tests/rdbload_reference.py: every status, offset, blob byte
and total, with a canary behind every buffer the call writes.  The batches are the smallest that
reach the kernels' paths: the header forms, the LZF sequences at their limits, the copy paths at
every source alignment, the ziplist entry classes of a List node, one stride of the grid.

Corrupt input and the kernels' own seams are in tests/test_gpu_rdbload_edges.py (it imports
run_device / compare / check from here): the mutation corpus of tests/rdbload_mutants.py (checked on
the CPU by tests/test_rdbload_mutants.py) in two orders, truncated values with their missing bytes
directly behind them, bad input offsets, LZF sequences and ziplist entries at every position round
the 64-byte reloads, and the LDS window at its limits."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import lzf_reference as lzf
import rdb_reference as ref
import rdbload_reference as ld
from helpers import batch_from_blobs, golden
from test_rdbload import HASH, HZL, ISET, L, S, SET, ZERO, ZSET, ZZL, intset_of, literal_cases, zl_of

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GRID_STRIDE = 16384 * 4          # the size / emit grid's cap: workgroups * waves (rr_rdbload.hip)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def run_device(engine, types, data, offsets, opts, cap, room, stream=None, d_data=None):
    """d_data: the payload bytes already on the device (tests/test_gpu_rdbload_edges.py passes a slice
    of a longer tensor, so that the call's data_cap is not the allocation's end)."""
    n = len(types)
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4 + 2,), -3, dtype=torch.int64, device="cuda")
    if d_data is None:
        d_data = _dev(data) if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_in_off = torch.from_numpy(np.ascontiguousarray(offsets, np.uint64).view(np.int64).copy()).cuda()
    d_types = _dev(np.asarray(types, np.uint8)) if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
    args = (d_data, d_in_off, d_types, out[:cap], d_off[:n + 1], d_status[:n], d_tot[:4])
    engine.rdbload(*args, opts=ld.c_opts(opts) if opts else None, stream=stream)
    return args, (out, d_off, d_status, d_tot)


def compare(bufs, n, want, room):
    out, d_off, d_status, d_tot = bufs
    data, offsets, status, totals, blobs = want
    got_off = d_off.cpu().numpy()
    assert np.array_equal(got_off[:n + 1].view(np.uint64), offsets) and (got_off[n + 1:] == 7).all()
    st = d_status.cpu().numpy()
    if not np.array_equal(st[:n], status):
        i = int(np.nonzero(st[:n] != status)[0][0])
        raise AssertionError(f"status of value {i}: got {st[i]}, want {status[i]}")
    assert (st[n:] == CANARY).all()
    t = d_tot.cpu().numpy()
    assert (t[4:] == -3).all()
    t = t.view(np.uint64)
    assert {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])} == totals
    exp = np.full(room, CANARY, np.uint8)
    for i, b in enumerate(blobs):
        if status[i] == 0:
            o = int(offsets[i])
            exp[o:o + len(b)] = np.frombuffer(b, np.uint8)
    got = out.cpu().numpy()
    if not np.array_equal(got, exp):
        at = int(np.nonzero(got != exp)[0][0])
        i = int(np.searchsorted(offsets, at, side="right")) - 1
        raise AssertionError(f"byte {at} (value {i}, offset {at - int(offsets[min(i, n)])}): got {got[at]:#x}, want {exp[at]:#x}")


def check(engine, types, payloads, opts=None, data_cap=None, host=False):
    """The device call on canary-filled buffers against the reference; host: the host entry too."""
    data, offsets = ld.pack(payloads)
    n = len(types)
    want = ld.load_batch(types, data, offsets, opts, data_cap)
    total = int(want[1][-1])
    cap = total + 40 if data_cap is None else data_cap
    room = max(cap, total) + 64
    _, bufs = run_device(engine, types, data, offsets, opts, cap, room)
    torch.cuda.synchronize()
    compare(bufs, n, want, room)
    if host:
        hd, ho, hs, ht = engine.rdbload_host(data, offsets, np.asarray(types, np.uint8), ld.c_opts(opts) if opts else None, data_cap)
        assert np.array_equal(ho, want[1]) and np.array_equal(hs, want[2]) and ht == want[3]
        if data_cap is None:
            assert np.array_equal(hd, want[0])
    return want[2], want[3]


# ---- 1. every literal of the CPU file, one call per option set, both entries ----------------------
def test_literals(engine):
    groups = {}
    for t, p, o, st, blob in literal_cases():
        groups.setdefault(tuple(sorted((o or ld.DEFAULTS).items())), []).append((t, p, st))
    seen = set()
    for key, cases in groups.items():
        st, _ = check(engine, [c[0] for c in cases], [c[1] for c in cases], dict(key), host=True)
        assert st.tolist() == [c[2] for c in cases]
        seen |= set(st.tolist())
    assert seen == {0, 32, 33, 34, 35, 36, 37, 38}


# ---- 2. round trip over the golden fixtures -----------------------------------------------------------
def models(values, elems, arena):
    ab = arena.tobytes()
    out = []
    for (val, descs), _ in zip(ref.flat_values(values, elems, arena), values):
        if val["status"] != 0 or not ref.accepted_value(val, descs, len(arena)):
            out.append(None)
        else:
            out.append(ref.model(val, descs[:1] if val["type"] in (HZL, ZZL) else descs, ab))
    return out


@pytest.mark.parametrize("lzf_flag", [False, True])
def test_roundtrip_golden(engine, lzf_flag):
    g = golden()
    blobs = [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]
    data, offs = batch_from_blobs(blobs)
    v1, e1, a1, _ = engine.decode_host(data, offs)
    first = models(v1, e1, a1)
    types, pdata, poffs, pst, _ = engine.rdbsave_host(v1, e1, a1, lzf=lzf_flag)
    # the fixtures' largest compact values: 32767 entries never convert (a ziplist with zllen 0xFFFF
    # would; the fixtures hold none that decodes).  (a) the compact kinds, (b) the hash-table kinds
    big = ld.options(set_max_intset_entries=32767, hash_max_ziplist_entries=32767, zset_max_ziplist_entries=32767)
    kinds_a, kinds_b = (S, L, ISET, HZL, ZZL), (SET, HASH, ZSET)
    n_checked = 0
    for opts, kinds in ((big, kinds_a), (ZERO, kinds_b)):
        sel = [i for i in range(len(types)) if pst[i] == 0 and types[i] in kinds and
               not (types[i] in kinds_b and int(v1["n_elems"][i]) == 0)]
        pays = [bytes(pdata[int(poffs[i]):int(poffs[i + 1])]) for i in sel]
        ty = [int(types[i]) for i in sel]
        for t, p in zip(ty, pays):                           # the restatement first, on the CPU
            assert ld.load_blob(t, p, opts)[0] == 0
        st, _ = check(engine, ty, pays, opts, host=True)
        assert (st == 0).all()
        bdata, boffs, bst, _ = engine.rdbload_host(*ld.pack(pays), np.asarray(ty, np.uint8), ld.c_opts(opts))
        pad = np.zeros((len(bdata) + 15) & ~15, np.uint8)
        pad[:len(bdata)] = bdata
        second = models(*engine.decode_host(pad, boffs)[:3])
        assert second == [first[i] for i in sel] and None not in second
        n_checked += len(sel)
    assert n_checked >= 20


# ---- 3. LZF edges ------------------------------------------------------------------------------------
def lzf_str(stream, ulen):
    return b"\xC3" + ref.save_len(len(stream)) + ref.save_len(ulen) + stream


def match(ml, off):
    l, o = ml - 2, off - 1
    return bytes([(l << 5) | (o >> 8), o & 0xFF]) if l < 7 else bytes([0xE0 | (o >> 8), l - 7, o & 0xFF])


def lits(b):
    return b"".join(bytes([len(b[k:k + 32]) - 1]) + b[k:k + 32] for k in range(0, len(b), 32))


def test_lzf_edges(engine):
    rng = np.random.default_rng(5)
    word = lambda k: bytes(rng.integers(97, 123, k, dtype=np.uint8))
    cases = []
    add = lambda stream, ulen: cases.append(lzf_str(stream, ulen))
    w32 = word(32)
    add(lits(w32), 32)                                         # a literal run of 32
    add(lits(w32) + match(3, 5), 35)                           # a match of 3
    add(lits(w32) + match(264, 32), 296)                       # of 264: the long form, and overlapping (period 32)
    add(lits(b"q") + match(100, 1), 101)                       # distance 1: a run
    far = word(8192)
    add(lits(far) + match(40, 8192), 8232)                     # distance 8192
    add(lits(far) + match(40, 8192) + match(9, 3) + lits(b"xyz"), 8244)
    s21 = b"abcabcabcabcabcabcabc"
    add(lzf.compress(s21, 17), 21)                             # a 21-byte string by the CPU compressor
    big = (word(700) * 100)[:70000]
    add(lzf.compress(big, len(big) - 4), 70000)                # a 70,000-byte string
    add(lzf.compress(bytes(70000), 69996), 70000)
    add(match(3, 1) + lits(b"abc"), 6)                         # a back reference one byte before the start
    add(lits(b"ab") + match(3, 3), 5)                          # and one byte before it, after two literals
    ok = lits(w32) + match(10, 7)
    add(ok[:-1], 42)                                           # a stream one byte short
    add(ok + b"\x00", 42)                                      # and one byte long (a literal run without its byte)
    add(ok, 43)                                                # a declared len one more than the stream yields
    add(ok, 41)                                                # and one less
    add(b"", 0)                                                # an empty stream
    add(lits(b"12345"), 5)                                     # LZF text that tryObjectEncoding turns into an integer
    want_bad = [0] * 9 + [ld.E_LZF] * 7 + [0]
    st, _ = check(engine, [S] * len(cases), cases, host=True)
    assert st.tolist() == want_bad
    # the same strings as Set members, Hash values, and an LZF intset blob, ziplist and List node
    members = [c for c, b in zip(cases, want_bad) if b == 0]
    pays = [ref.save_len(len(members)) + b"".join(members),
            ref.save_len(len(members)) + b"".join(b"\x01k" + m for m in members)]
    iset = intset_of(8, list(range(100, 140)))
    zl = zl_of(20)
    nodes = ref.list_nodes([b"e%d" % k for k in range(300)] + [b"17", word(300)], -2)
    lz = lambda b: lzf_str(lzf.compress(b, len(b) - 4) or lits(b), len(b))   # (literal runs where it does not compress)
    pays += [lz(iset), lz(zl), lz(zl), ref.save_len(len(nodes) + 1) + b"".join(lz(z) for z in nodes) + b"\x0B" + zl_of(0)]
    st, tot = check(engine, [SET, HASH, ISET, HZL, ZZL, L], pays, ZERO | {"set_max_intset_entries": 512,
                    "hash_max_ziplist_entries": 512, "zset_max_ziplist_entries": 128}, host=True)
    assert st.tolist() == [0, 0, 0, 0, 0, 0] and tot["n_elems"] > 300
    # an LZF node above the window is the CPU path's; a corrupt LZF node is E_ZIPLIST
    ents = [bytes([97 + k % 26]) * 60 for k in range(200)]
    bignode = ref.list_nodes(ents, -5)[0]
    bad = bytearray(nodes[0]); bad[4] ^= 1                     # a wrong zltail
    st, _ = check(engine, [L, L, L], [b"\x01" + lz(bignode), b"\x01" + ref.save_len(len(bignode)) + bignode, b"\x01" + lz(bytes(bad))])
    assert st.tolist() == [ld.E_CONVERT, 0, ld.E_ZIPLIST]


# ---- 4. copy paths: body lengths at every source alignment --------------------------------------------
def test_copy_paths(engine):
    rng = np.random.default_rng(6)
    types, pays = [], []
    at = 0
    for ln in (0, 1, 31, 32, 33, 63, 64, 65, 1040):
        for a in range(16):
            hdr = ref.save_len(ln)
            while (at + len(hdr)) % 16 != a:                   # one-byte filler values shift the next body
                types.append(S); pays.append(b"\x00"); at += 1
            body = bytes(rng.integers(97, 123, ln, dtype=np.uint8))
            types.append(S); pays.append(hdr + body); at += len(hdr) + ln
    # the same bodies as members (8-byte length in front: other destination alignments) and List entries
    bodies = [bytes(rng.integers(97, 123, ln, dtype=np.uint8)) for ln in (0, 1, 31, 32, 33, 63, 64, 65, 1040) for _ in range(3)]
    types.append(SET); pays.append(ref.save_len(len(bodies)) + b"".join(ref.save_len(len(b)) + b for b in bodies))
    nodes = ref.list_nodes(bodies, -2)
    types.append(L); pays.append(ref.save_len(len(nodes)) + b"".join(ref.save_len(len(z)) + z for z in nodes))
    st, _ = check(engine, types, pays, ZERO, host=True)
    assert (st == 0).all()


# ---- 5. List nodes -----------------------------------------------------------------------------------
def node_of(entries):
    """A ziplist from raw (encoding + body) entries, the prevlen chain computed."""
    body, prev, tail = b"", 0, 10
    for e in entries:
        tail = 10 + len(body)
        ent = (bytes([prev]) if prev < 254 else b"\xFE" + struct.pack("<I", prev)) + e
        body += ent
        prev = len(ent)
    return struct.pack("<IIH", 11 + len(body), tail, len(entries)) + body + b"\xFF"


def test_list_nodes(engine):
    rng = np.random.default_rng(7)
    word = lambda k: bytes(rng.integers(97, 123, k, dtype=np.uint8))
    ints = [bytes([0xF1 + k]) for k in range(13)]                                    # 0..12
    for enc, w, vals in ((0xFE, 1, (-128, -1, 13, 127)), (0xC0, 2, (-32768, -129, 128, 32767)),
                         (0xF0, 3, (-2**23, -32769, 32768, 2**23 - 1)), (0xD0, 4, (-2**31, -2**23 - 1, 2**23, 2**31 - 1)),
                         (0xE0, 8, (-2**63, -2**31 - 1, 2**31, 2**63 - 1))):
        ints += [bytes([enc]) + int(v).to_bytes(w, "little", signed=True) for v in vals]
    strs = [bytes([5]) + b"hello", bytes([0]), bytes([0x40 | (300 >> 8), 300 & 0xFF]) + word(300),
            b"\x80" + struct.pack(">I", 17000) + word(17000), bytes([3]) + b"end"]  # the entry after 17000 bytes: a 5-byte prevlen
    good = [node_of(ints), node_of(strs), node_of([]), node_of(ints + strs + ints)]
    lst = lambda nodes: ref.save_len(len(nodes)) + b"".join(ref.save_len(len(z)) + z for z in nodes)
    pays = [lst(good), lst([node_of([bytes([1]) + b"x"])] * 65)]                     # 65 nodes: the two-byte count
    want = [0, 0]
    base = node_of([bytes([2]) + b"ab", bytes([2]) + b"cd", bytes([0xF3])])
    for mutate in ("prevlen", "zltail", "end", "zllen", "zlbytes", "enc"):
        z = bytearray(base)
        if mutate == "prevlen": z[14] ^= 1                     # the second entry's prevlen
        if mutate == "zltail": z[4] += 1
        if mutate == "end": z[-1] = 0x00
        if mutate == "zllen": z[8] += 1
        if mutate == "zlbytes": z[0] += 1
        if mutate == "enc": z[-2] = 0xFF                       # the last entry's encoding: an early end byte
        pays.append(lst([good[0], bytes(z)]))
        want.append(ld.E_ZIPLIST)
    pays.append(lst([base[:-1]]))                              # the end byte missing
    want.append(ld.E_ZIPLIST)
    st, tot = check(engine, [L] * len(pays), pays, host=True)
    assert st.tolist() == want and tot["n_elems"] > 100


# ---- 6. grid and capacity -----------------------------------------------------------------------------
def tiling_base():
    """61 short values of every type and a few statuses, tiled the way flat_forge.tile_records tiles."""
    iset, zl = intset_of(2, [3, 4]), zl_of(2)
    base = [(S, b"\x03abc"), (S, b"\xC0\x07"), (SET, b"\x02\x01a\x01b"), (HASH, b"\x01\x01f\x01v"),
            (ZSET, b"\x01\x01m" + struct.pack("<d", 2.5)), (ISET, bytes([len(iset)]) + iset), (HZL, bytes([len(zl)]) + zl),
            (ZZL, bytes([len(zl)]) + zl), (L, b"\x01" + bytes([len(zl)]) + zl), (S, b"\x05ab"), (7, b"\x00"),
            (S, lzf_str(b"\x00a" + match(9, 1), 10)), (SET, b"\x01\x011")]
    cases = [base[k % len(base)] for k in range(61)]
    return [c[0] for c in cases], [c[1] for c in cases]


def tiled_expect(types, pays, n, opts, data_cap=None):
    """load_batch of the base, its results repeated (tests/test_rdbload.py checks load_batch itself)."""
    m = len(types)
    b = ld.load_batch(types, *ld.pack(pays), opts)
    reps = -(-n // m)
    sizes = np.tile(np.diff(b[1].astype(np.int64)), reps)[:n]
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(sizes, out=offs[1:])
    status = np.tile(b[2], reps)[:n].copy()
    blobs = (b[4] * reps)[:n]
    cap = int(offs[-1]) if data_cap is None else data_cap
    fits = offs[1:] <= cap
    status[(status == 0) & ~fits] = ld.E_CAPACITY
    per = [ld.load_blob(t, p, opts) for t, p in zip(types, pays)]
    pay = sum(per[i % m][2] for i in range(n) if status[i] == 0)
    nel = sum(per[i % m][3] for i in range(n) if status[i] == 0)
    totals = {"n_elems": nel, "bytes": int(offs[-1]), "n_bad": int((status != 0).sum()), "payload": pay}
    return None, offs, status, totals, blobs


def test_grid_stride_plus_61(engine):
    types, pays = tiling_base()
    n = GRID_STRIDE + 61
    m = len(types)
    reps = -(-n // m)
    lens = np.tile([len(p) for p in pays], reps)[:n]
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer((b"".join(pays) * reps)[:int(offsets[-1])], np.uint8)
    tt = np.tile(np.asarray(types, np.uint8), reps)[:n]
    want = tiled_expect(types, pays, n, ZERO)
    total = int(want[1][-1])
    _, bufs = run_device(engine, tt, data, offsets, ZERO, total, total + 64)
    torch.cuda.synchronize()
    compare(bufs, n, want, total + 64)
    assert (want[2][GRID_STRIDE:] == 0).any() and (want[2][GRID_STRIDE:] != 0).any()   # both kinds past the stride


def test_capacity_and_empty(engine):
    types, pays = tiling_base()
    offs = ld.load_batch(types, *ld.pack(pays), ZERO)[1]
    n = len(types)
    ok = [i for i in range(n) if offs[i + 1] > offs[i]]
    for i in (ok[0], ok[len(ok) // 2], ok[-1]):
        cut = (int(offs[i]) + int(offs[i + 1])) // 2          # inside value i
        st, _ = check(engine, types, pays, ZERO, data_cap=cut, host=True)
        assert st[i] == ld.E_CAPACITY and (st[:i] != ld.E_CAPACITY).all()
    st, _ = check(engine, types, pays, ZERO, data_cap=int(offs[-1]))   # exactly offsets[n]
    assert (st != ld.E_CAPACITY).all()
    check(engine, types, pays, ZERO, data_cap=0, host=True)            # sizes only
    check(engine, [], [], ZERO, host=True)                             # n == 0


def test_side_stream_graph_replayed_twice(engine):
    types, pays = tiling_base()
    data, offsets = ld.pack(pays)
    n = len(types)
    want = ld.load_batch(types, data, offsets, ZERO)
    total = int(want[1][-1])
    engine.reserve(n, len(data))
    side = torch.cuda.Stream()
    args, bufs = run_device(engine, types, data, offsets, ZERO, total, total + 64, stream=side)   # a warm call
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        engine.rdbload(*args, opts=ld.c_opts(ZERO), stream=torch.cuda.current_stream())
    for _ in range(2):
        bufs[0].fill_(CANARY)
        bufs[2][:n].fill_(CANARY)
        bufs[3][:4].fill_(-3)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        compare(bufs, n, want, total + 64)
