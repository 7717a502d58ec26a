"""rr_rdbsave_batch with RR_RDBSAVE_LZF on the GPU (include/rr_rdbsave.h, "LZF").

The streams are the library's own, so nothing is compared with a CPU compressor's bytes.  Every
test checks the whole answer instead (check_lzf): each payload is read by tests/lzf_reference.py's
loader, every LZF string has clen <= len - 4 and a stream that lzf_d.c's rule decodes to exactly
len bytes, the payload with its LZF strings written back raw is tests/rdb_reference.py's payload
byte for byte (so every other byte is the flag-off byte, and the parsed value is the model of the
flat value), offsets, statuses, types and totals are consistent, and a canary behind every buffer
is intact.  On top of that each test states what its strings must have become.

Size assertion (test_compressed_size): the GPU's bytes for the eligible strings of a fixed corpus
against lzf_reference.compress (lzf_c.c over a zeroed table) under the same len - 4 rule, measured
on an MI355X: GPU 9,578,537 bytes, yardstick 9,561,186, excess 0.1815 %; the test allows 2 points more.
"""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import flat_forge as ff
import lzf_reference as lz
import rdb_reference as ref
from test_gpu_rdbsave import CANARY, INT_RULE, _dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snappy")
MEASURED_EXCESS = 0.001815         # (GPU - yardstick) / yardstick on the corpus of test_compressed_size
WPB, GRID_CAP = 4, 16384          # rr_rdbsave.hip: waves per workgroup, the grid's cap


def _rand(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def run_device(engine, values, elems, arena, data_cap=None, room=None, fill=-2, lzf=True, flags=None, stream=None):
    """The device call over canaries: (offsets, status, types, totals, data bytes up to room)."""
    n = len(values)
    if room is None:
        room = rr.rdbsave_bound(values, elems) + 64
    cap = room - 64 if data_cap is None else data_cap
    out = torch.full((max(room, cap + 64),), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_types = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    engine.rdbsave_device(_dev(values), _dev(elems), _dev(arena), out[:cap], d_off, d_types[:n], d_status[:n], d_tot,
                          list_fill=fill, lzf=lzf, flags=flags, stream=stream)
    torch.cuda.synchronize()
    ty, st = d_types.cpu().numpy(), d_status.cpu().numpy()
    assert (ty[n:] == CANARY).all() and (st[n:] == CANARY).all()
    t = d_tot.cpu().numpy().view(np.uint64)
    totals = {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])}
    return d_off.cpu().numpy().view(np.uint64), st[:n], ty[:n], totals, out.cpu().numpy()


def verify(values, elems, arena, got, data_cap=None, fill=-2):
    """The whole answer of one call (see the module's docstring).  Returns per value the LZF strings
    met, as (clen, len, stream, bytes), None for a value that was not written."""
    offsets, status, types, totals, data = got
    n = len(values)
    r_types, _, _, _, r_totals, r_payloads = ref.save_batch(values, elems, arena, fill)
    assert np.array_equal(types, r_types)
    assert int(offsets[0]) == 0 and (np.diff(offsets.astype(np.int64)) >= 0).all()
    total = int(offsets[n])
    cap = total if data_cap is None else data_cap
    met, written, n_bad, pay = [], 0, 0, 0
    flat = list(ref.flat_values(values, elems, arena))
    ab = arena.tobytes()
    for i in range(n):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if r_payloads[i] is None:
            assert status[i] == rr.E_ENCODE and o1 == o0, i
            n_bad += 1
            met.append(None)
            continue
        assert o1 > o0, i
        if o1 > cap:
            assert status[i] == rr.E_CAPACITY, i
            n_bad += 1
            met.append(None)
            continue
        assert status[i] == 0, i
        payload = bytes(data[o0:o1])
        plain, strings = lz.expand(int(types[i]), payload)
        assert plain == r_payloads[i], f"value {i}: not the reference's payload once its LZF strings are raw again"
        val, descs = flat[i]
        used = descs[:1] if val["type"] in (rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST) else descs
        assert ref.load(int(types[i]), plain) == ref.model(val, used, ab), i
        for clen, ulen, _, _ in strings:
            assert ulen > 20 and 0 < clen <= ulen - 4, (i, clen, ulen)
        pay += sum(d[2] for d in used if d[0] in (rr.K_STR, rr.K_ZLRAW))
        met.append(strings)
        written = o1
    # nothing behind the last value written: not in a value that did not fit, not behind the buffer
    first_cut = next((i for i in range(n) if status[i] == rr.E_CAPACITY), None)
    end = int(offsets[first_cut]) if first_cut is not None else total
    if first_cut is not None:
        assert (status[first_cut:][status[first_cut:] != rr.E_ENCODE] == rr.E_CAPACITY).all()
    assert (data[end:] == CANARY).all(), f"byte {end + int(np.nonzero(data[end:] != CANARY)[0][0])} written"
    assert totals == {"n_elems": r_totals["n_elems"], "bytes": total, "n_bad": n_bad, "payload": pay}
    assert total <= r_totals["bytes"]                       # never larger than the flag-off output
    return met


def check_lzf(engine, values, elems, arena, data_cap=None, fill=-2, room=None):
    got = run_device(engine, values, elems, arena, data_cap=data_cap, fill=fill, room=room)
    return verify(values, elems, arena, got, data_cap, fill), got


def strings_batch(strings, seed=0):
    f = ff.Flat(seed)
    for s in strings:
        f.add(rr.T_STRING, 8 if len(s) <= 44 else 0, [s])
    return f.done()


def one_each(engine, strings, seed=0):
    """Each string as a String value: the list of its LZF tuple or None (raw), and the call's answer."""
    v, e, a = strings_batch(strings, seed)
    met, got = check_lzf(engine, v, e, a)
    assert all(m is not None and len(m) <= 1 for m in met)
    return [m[0] if m else None for m in met], got, (v, e, a)


def flag_off(engine, v, e, a):
    return run_device(engine, v, e, a, lzf=False)


# ---- threshold ----------------------------------------------------------------------------------
def test_threshold_and_incompressible(engine):
    rng = np.random.default_rng(11)
    runs = [b"z" * k for k in (20, 21, 22, 24, 25, 4096)]
    noise = [_rand(rng, k) for k in (21, 64, 4096, 70000)]
    forms, got, batch = one_each(engine, runs + noise)
    assert forms[0] is None                                   # rdb.c:426: len > 20
    assert all(f is not None for f in forms[1:6])
    assert forms[5][0] <= 64                                  # 16 back references and a 2-byte literal make 50
    assert all(f is None for f in forms[6:])                  # no valid stream of noise is shorter than it
    off = flag_off(engine, *batch)
    for i in [0] + list(range(6, 10)):                        # raw: the flag-off bytes
        a, b = (bytes(g[4][int(g[0][i]):int(g[0][i + 1])]) for g in (got, off))
        assert a == b


# ---- rdbSaveLen widths ----------------------------------------------------------------------------
def test_len_widths(engine):
    lens = (63, 64, 16383, 16384)
    forms, _, _ = one_each(engine, [b"q" * k for k in lens] + [(b"abcdefg" * 3000)[:k] for k in lens])
    assert all(f is not None for f in forms) and [f[1] for f in forms] == list(lens) * 2


@pytest.mark.parametrize("edge,lo,hi,zeros", [(64, 30, 75, 300), (16384, 15800, 15900, 2000)])
def test_clen_widths(engine, edge, lo, hi, zeros):
    """R bytes of noise then a zero run, R swept a byte at a time: clen crosses `edge`, so both widths
    of rdbSaveLen(clen) are written."""
    noise = _rand(np.random.default_rng(12), hi)
    forms, _, _ = one_each(engine, [noise[:r] + bytes(zeros) for r in range(lo, hi)])
    assert all(f is not None for f in forms)
    clens = [f[0] for f in forms]
    assert min(clens) < edge <= max(clens), (min(clens), max(clens))
    assert edge - 1 in clens or edge - 2 in clens            # (a step is 1 or 2: the sweep comes close below)
    assert edge in clens or edge + 1 in clens                # and lands at or just above


# ---- match distance, match length, literal runs ---------------------------------------------------
def _refs(stream, kinds=None):
    """(offset, length) of every back reference of a valid stream; kinds collects 'L' / 'R' per item."""
    out, ip = [], 0
    while ip < len(stream):
        c = stream[ip]
        if kinds is not None:
            kinds.append("L" if c < 32 else "R")
        if c < 32:
            ip += 2 + c
            continue
        ln = c >> 5
        ip += 1
        if ln == 7:
            ln += stream[ip]
            ip += 1
        out.append((((c & 0x1F) << 8 | stream[ip]) + 1, ln + 2))
        ip += 1
    return out


def test_match_distance(engine):
    rng = np.random.default_rng(13)
    r = _rand(rng, 8193)
    head = b"The quick brown fox jumps over the lazy dog, and 100 bytes are enough to be worth a back reference, no?"[:100]
    assert len(head) == 100
    cases = [r[:8192] + r[:100], r + r[:100],                 # as noise: the literals' run bytes outweigh the repeat, raw
             head + bytes(8092) + head, head + bytes(8093) + head,   # the repeat at distance 8192 and 8193
             r[:8192] + r[:100] + bytes(600), r + r[:100] + bytes(600)]
    forms, _, _ = one_each(engine, cases)
    assert forms[0] is None and forms[1] is None
    assert all(f is not None for f in forms[2:])
    at8192 = _refs(forms[2][2])
    assert (8192, 100) in at8192                              # the farthest offset the format has
    assert all(o <= 8192 for f in forms[2:] for o, _ in _refs(f[2]))
    assert not any(o > 4096 and ln >= 50 for o, ln in _refs(forms[3][2]))   # 8193 is out of reach


def test_match_lengths_and_periods(engine):
    rng = np.random.default_rng(14)
    cases = []
    for rep in (3, 8, 9, 10, 264, 265, 266, 600):
        pre = _rand(rng, 40)
        body = _rand(rng, rep)
        cases.append(pre + body + b"\x01\x02" + body + bytes(80))   # (the zero tail keeps it worth compressing)
    for period in (1, 2, 3, 5):
        cases.append(_rand(rng, 10) + (_rand(rng, period) * 400)[:700])
    forms, _, _ = one_each(engine, cases)
    assert all(f is not None for f in forms)
    for f in forms:
        assert all(3 <= ln <= 264 for _, ln in _refs(f[2]))
    assert any(ln == 264 for _, ln in _refs(forms[7][2]))     # 600 bytes: the longest reference, then the rest
    for k, period in enumerate((1, 2, 3, 5)):
        assert any(o == period and ln > o for o, ln in _refs(forms[8 + k][2]))   # an overlapping copy


def test_literal_runs(engine):
    rng = np.random.default_rng(15)
    cases = [_rand(rng, k) + b"r" * 200 for k in (31, 32, 33, 64, 65)]
    cases.append(_rand(rng, 30) + b"s" * 100)                 # a match that ends on the last byte
    cases.append(b"t" * 100 + b"!")                           # a last literal run of one byte
    forms, _, _ = one_each(engine, cases)
    assert all(f is not None for f in forms)
    assert forms[6][2][-2:] == b"\x00!"
    kinds = []
    _refs(forms[5][2], kinds)
    assert kinds[-1] == "R"                                   # ends in a back reference


def test_positions_past_16_bits(engine):
    rng = np.random.default_rng(16)
    text = b" ".join(bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(400))
    cases = [(text * 40)[:k] for k in (65535, 65536, 70000)]
    cases.append((_rand(rng, 5000) * 41)[:200 * 1024])        # period 5000, across three chunks
    forms, _, _ = one_each(engine, cases)
    assert all(f is not None for f in forms)
    # the second period alone is 5000 bytes in back references of 3 bytes per 264: whatever the table
    # loses of the later periods, the stream is well below the string
    assert forms[3][0] < 200 * 1024 - 4000


# ---- every site -----------------------------------------------------------------------------------
def every_site_batch():
    f = ff.Flat(17)
    rng = f.rng

    def mix(k):
        if k % 4 == 0:
            return b"member:%04d:" % k + b"x" * int(rng.integers(14, 90))       # eligible
        if k % 4 == 1:
            return b"m%d" % k                                                     # short
        if k % 4 == 2:
            return INT_RULE[k % len(INT_RULE)]                                    # integer rule
        return _rand(rng, int(rng.integers(21, 70)))                              # eligible, incompressible
    f.add(rr.T_STRING, 0, [b"raw string " * 30])
    for k in (21, 30, 44):
        f.add(rr.T_STRING, 8, [(b"embstr-" * 7)[:k]])
    f.add(rr.T_STRING, 1, [-(2**40)])
    f.add(rr.T_STRING, 1, [12345])
    f.add(rr.T_SET_HT, 0, [mix(k) for k in range(130)])
    f.add(rr.T_HASH_HT, 0, [mix(k) for k in range(200)])
    items = []
    for k in range(70):
        items += [b"zset member number %d " % k * 3, ("score", struct.unpack("<Q", struct.pack("<d", k / 4))[0])]
    f.add(rr.T_ZSET_SKIPLIST, 0, items)
    data, offs = rr.gen_batch(3, 4)
    zv, ze, za = rr.host_decode_ex(data, offs, rr.CTX_ZL_RAW)[:3]
    assert int(ze["kind"][0]) == rr.K_ZLRAW
    zl = bytes(za[int(ze["data"][0]):int(ze["data"][0]) + int(ze["len"][0])])
    f.add(rr.T_HASH_ZIPLIST, 0, [("zl", zl)])
    f.add(rr.T_ZSET_ZIPLIST, 0, [("zl", zl), 9])
    f.add(rr.T_SET_INTSET, 4, list(range(0, 4000, 40)))                           # a 408-byte blob of small ints
    f.add(rr.T_LIST_QUICKLIST, 0, [b"list entry, repeated " * 4] * 30)
    f.add(rr.T_LIST_QUICKLIST, 0, [])
    return f.done()


def test_every_site(engine):
    v, e, a = every_site_batch()
    met, got = check_lzf(engine, v, e, a)
    off = flag_off(engine, v, e, a)
    n_lzf = [len(m) for m in met]
    assert n_lzf[0] == 1 and n_lzf[1:4] == [1, 1, 1]          # RAW and EMBSTR Strings
    assert n_lzf[4] == n_lzf[5] == 0                          # INT Strings
    assert n_lzf[6] == 33 and n_lzf[7] == 50                  # every fourth member, past the first round of 64
    assert n_lzf[8] == 70                                     # members, not scores
    assert n_lzf[9] == n_lzf[10] == 1                         # ZLRAW
    assert n_lzf[11:] == [0, 0, 0]                            # intset blob and List nodes stay raw
    for i in (4, 5, 11, 12, 13):
        x, y = (bytes(g[4][int(g[0][i]):int(g[0][i + 1])]) for g in (got, off))
        assert x == y and (b"\xC3" not in x[:1])
    assert int(got[0][-1]) < int(off[0][-1])


# ---- independence ---------------------------------------------------------------------------------
def test_stream_depends_on_the_bytes_only(engine):
    s = (b"independent of where it lies; " * 4)[:100]
    alone, alone_got = check_lzf(engine, *strings_batch([s]))
    size = int(alone_got[0][1])                               # 0xC3, the two lengths, the stream
    assert len(alone[0]) == 1
    f = ff.Flat(18)
    total = 0
    for a in range(16):
        pad = (a - total - 1) % 16                            # 1 + pad bytes in front: output alignment a
        f.add(rr.T_STRING, 8, [b"p" * pad])
        total += 1 + pad + size
        f.arena += bytes((a - len(f.arena)) % 16)
        at = len(f.arena)
        f.arena += s
        f.add(rr.T_STRING, 0, [("raw", rr.K_STR, at, len(s), 0, 0)])
    v, e, a = f.done()
    met, got = check_lzf(engine, v, e, a)
    streams = {m[0][2] for m in met[1::2]}
    assert len(streams) == 1 and all(len(m) == 1 for m in met[1::2])
    assert len({int(got[0][i]) % 16 for i in range(1, 32, 2)}) == 16
    # 1000 Strings over one arena string
    f = ff.Flat(19)
    at = f.put(s)
    for _ in range(1000):
        f.add(rr.T_STRING, 0, [("raw", rr.K_STR, at, len(s), 0, 0)])
    v, e, a = f.done()
    met, first = check_lzf(engine, v, e, a)
    assert {m[0][2] for m in met} == streams
    # and a second run gives the same bytes
    again = run_device(engine, v, e, a)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[4], first[4])


# ---- capacity --------------------------------------------------------------------------------------
def test_capacity(engine):
    v, e, a = strings_batch([b"first " * 20, b"second" * 50, b"third " * 30, b"x"])
    full, whole = check_lzf(engine, v, e, a)
    offsets = whole[0]
    assert all(len(m) == 1 for m in full[:3])
    o1, o2 = int(offsets[1]), int(offsets[2])
    for cap, ok in (((o1 + o2) // 2, 1), (o2, 2), (o2 - 1, 1)):
        met, got = check_lzf(engine, v, e, a, data_cap=cap)
        assert np.array_equal(got[0], offsets)                # complete whatever data_cap is
        assert (got[1][:ok] == 0).all() and (got[1][ok:] == rr.E_CAPACITY).all()
    # host entry: n == 0 with the flag set, and a small batch
    none_e, none_a = np.zeros(0, rr.ELEM_DT), np.zeros(0, np.uint8)
    ty, data, off, st, tot = engine.rdbsave_host(v[:0], none_e, none_a, lzf=True)
    assert len(ty) == len(st) == len(data) == 0 and tot == {"n_elems": 0, "bytes": 0, "n_bad": 0, "payload": 0}
    ty, data, off, st, tot = engine.rdbsave_host(v, e, a, lzf=True)
    assert np.array_equal(off, offsets) and (st == 0).all()
    assert bytes(data) == bytes(whole[4][:int(offsets[-1])])


# ---- past one grid ---------------------------------------------------------------------------------
def test_second_grid_stride(engine):
    """65,536 + 61 values: the size and emit kernels' second grid-stride step with the flag on.  The
    expectation is the base batch's own checked payloads, tiled: a stream depends on its bytes only."""
    bv, be, ba = every_site_batch()
    base_n = 61
    bv = ff.tile_records(bv, base_n)
    base_ref, pays = ff.tiling_reference(bv, be, ba, fill=-2)
    # (tiled records share descriptors: room from the flag-off size, which the flag never exceeds)
    met, base = check_lzf(engine, bv, be, ba, room=((int(base_ref[2][-1]) + 15) & ~15) + 64)
    assert sum(len(m) for m in met) > 100
    n = GRID_CAP * WPB + 61
    reps = (n + base_n - 1) // base_n
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(np.tile(np.diff(base[0].astype(np.int64)), reps)[:n])
    total = int(offsets[n])
    want = np.tile(base[4][:int(base[0][-1])], reps)[:total]
    got = run_device(engine, ff.tile_records(bv, n), be, ba, room=((total + 15) & ~15) + 64, data_cap=total)
    assert np.array_equal(got[0], offsets) and (got[1] == 0).all()
    assert np.array_equal(got[2], np.tile(base[2], reps)[:n])
    assert np.array_equal(got[4][:total], want) and (got[4][total:] == CANARY).all()
    assert got[3] == {"n_elems": int(np.tile(bv["n_elems"].astype(np.int64), reps)[:n].sum()), "bytes": total, "n_bad": 0,
                      "payload": int(np.tile(np.asarray(pays, np.int64), reps)[:n].sum())}


# ---- stream and graph ------------------------------------------------------------------------------
def test_side_stream_and_graph_replay():
    """decode -> save with the flag on a side stream; after that warm call the pair captured and
    replayed three times, the last over a second batch."""
    eng = rr.Engine(0)
    try:
        n = 3000
        batches = [rr.gen_batch(3, n, seed=61), rr.gen_batch(4, n, seed=62)]
        hosts = [rr.host_decode(d, o)[:3] for d, o in batches]
        nb = (max(int(o[-1]) for _, o in batches) + 15) & ~15
        cap = max(rr.elem_bound(n, int(o[-1])) for _, o in batches)
        room = max(rr.rdbsave_bound(h[0], h[1]) for h in hosts) + 64
        dev = torch.device("cuda:0")
        d_data = torch.zeros(nb, dtype=torch.uint8, device=dev)
        d_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_vals = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_elems = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
        d_arena = torch.zeros(nb, dtype=torch.uint8, device=dev)
        d_tot = torch.zeros(4, dtype=torch.int64, device=dev)
        out = torch.zeros(room, dtype=torch.uint8, device=dev)
        o_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        o_ty = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
        o_st = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
        o_tot = torch.zeros(4, dtype=torch.int64, device=dev)
        eng.reserve(n, nb)

        def load(k):
            dd, oo = batches[k]
            d_data.zero_()
            d_data[:dd.size].copy_(torch.from_numpy(dd))
            d_offs.copy_(torch.from_numpy(oo.view(np.int64)))

        def canaries():
            for t in (out, o_ty, o_st):
                t.fill_(CANARY)
            d_vals.zero_()
            d_elems.zero_()
            o_off.fill_(7)
            o_tot.fill_(-3)

        def check(k, what):
            ty, st = o_ty.cpu().numpy(), o_st.cpu().numpy()
            assert (ty[n:] == CANARY).all() and (st[n:] == CANARY).all(), what
            t = o_tot.cpu().numpy().view(np.uint64)
            totals = {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])}
            got = (o_off.cpu().numpy().view(np.uint64), st[:n], ty[:n], totals, out.cpu().numpy())
            met = verify(*hosts[k], got, data_cap=room - 64)
            # config 3: a ziplist a value, each worth compressing; config 4: a few of its strings
            assert (st[:n] == 0).all() and sum(len(m) for m in met) > (n // 2 if k == 0 else 0), what

        def chain(stream):
            eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=stream)
            eng.rdbsave_device(d_vals, d_elems, d_arena, out[:room - 64], o_off, o_ty[:n], o_st[:n], o_tot, stream=stream,
                               lzf=True)

        load(0)
        canaries()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain(s)                                           # the warm call: sizes the scratch
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        check(0, "side stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            chain(torch.cuda.current_stream())
        for r in range(3):
            if r == 2:
                load(1)
            canaries()
            g.replay()
            torch.cuda.synchronize()
            check(1 if r == 2 else 0, f"replay {r}")
    finally:
        eng.close()


# ---- flag handling ---------------------------------------------------------------------------------
def test_flags(engine):
    v, e, a = strings_batch([b"flagged " * 10, b"short"])
    for bad in (2, 3, 1 << 31):
        with pytest.raises(rr.RRError, match=r"\(-1\)"):      # RR_API_EINVAL
            run_device(engine, v, e, a, flags=bad)
        with pytest.raises(rr.RRError, match=r"\(-1\)"):
            engine.rdbsave_host(v, e, a, flags=bad)
    zero = run_device(engine, v, e, a, flags=0)
    types, data, offsets, status, totals, _ = ref.save_batch(v, e, a)     # what opts == NULL gives (test_gpu_rdbsave.py)
    assert np.array_equal(zero[0], offsets) and zero[3] == totals
    assert np.array_equal(zero[4][:int(offsets[-1])], data)
    n, room = len(v), rr.rdbsave_bound(v, e)
    outs = []
    for opts in (None, rr.RdbSaveOpts(-2, 0)):
        out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_ty = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        dv, de, da = _dev(v), _dev(e), _dev(a)
        inb = rr.FlatBatch(dv.data_ptr(), de.data_ptr(), da.data_ptr(), n, len(e), len(a))
        outb = rr.BlobBatch(out.data_ptr(), d_off.data_ptr(), n, room)
        rc = rr.lib().rr_rdbsave_batch(engine._ctx, C.byref(inb), C.byref(outb), C.c_void_p(d_ty.data_ptr()),
                                       C.c_void_p(d_st.data_ptr()), C.c_void_p(d_tot.data_ptr()),
                                       C.byref(opts) if opts is not None else None, None)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0][:int(offsets[-1])], data)


# ---- compressed size -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def size_corpus():
    """Config 3 and config 4 at 10K values, and three files of tests/golden/snappy as one String each."""
    parts = []
    for cfg in (3, 4):
        data, offs = rr.gen_batch(cfg, 10000)
        parts.append(rr.host_decode(data, offs)[:3])
    parts.append(strings_batch([open(os.path.join(GOLDEN, name), "rb").read()
                                for name in ("alice29.txt", "html", "geo.protodata")]))
    return parts


def yardstick_bytes(values, elems, arena):
    """(bytes the eligible strings take under lzf_reference.compress and the len - 4 rule, their
    number, how many took the LZF form)."""
    ab = arena.tobytes()
    total = count = lzfd = 0
    for val, descs in ref.flat_values(values, elems, arena):
        if descs is None or not ref.accepted_value(val, descs, len(arena)):
            continue
        for s in lz.eligible_strings(val, descs, ab):
            c = lz.compress(s, len(s) - 4)
            count += 1
            lzfd += c is not None
            total += lz.lzf_cost(s, len(c)) if c is not None else len(ref.save_len(len(s))) + len(s)
    return total, count, lzfd


def test_compressed_size(engine):
    gpu = yard = 0
    for k, (v, e, a) in enumerate(size_corpus()):
        y, count, lzfd = yardstick_bytes(v, e, a)
        if k == 0:
            assert 2 * lzfd >= count                          # the yardstick compresses config 3 at all
        on, off = run_device(engine, v, e, a), flag_off(engine, v, e, a)
        # the eligible strings' bytes: the flag-off output less everything else, which the flag leaves alone
        ab = a.tobytes()
        elig_raw = sum(len(ref.save_len(len(s))) + len(s) for val, descs in ref.flat_values(v, e, a)
                       if descs is not None and ref.accepted_value(val, descs, len(a))
                       for s in lz.eligible_strings(val, descs, ab))
        g = int(on[0][-1]) - (int(off[0][-1]) - elig_raw)
        print(f"corpus part {k}: eligible strings {count}, yardstick LZF {lzfd}, raw {elig_raw}, yardstick {y}, GPU {g}")
        gpu += g
        yard += y
    print(f"GPU {gpu} bytes, yardstick {yard} bytes, excess {(gpu - yard) / yard:.4%}")
    assert gpu <= yard * (1 + MEASURED_EXCESS + 0.02)
