"""rr_rdbread_split and rr_rdbread_verify on the GPU against tests/rdbread_reference.py: every byte,
offset, status and total, with a canary behind every buffer a call writes.  The sizes come from the
kernels' exported shape: one grid stride of records (a wave a record), the 16 bytes a lane copies
and the bytes a wave copies a step; the CRC's run and piece.  No input here is outside the
contract: a corrupt record is one the header defines a status for, and the index's
[rec_start, rec_end) and data_cap bound every read."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import rdb_reference as ref
import rdbfile_reference as rf
import rdbload_reference as ld
import rdbread_reference as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
LANE, STEP, STRIDE = rr.RDBREAD_LANE_BYTES, rr.RDBREAD_WAVE_STEP, rr.RDBREAD_MAX_WAVES
RUN, PIECE = rr.CRC64_RUN, rr.CRC64_PIECE
C1 = 0x8F3B5D7A1C2E4F60          # a nonzero incoming checksum
RNG = np.random.default_rng(20261021)
rand = lambda n: RNG.integers(0, 256, n, dtype=np.uint8).tobytes()
U64_MAX = (1 << 64) - 1


def _dev(a, dtype=np.uint8):
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda() if a.size else torch.zeros(0, dtype=torch.uint8, device="cuda")


def rec(typ, key_enc, payload, prefix=b""):
    return prefix + bytes([typ]) + key_enc + payload


def lz(s):
    return R.lzf_string(R.lzf_literal(s), len(s))


def place(recs, gaps=None):
    """The records one behind the other, gaps[i] junk bytes in front of record i: (data, starts, ends)."""
    parts, starts, ends, at = [], [], [], 0
    for i, r in enumerate(recs):
        g = gaps[i] if gaps is not None else 0
        parts.append(b"\xFF" * g)                            # (an opcode no record may hold: a stray read shows)
        at += g
        starts.append(at)
        at += len(r)
        ends.append(at)
        parts.append(r)
    return b"".join(parts), np.array(starts, np.uint64), np.array(ends, np.uint64)


def run_split(engine, data, starts, ends, key_cap=None, pay_cap=None, data_cap=None, stream=None, d_data=None, want=None,
              shift=0):
    """The device call on canary-filled buffers against the reference.  key_cap / pay_cap None: exactly
    what is needed.  d_data / shift: the stream already on the device, its records `shift` bytes further."""
    n = len(starts)
    if want is None:
        want = R.split(data, starts, ends, data_cap, key_cap, pay_cap)
    ktot, ptot = int(want["key_offsets"][n]), int(want["pay_offsets"][n])
    kc = ktot if key_cap is None else key_cap
    pc = ptot if pay_cap is None else pay_cap
    kd = torch.full((kc + 64,), CANARY, dtype=torch.uint8, device="cuda")
    pd = torch.full((pc + 64,), CANARY, dtype=torch.uint8, device="cuda")
    ko = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    po = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    ty = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ex = torch.full((n + 4,), 7, dtype=torch.int64, device="cuda")
    idl = torch.full((n + 4,), 7, dtype=torch.int64, device="cuda")
    fq = torch.full((n + 4,), 7, dtype=torch.int16, device="cuda")
    res = torch.full((24 + 8,), CANARY, dtype=torch.uint8, device="cuda")
    if d_data is None:
        d_data = _dev(np.frombuffer(bytes(data), np.uint8))
    d_rs = torch.from_numpy((np.asarray(starts, np.uint64) + np.uint64(shift)).view(np.int64).copy()).cuda()
    d_re = torch.from_numpy((np.asarray(ends, np.uint64) + np.uint64(shift)).view(np.int64).copy()).cuda()
    engine.rdbread_split(d_data, d_rs, d_re, 9, kd, ko[:n + 1], pd, po[:n + 1], ty[:n], ex[:n], idl[:n], fq[:n], st[:n], res[:24],
                         stream=stream, data_cap=data_cap, key_cap=kc, pay_cap=pc)
    torch.cuda.synchronize()
    g = ko.cpu().numpy()
    assert np.array_equal(g[:n + 1].view(np.uint64), want["key_offsets"]) and (g[n + 1:] == 7).all()
    g = po.cpu().numpy()
    assert np.array_equal(g[:n + 1].view(np.uint64), want["pay_offsets"]) and (g[n + 1:] == 7).all()
    g = st.cpu().numpy()
    assert np.array_equal(g[:n], want["status"]), (g[:n].tolist(), want["status"].tolist())
    assert (g[n:] == CANARY).all()
    g = ty.cpu().numpy()
    assert np.array_equal(g[:n], want["types"]) and (g[n:] == CANARY).all()
    g = ex.cpu().numpy()
    assert np.array_equal(g[:n], want["expires"]) and (g[n:] == 7).all()
    g = idl.cpu().numpy()
    assert np.array_equal(g[:n].view(np.uint64), want["idle"]) and (g[n:] == 7).all()
    g = fq.cpu().numpy()
    assert np.array_equal(g[:n], want["freq"]) and (g[n:] == 7).all()
    r = res.cpu().numpy()
    assert (r[24:] == CANARY).all()
    assert struct.unpack("<QQI", r[:20].tobytes()) == (want["bytes"], want["n_bad"], want["result_status"])
    for name, buf, cap, items, offs in (("key", kd, kc, want["keys"], want["key_offsets"]), ("payload", pd, pc, want["pays"], want["pay_offsets"])):
        exp = np.full(cap + 64, CANARY, np.uint8)
        for x, o in zip(items, offs):
            if x:
                exp[int(o):int(o) + len(x)] = np.frombuffer(x, np.uint8)
        got = buf.cpu().numpy()
        if not np.array_equal(got, exp):
            at = int(np.nonzero(got != exp)[0][0])
            raise AssertionError(f"{name} byte {at} (record {int(np.searchsorted(offs, at, side='right')) - 1}): got {got[at]:#x}, want {exp[at]:#x}")
    return want


def run_verify(engine, d_data, eof_at, crc_in=0, stream=None):
    state = torch.from_numpy(np.array([crc_in, 0x1111, 0x2222], np.uint64).view(np.int64).copy()).cuda()
    res = torch.full((24 + 8,), CANARY, dtype=torch.uint8, device="cuda")
    engine.rdbread_verify(d_data, eof_at, state[:2], res[:24], stream=stream)
    torch.cuda.synchronize()
    st = state.cpu().numpy().view(np.uint64)
    r = res.cpu().numpy()
    assert st[2] == 0x2222 and int(st[1]) == eof_at + 1 and (r[24:] == CANARY).all()
    nbytes, n_bad, status = struct.unpack("<QQI", r[:20].tobytes())
    assert nbytes == eof_at + 9 and n_bad == (status == rr.RDBDUMP_E_CRC)
    return status, int(st[0])


# ---- round trip: rr_rdbfile_section's output back into its inputs ----------------------------------------
def section_inputs(n, small=False):
    keys = [b"k%d" % i if small or i % 5 else str(i * 997 - 40000).encode() for i in range(n)]
    pays = [ref.save_raw_string(b"v" if small else rand(int(RNG.integers(0, 120)))) for _ in range(n)]
    ex = np.where(np.arange(n) % 4 == 0, 1_700_000_000_000 + np.arange(n), -1).astype(np.int64)
    idle = (np.arange(n, dtype=np.uint64) * np.uint64(7919)) % np.uint64(70000)
    freq = (np.arange(n) % 256).astype(np.uint8)
    return keys, pays, ex, idle, freq


def pk(xs):
    offs = np.zeros(len(xs) + 1, np.uint64)
    if len(xs):
        np.cumsum([len(x) for x in xs], out=offs[1:])
    return np.frombuffer(b"".join(xs), np.uint8), offs


def roundtrip(engine, n, small=False, stream=None):
    keys, pays, ex, idle, freq = section_inputs(n, small)
    hd = rf.head("6.0.20", 1700000000, 1 << 33, (0, "a" * 40, 1)) + rf.selectdb(0, n, n // 4)
    sec, ro, rs, crc, res = engine.rdbfile_section_host(*pk(pays), np.zeros(n, np.uint8), np.zeros(n, np.uint8), *pk(keys),
                                                        expires=ex, idle=idle, freq=freq, head=hd,
                                                        flags=rr.RDBFILE_IDLE | rr.RDBFILE_FREQ | rr.RDBFILE_EOF)
    assert res["status"] == 0 and res["n_bad"] == 0
    s = sec.tobytes()
    ix = rr.rdbread_index(s)
    assert ix["rc"] == rr.RDBREAD_DONE and len(ix["rec_start"]) == n and ix["cksum"] == crc
    assert np.array_equal(ix["rec_start"], ro[:n]) and np.array_equal(ix["rec_end"], ro[1:])
    d = _dev(sec)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    want = run_split(engine, s, ix["rec_start"], ix["rec_end"], d_data=d, stream=stream)
    assert want["keys"] == keys and want["pays"] == pays and (want["status"] == 0).all() and (want["types"] == 0).all()
    assert np.array_equal(want["expires"], ex) and np.array_equal(want["idle"], idle) and np.array_equal(want["freq"], freq)
    assert run_verify(engine, d, ix["eof_at"], stream=stream) == (0, crc)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_roundtrip(engine, n):
    roundtrip(engine, n)


def test_roundtrip_one_grid_stride_plus_one(engine):
    roundtrip(engine, STRIDE + 1, small=True)


def test_roundtrip_on_a_side_stream(engine):
    roundtrip(engine, 200, stream=torch.cuda.Stream())


# ---- keys -------------------------------------------------------------------------------------------------
def test_key_edges(engine):
    lens = [0, 1, 63, 64, 16383, 16384, LANE - 1, LANE, LANE + 1, STEP - 1, STEP, STEP + 1, 2 * STEP + 5]
    recs = [rec(0, R.raw(rand(k)), R.raw(b"v")) for k in lens]
    ints = (0, -128, 127, -32768, 32767, -2147483648, 2147483647)
    recs += [rec(0, R.int_string(v), R.raw(b"v")) for v in ints]
    recs += [rec(0, b"\xC1\x05\x00", R.raw(b"v")), rec(0, b"\xC2\xFF\xFF\xFF\xFF", R.raw(b"v"))]     # wider forms than needed
    long = rand(40) * 30
    recs += [rec(2, lz(long), R.counted([R.raw(b"m")])),                                            # literal runs
             rec(0, R.lzf_string(b"\x00a" + R.lzf_backref(264, 1), 265), R.raw(b"v")),               # an overlapping reference
             rec(0, R.lzf_string(b"\x02abc" + R.lzf_backref(3, 3) + b"\x00z", 7), R.raw(b"v")),
             rec(0, R.lzf_string(R.lzf_literal(rand(70)) + R.lzf_backref(100, 64), 170), R.raw(b"v"))]
    want = run_split(engine, *place(recs))
    assert (want["status"] == 0).all()
    assert [len(k) for k in want["keys"][:len(lens)]] == lens
    assert want["keys"][len(lens):len(lens) + len(ints)] == [str(v).encode() for v in ints]
    assert want["keys"][-4] == long and want["keys"][-3] == b"a" * 265 and want["keys"][-2] == b"abcabcz"


def test_lzf_key_length_rule(engine):
    """A stream that gives exactly, one under and one over its stated length; a reference before the start."""
    body = rand(50)
    good = rec(0, R.raw(b"good"), R.raw(b"v"))
    recs = [good, rec(0, R.lzf_string(R.lzf_literal(body), 50), R.raw(b"v")), good,
            rec(0, R.lzf_string(R.lzf_literal(body), 51), R.raw(b"v")), good,                       # one under its length
            rec(0, R.lzf_string(R.lzf_literal(body), 49), R.raw(b"v")), good,                       # one over
            rec(0, R.lzf_string(b"\x00a" + R.lzf_backref(3, 2), 4), R.raw(b"v")), good,             # before the start
            rec(0, R.lzf_string(b"", 0), R.raw(b"v")), good]
    want = run_split(engine, *place(recs))
    assert want["status"].tolist() == [0, 0, 0, R.E_KEY, 0, R.E_KEY, 0, R.E_KEY, 0, R.E_KEY, 0]
    assert want["keys"][1] == body


def aligned(lens, which):
    """For every length of lens, a record at each source x destination alignment 0-15 of its key
    (which == 0) or payload (which == 1): junk bytes in front of the record set the source, a filler
    record in front of it the destination."""
    recs, gaps, at, out = [], [], 0, 0
    for ln in lens:
        for sa in range(16):
            for da in range(16):
                pad = (da - out) % 16                        # the filler's key or payload
                f = rec(0, R.raw(b"f" * pad), R.raw(b"")) if which == 0 else rec(0, R.raw(b""), b"p" * pad)
                recs.append(f)
                gaps.append(0)
                at += len(f)
                out += pad
                body = rand(ln)
                r = rec(0, R.raw(body), R.raw(b"")) if which == 0 else rec(0, R.raw(b"k"), body)
                lead = (2 if ln < 64 else 3) if which == 0 else 3   # the body's offset in the record
                g = (sa - (at + lead)) % 16
                recs.append(r)
                gaps.append(g)
                at += g + len(r)
                out += ln
    return recs, gaps


def test_key_copy_alignments(engine):
    recs, gaps = aligned([1, LANE - 1, LANE + 1, 2 * LANE + 1, STEP + 37], 0)
    data, starts, ends = place(recs, gaps)
    want = run_split(engine, data, starts, ends)
    seen = {(int(s + (2 if len(k) < 64 else 3)) % 16, int(o) % 16) for s, k, o in zip(starts[1::2], want["keys"][1::2], want["key_offsets"][1::2])}
    assert len(seen) == 256 and (want["status"] == 0).all()


def test_payload_copy_alignments(engine):
    recs, gaps = aligned([0, 1, 15, 16, 17, 32, 33, STEP + 37], 1)
    data, starts, ends = place(recs, gaps)
    want = run_split(engine, data, starts, ends)
    seen = {(int(s + 3) % 16, int(o) % 16) for s, o in zip(starts[1::2], want["pay_offsets"][1::2])}
    assert len(seen) == 256 and (want["status"] == 0).all()
    assert sorted({len(p) for p in want["pays"][1::2]}) == [0, 1, 15, 16, 17, 32, 33, STEP + 37]


# ---- prefix opcodes -------------------------------------------------------------------------------------------
def test_prefix_opcodes(engine):
    fd = lambda v: b"\xFD" + struct.pack("<i", v)
    fc = lambda v: b"\xFC" + struct.pack("<q", v)
    f8 = lambda v: b"\xF8" + ref.save_len(v)
    pre = [b"", fd(0), fd(-1), fd(-(1 << 31)), fd((1 << 31) - 1), fc(0), fc(-2), fc(-(1 << 63)), fc((1 << 63) - 1),
           fc(1) + fc(2), fd(5) + fc(7), fc(7) + fd(5),                                            # a repeated one overwrites
           f8(0), f8(63), f8(64), f8(16383), f8(16384), f8((1 << 32) - 1), f8(1 << 32), f8(U64_MAX), b"\xF8\xC5",
           f8(3) + f8(1 << 40), b"\xF9\x00", b"\xF9\xFF", b"\xF9\x01\xF9\x02",
           fc(1700000000123) + f8(300) + b"\xF9\x09", b"\xF9\x09" + f8(300) + fc(1700000000123),
           (fc(1) + f8(2) + b"\xF9\x03") * 9]                                                       # more than one 64-byte load holds
    recs = [rec(int(t), R.raw(b"key%d" % i), rand(i), p) for i, (p, t) in enumerate(zip(pre, RNG.integers(0, 15, len(pre))))]
    want = run_split(engine, *place(recs))
    assert (want["status"] == 0).all()
    assert want["expires"][:12].tolist() == [-1, 0, -1000, -(1 << 31) * 1000, ((1 << 31) - 1) * 1000, 0, -2, -(1 << 63), (1 << 63) - 1, 2, 7, 5000]
    assert want["idle"][12:22].tolist() == [0, 63, 64, 16383, 16384, (1 << 32) - 1, 1 << 32, U64_MAX, 5, 1 << 40]
    assert want["freq"][22:25].tolist() == [0, 255, 2] and want["freq"][0] == -1 and want["idle"][0] == U64_MAX


# ---- status ------------------------------------------------------------------------------------------------------
def test_each_status_among_good_neighbours(engine):
    good = lambda i: rec(0, R.raw(b"good%d" % i), R.raw(rand(20 + i)), b"\xFC" + struct.pack("<q", i))
    bad = [
        (rec(0, R.raw(b"cut-in-key"), b"")[:-3], R.E_TRUNC),                                       # the key runs past rec_end
        (b"\xFC\x01\x02\x03", R.E_TRUNC),                                                          # the prefix does
        (b"\xF9\x01", R.E_TRUNC),                                                                  # no type byte
        (b"", R.E_TRUNC),
        (b"\xF8\x80\x00", R.E_TRUNC),
        (b"\x00", R.E_TRUNC),                                                                      # no key
        (b"\x00\x81" + b"\xFF" * 8 + b"abc", R.E_TRUNC),                                           # a key of 2^64 - 1 bytes
        (b"\x00\xC3\x05\x03ab", R.E_TRUNC),                                                        # an LZF stream past the end
        (b"\xF7" + R.raw(b"k"), R.E_OPCODE), (b"\xFA" + R.raw(b"k") + R.raw(b"v"), R.E_OPCODE),
        (b"\xFC" + bytes(8) + b"\xFB\x01\x01", R.E_OPCODE), (b"\xFE\x01", R.E_OPCODE), (b"\xF9\x05\xFF" + bytes(8), R.E_OPCODE),
        (b"\xF8\x82\x00" + R.raw(b"k"), R.E_OPCODE),                                               # an idle time of no form
        (b"\x00\xC4\x00\x00", R.E_KEY), (b"\x00\x82\x00\x00", R.E_KEY), (b"\x00\xBF", R.E_KEY),
        (rec(0, R.lzf_string(R.lzf_literal(b"abc"), 5), R.raw(b"v")), R.E_KEY),
        (rec(0, R.lzf_string(b"\x00a", 0x7FFFFFF0), R.raw(b"v")), R.E_KEY),
    ]
    recs, codes = [], []
    for i, (b, c) in enumerate(bad):
        recs += [good(i), b]
        codes += [0, c]
    recs.append(good(99))
    codes.append(0)
    data, starts, ends = place(recs, [i % 5 for i in range(len(recs))])
    want = run_split(engine, data, starts, ends)
    assert want["status"].tolist() == codes and want["n_bad"] == len(bad)
    # slices: reversed, past data_cap, and one whose end is the last byte
    n = len(starts)
    s2, e2 = starts.copy(), ends.copy()
    s2[2], e2[2] = ends[2], starts[2]
    e2[4] = np.uint64(len(data) + 1)
    s2[6], e2[6] = np.uint64(U64_MAX - 5), np.uint64(U64_MAX)
    s2[8], e2[8] = np.uint64(0), np.uint64(1 << 62)
    want = run_split(engine, data, s2, e2)
    assert [int(want["status"][i]) for i in (2, 4, 6, 8)] == [R.E_SLICE] * 4 and want["status"][n - 1] == 0
    # a data_cap inside the stream: the records past it are not read
    cap = int(ends[10])
    want = run_split(engine, data, starts, ends, data_cap=cap)
    assert (want["status"][11:] == R.E_SLICE).all() and want["status"][:11].tolist() == codes[:11]
    # a slice of exactly the limit is refused unread; nothing of it lies in the buffer
    want = run_split(engine, data, np.array([0, starts[0]], np.uint64), np.array([0x7FFFFFF0, ends[0]], np.uint64), data_cap=1 << 40)
    assert want["status"].tolist() == [R.E_SLICE, 0]


def test_capacity_and_sizing(engine):
    recs = [rec(0, R.raw(rand(10 + 3 * i)), rand(40 + 5 * i)) for i in range(8)] + [rec(0, lz(rand(33) * 4), rand(9)), rec(0, R.int_string(-77), rand(3))]
    data, starts, ends = place(recs)
    full = R.split(data, starts, ends)
    ktot, ptot = int(full["key_offsets"][-1]), int(full["pay_offsets"][-1])
    n = len(recs)
    # keys one byte short: the last record alone; its payload is not written either
    want = run_split(engine, data, starts, ends, key_cap=ktot - 1, pay_cap=ptot)
    assert want["status"].tolist() == [0] * (n - 1) + [rf.E_CAPACITY] and want["result_status"] == rf.E_CAPACITY
    # payloads short from the middle on
    want = run_split(engine, data, starts, ends, key_cap=ktot, pay_cap=int(full["pay_offsets"][5]) - 1)
    assert want["status"].tolist() == [0] * 4 + [rf.E_CAPACITY] * (n - 4)
    assert np.array_equal(want["key_offsets"], full["key_offsets"]) and np.array_equal(want["pay_offsets"], full["pay_offsets"])
    # the sizing call: capacities 0, complete offsets; then exactly that much
    want = run_split(engine, data, starts, ends, key_cap=0, pay_cap=0)
    assert (want["status"] == rf.E_CAPACITY).all() and int(want["key_offsets"][-1]) == ktot and want["bytes"] == ptot
    want = run_split(engine, data, starts, ends, key_cap=ktot, pay_cap=ptot)
    assert (want["status"] == 0).all() and want["result_status"] == 0
    # an empty batch
    run_split(engine, data, starts[:0], ends[:0])


def test_host_entry_points(engine):
    recs = [rec(int(t), R.raw(b"key:%d" % i), rand(5 * i), b"\xF9" + bytes([i])) for i, t in enumerate(RNG.integers(0, 15, 12))]
    recs[3] = b"\xFF"
    recs[5] = rec(0, lz(b"lzf-key " * 20), R.raw(b"v"))
    body = rf.head("6.0.20", 1, 2, None) + b"".join(recs[:3])
    data, starts, ends = place(recs)
    want = R.split(data, starts, ends)
    got = engine.rdbread_split_host(np.frombuffer(data, np.uint8), starts, ends, 9)
    for k in ("key_offsets", "pay_offsets", "types", "expires", "idle", "freq", "status"):
        assert np.array_equal(got[k], want[k]), k
    assert got["key_data"].tobytes() == b"".join(k for k in want["keys"] if k) and got["pay_data"].tobytes() == b"".join(p for p in want["pays"] if p)
    assert got["result"] == {"bytes": want["bytes"], "n_bad": 1, "status": 0}
    short = engine.rdbread_split_host(np.frombuffer(data, np.uint8), starts, ends, 9, key_cap=5, pay_cap=int(want["pay_offsets"][-1]))
    assert short["result"]["status"] == rf.E_CAPACITY and np.array_equal(short["key_offsets"], want["key_offsets"])
    with pytest.raises(rr.RRError):
        engine.rdbread_split_host(np.frombuffer(data, np.uint8), starts, ends, 10)                  # the version
    s = body + b"\xFF"
    s += struct.pack("<Q", rf.crc64(C1, s))
    assert engine.rdbread_verify_host(np.frombuffer(s, np.uint8), len(s) - 9, crc_in=C1) == (0, rf.crc64(C1, s[:-8]))
    assert engine.rdbread_verify_host(np.frombuffer(s, np.uint8), len(s) - 9)[0] == rr.RDBDUMP_E_CRC


# ---- stream positions past 4 GiB ------------------------------------------------------------------------------
def test_records_on_both_sides_of_4gib(engine):
    """A buffer a little over 4 GiB; only the records' bytes are written, a few in front of offset
    2^32, one across it, a few behind."""
    room = (1 << 32) + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < room + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the buffer needs {room >> 20} MiB")
    try:
        big = torch.empty(room, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:
        pytest.skip(f"the allocation failed: {e}")
    recs = [rec(0, R.raw(rand(10 + i)), rand(100 + 37 * i), b"\xFC" + struct.pack("<q", i)) for i in range(4)]
    recs += [rec(0, lz(rand(30) * 3), rand(5000)), rec(0, R.int_string(123456), rand(2 * STEP + 3))]
    recs += [rec(2, R.raw(rand(300)), rand(77)) for _ in range(3)]
    data, starts, ends = place(recs, [3] * len(recs))
    base = (1 << 32) - int(starts[4]) - 2000                  # record 4 lies across 2^32
    assert base + int(ends[3]) < 1 << 32 < base + int(ends[4]) and base + int(starts[5]) > 1 << 32
    big[base:base + len(data)] = _dev(np.frombuffer(data, np.uint8))
    want = R.split(data, starts, ends)
    run_split(engine, data, starts, ends, d_data=big, shift=base, want=want)
    assert (want["status"] == 0).all()
    del big
    torch.cuda.empty_cache()


# ---- the checksum's verdict ------------------------------------------------------------------------------------
def big_stream(crc_in=0, nbytes=3 * PIECE + 777):
    body = rf.head("6.0.20", 1, 2, None) + rf.selectdb(0, 1, 0) + rec(0, R.raw(b"big"), R.raw(rand(nbytes))) + b"\xFF"
    return body + struct.pack("<Q", rf.crc64(crc_in, body))


def test_verify_verdicts(engine):
    s = big_stream()
    eof = len(s) - 9
    want = rf.crc64(0, s[:eof + 1])
    d = _dev(np.frombuffer(s, np.uint8))
    assert run_verify(engine, d, eof) == (0, want)
    for at in (3, PIECE + 100, eof // 2, eof - 5, eof):                       # the first, a middle and the last piece
        bad = bytearray(s)
        bad[at] ^= 0x10
        st, crc = run_verify(engine, _dev(np.frombuffer(bytes(bad), np.uint8)), eof)
        assert st == rr.RDBDUMP_E_CRC and crc == rf.crc64(0, bytes(bad[:eof + 1])) != want
    for bit in (0, 63):                                                       # the stored value itself
        bad = bytearray(s)
        bad[eof + 1 + bit // 8] ^= 1 << (bit % 8)
        assert run_verify(engine, _dev(np.frombuffer(bytes(bad), np.uint8)), eof) == (rr.RDBDUMP_E_CRC, want)
    zero = s[:eof + 1] + bytes(8)                                             # saved with checksum disabled
    assert run_verify(engine, _dev(np.frombuffer(zero, np.uint8)), eof) == (rr.RDBREAD_NO_CKSUM, want)
    assert run_verify(engine, d, eof, crc_in=C1) == (rr.RDBDUMP_E_CRC, rf.crc64(C1, s[:eof + 1]))


def test_verify_short_streams(engine):
    for s in (b"REDIS0009\xFF", rf.head("6.0.20", 1, 2, None) + b"\xFF"):
        assert len(s) < RUN
        s += struct.pack("<Q", rf.crc64(0, s))
        for mis in (0, 1, 5):
            d = _dev(np.frombuffer(bytes(mis) + s, np.uint8))[mis:]
            assert run_verify(engine, d, len(s) - 9) == (0, rf.crc64(0, s[:-8]))
    with pytest.raises(rr.RRError):
        run_verify(engine, _dev(np.frombuffer(s, np.uint8)), len(s) - 8)      # no 8 bytes behind eof_at


def test_verify_chained_over_a_cut_stream(engine):
    """The stream uploaded in two parts, cut at no piece boundary, a nonzero state coming in."""
    s = big_stream(crc_in=C1)
    eof = len(s) - 9
    cut = PIECE + RUN + 13
    a, b = _dev(np.frombuffer(s[:cut], np.uint8)), _dev(np.frombuffer(s[cut:], np.uint8))
    state = torch.from_numpy(np.array([C1, 0], np.uint64).view(np.int64).copy()).cuda()
    res = torch.full((24,), CANARY, dtype=torch.uint8, device="cuda")
    engine.crc64_device(a, cut, state)
    engine.rdbread_verify(b, eof - cut, state, res)
    torch.cuda.synchronize()
    want = rf.crc64(C1, s[:eof + 1])
    assert int(state.cpu().numpy().view(np.uint64)[0]) == want == struct.unpack("<Q", s[-8:])[0]
    assert struct.unpack("<QQI", res.cpu().numpy()[:20].tobytes()) == (eof - cut + 9, 0, 0)


# ---- the chain a loader runs ------------------------------------------------------------------------------------
def test_chain_equals_the_loader_on_the_original_payloads(engine):
    n = 400
    data, offs = rr.gen_batch(4, n, seed=4242)
    v, e, a = rr.host_decode(data, offs)[:3]
    types, pdata, poffs, pst, _ = engine.rdbsave_host(v, e, a)
    good = np.nonzero(pst == 0)[0]
    assert len(good) > 300
    keys = [b"chain:%d" % i for i in range(n)]
    hd = rf.head("6.0.20", 1700000000, 1 << 33, None) + rf.selectdb(0, n, 0)
    sec, ro, rs, crc, res = engine.rdbfile_section_host(pdata, poffs, types, pst, *pk(keys), head=hd, flags=rr.RDBFILE_EOF)
    ix = rr.rdbread_index(sec)
    assert ix["rc"] == rr.RDBREAD_DONE and len(ix["rec_start"]) == len(good)
    assert engine.rdbread_verify_host(sec, ix["eof_at"]) == (0, crc)
    sp = engine.rdbread_split_host(sec, ix["rec_start"], ix["rec_end"], ix["state"].version)
    assert (sp["status"] == 0).all() and np.array_equal(sp["types"], types[good])
    assert sp["key_data"].tobytes() == b"".join(keys[i] for i in good)
    orig = [bytes(pdata[int(poffs[i]):int(poffs[i + 1])]) for i in good]
    od, oo = ld.pack(orig)
    assert sp["pay_data"].tobytes() == od.tobytes() and np.array_equal(sp["pay_offsets"], oo)
    opts = ld.c_opts(ld.options(set_max_intset_entries=0, hash_max_ziplist_entries=0, zset_max_ziplist_entries=0))
    l1 = engine.rdbload_host(sp["pay_data"], sp["pay_offsets"], sp["types"], opts)
    l0 = engine.rdbload_host(od, oo, types[good], opts)
    for x, y in zip(l1[:3], l0[:3]):
        assert np.array_equal(x, y)
    assert l1[3] == l0[3] and (l1[2] == ld.E_CONVERT).any() and (l1[2] == 0).any()
    c1 = engine.rdbconvert_host(sp["pay_data"], sp["pay_offsets"], sp["types"], l1[2], opts)
    c0 = engine.rdbconvert_host(od, oo, types[good], l0[2], opts)
    for x, y in zip(c1[:4], c0[:4]):
        assert np.array_equal(x, y)
    assert c1[4] == c0[4]
