"""rr_rdbfile_section, rr_crc64_device, rr_rdbdump_batch and rr_rdbdump_verify_batch on the GPU
against tests/rdbfile_reference.py: every byte, offset, status, total and checksum, with a canary
behind every buffer a call writes.  The sizes come from the kernels' exported shape: R bytes a lane,
P bytes a wave and step, one grid stride of pieces or values.  Data is random and the incoming
checksum nonzero wherever a shift is under test: a wrong shift is invisible on zeros."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import rdbfile_reference as rf
import rdbload_reference as ld
from helpers import batch_from_blobs, golden

pytestmark = pytest.mark.gpu

CANARY = 0xA5
R, P = rr.CRC64_RUN, rr.CRC64_PIECE
STRIDE = rr.CRC64_MAX_WAVES * P
C1 = 0x8F3B5D7A1C2E4F60          # a nonzero incoming checksum
RNG = np.random.default_rng(20261020)
rand = lambda n: RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def _dev(a, dtype=np.uint8):
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda() if a.size else torch.zeros(0, dtype=torch.uint8, device="cuda")


def pack(xs):
    offs = np.zeros(len(xs) + 1, np.uint64)
    if len(xs):
        np.cumsum([len(x) for x in xs], out=offs[1:])
    return np.frombuffer(b"".join(xs), np.uint8), offs


class Batch:
    def __init__(self, pays, keys, types=None, status=None, expires=None, idle=None, freq=None, key_offs=None):
        n = len(pays)
        self.n = n
        self.pay_data, self.pay_offs = pack(pays)
        if key_offs is None:
            self.key_data, self.key_offs = pack(keys)
        else:
            self.key_data, self.key_offs = np.frombuffer(bytes(keys), np.uint8), np.asarray(key_offs, np.uint64)
        self.types = np.asarray(types if types is not None else [0] * n, np.uint8)
        self.status = np.asarray(status if status is not None else [0] * n, np.uint8)
        self.expires = None if expires is None else np.asarray(expires, np.int64)
        self.idle = None if idle is None else np.asarray(idle, np.uint64)
        self.freq = None if freq is None else np.asarray(freq, np.uint8)

    def want(self, head, flags, crc_in, out_cap=None):
        return rf.section(self.pay_data, self.pay_offs, self.types, self.status, self.key_data, self.key_offs, self.expires,
                          self.idle, self.freq, head, flags, crc_in, out_cap=out_cap)

    def device(self):
        t = lambda a, dt: None if a is None else _dev(a, dt)
        return dict(pay_data=_dev(self.pay_data), pay_offsets=_dev(self.pay_offs, np.uint64), types=_dev(self.types),
                    status=_dev(self.status), key_data=_dev(self.key_data), key_offsets=_dev(self.key_offs, np.uint64),
                    expires=t(self.expires, np.int64), idle=t(self.idle, np.uint64), freq=t(self.freq, np.uint8))


def section_buffers(n, cap, crc_in):
    room = cap + 64
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    ro = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    rs = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    state = torch.from_numpy(np.array([crc_in, 0x1111, 0x2222, 0x3333], np.uint64).view(np.int64).copy()).cuda()
    res = torch.full((24 + 8,), CANARY, dtype=torch.uint8, device="cuda")
    return out, ro, rs, state, res


def compare_section(bufs, n, want, cap, crc_in):
    out, ro, rs, state, res = bufs
    got_ro = ro.cpu().numpy()
    assert np.array_equal(got_ro[:n + 1].view(np.uint64), want["rec_offsets"]) and (got_ro[n + 1:] == 7).all()
    got_rs = rs.cpu().numpy()
    assert np.array_equal(got_rs[:n], want["rec_status"]) and (got_rs[n:] == CANARY).all()
    st = state.cpu().numpy().view(np.uint64)
    assert (int(st[0]), int(st[1])) == (want["crc"], want["bytes"]), (hex(int(st[0])), hex(want["crc"]), int(st[1]), want["bytes"])
    assert st[2] == 0x2222 and st[3] == 0x3333
    r = res.cpu().numpy()
    assert (r[24:] == CANARY).all()
    nbytes, n_bad, status = struct.unpack("<QQI", r[:20].tobytes())
    assert (nbytes, n_bad, status) == (want["bytes"], want["n_bad"], want["status"])
    exp = np.full(cap + 64, CANARY, np.uint8)
    if want["data"] is not None:
        exp[:len(want["data"])] = np.frombuffer(want["data"], np.uint8)
    else:
        assert int(st[0]) == crc_in
    got = out.cpu().numpy()
    if not np.array_equal(got, exp):
        at = int(np.nonzero(got != exp)[0][0])
        raise AssertionError(f"section byte {at} of {want['bytes']}: got {got[at]:#x}, want {exp[at]:#x}")


def check_section(engine, B, head=b"", flags=0, crc_in=0, slack=40, stream=None, dev=None, want=None):
    """The device call on canary-filled buffers against the reference; out_cap = the bytes needed + slack
    (slack -1: one byte short)."""
    if want is None:
        full = B.want(head, flags, crc_in)
        want = full if slack >= 0 else B.want(head, flags, crc_in, out_cap=full["bytes"] + slack)
    cap = want["bytes"] + slack
    bufs = section_buffers(B.n, max(cap, 0), crc_in)
    dev = dev or B.device()
    engine.rdbfile_section(out=bufs[0], rec_offsets=bufs[1][:B.n + 1], rec_status=bufs[2][:B.n], state=bufs[3][:2], result=bufs[4][:24],
                           head=_dev(np.frombuffer(head, np.uint8)) if head else None, flags=flags, stream=stream, out_cap=max(cap, 0),
                           **dev)
    torch.cuda.synchronize()
    compare_section(bufs, B.n, want, max(cap, 0), crc_in)
    return want


# ---- keys, expiries, idle and freq ----------------------------------------------------------------
KEYS = [b"", b"0", b"-1", b"127", b"128", b"-128", b"-129", b"32767", b"32768", b"2147483647", b"2147483648", b"-2147483648",
        b"007", b"-0", b" 1", b"1 ", b"123456789012"] + [rand(k) for k in (63, 64, 16383, 16384, 70000)]


def key_form_batch():
    n = len(KEYS)
    pays = [rand(int(k)) for k in RNG.integers(0, 90, n)]
    return Batch(pays, KEYS, types=RNG.integers(0, 15, n))


def test_key_forms(engine):
    B = key_form_batch()
    want = check_section(engine, B, flags=rr.RDBFILE_EOF, crc_in=C1)
    sizes = np.diff(want["rec_offsets"].astype(np.int64)) - np.diff(B.pay_offs.astype(np.int64)) - 1   # the keys' encoded sizes
    #            ""  0  -1 127 128 -128 -129 32767 32768 2^31-1 2^31 -2^31 007 -0 " 1" "1 " 12 digits, then raw lengths
    assert sizes.tolist() == [1, 2, 2, 2, 3, 2, 3, 3, 5, 5, 11, 5, 4, 3, 3, 3, 13, 64, 66, 16385, 16389, 70005]


def test_expiries(engine):
    ex = [-1, 0, 1, -2, -(1 << 63), (1 << 63) - 1, -1, 5]
    n = len(ex)
    pays, keys = [rand(5 + i) for i in range(n)], [b"key%d" % i for i in range(n)]
    want = check_section(engine, Batch(pays, keys, expires=ex), crc_in=C1)
    assert want["data"][0] != 0xFC and b"\xFC" + struct.pack("<q", -2) in want["data"]
    check_section(engine, Batch(pays, keys, expires=None), crc_in=C1)          # NULL: none for every key


@pytest.mark.parametrize("flags", [0, rr.RDBFILE_IDLE, rr.RDBFILE_FREQ, rr.RDBFILE_IDLE | rr.RDBFILE_FREQ])
def test_idle_and_freq(engine, flags):
    idle = [0, 63, 64, 16383, 16384, (1 << 32) - 1, 1 << 32, 1 << 63]
    n = len(idle)
    B = Batch([rand(3 + i) for i in range(n)], [b"k%d" % i for i in range(n)], idle=idle, freq=[0, 255] * (n // 2),
              expires=[-1, 77] * (n // 2))
    want = check_section(engine, B, flags=flags, crc_in=C1)
    if flags & rr.RDBFILE_IDLE:
        assert b"\xF8\x81" + struct.pack(">Q", 1 << 63) in want["data"]         # the 9-byte form


# ---- section sizes -----------------------------------------------------------------------------------
def sized(total, head_bytes=0):
    """(batch, head) of a section of exactly `total` bytes without EOF."""
    if total >= head_bytes + 2:
        return Batch([rand(total - head_bytes - 2)], [b""]), rand(head_bytes)   # type | 0x00 | payload
    return Batch([], []), rand(total)


@pytest.mark.parametrize("total", [0, 1, R - 1, R, R + 1, P - 1, P, P + 1, 2 * P + R + 1])
def test_section_sizes(engine, total):
    B, head = sized(total, 3 if total > 8 else 0)
    for crc_in in (0, C1):
        want = check_section(engine, B, head, 0, crc_in)
        assert want["bytes"] == total
    if total == 0:
        assert want["crc"] == C1


def test_one_grid_stride_plus_a_piece_plus_one(engine):
    total = STRIDE + P + 1
    head = rand(5)
    len0 = total // 2
    len1 = total - len(head) - (1 + 9 + len0) - (9 + 1 + 10)                   # type, key; expire, type, key
    B = Batch([rand(len0), rand(len1)], [b"left:key", b"right:key"], expires=[-1, 1700000000000])
    w0 = B.want(head, 0, 0)
    assert w0["bytes"] == total
    dev = B.device()
    check_section(engine, B, head, 0, 0, dev=dev, want=w0)
    w1 = dict(w0, crc=w0["crc"] ^ rf.shift(C1, total))                          # crc(c, B) = crc(0, B) ^ shift(c, |B|)
    check_section(engine, B, head, 0, C1, dev=dev, want=w1)


@pytest.mark.parametrize("head_bytes", range(18))
def test_head_alignments(engine, head_bytes):
    """Records, and the copies inside them, start at every alignment."""
    n = 6
    B = Batch([rand(40 + 17 * i) for i in range(n)], [rand(3 + 5 * i) for i in range(n)], expires=[-1, 9] * 3)
    check_section(engine, B, rand(head_bytes), rr.RDBFILE_EOF, C1)


def test_only_head_and_eof(engine):
    hd = rf.head("6.0.20", 1700000000, 12345, None) + rf.selectdb(0, 0, 0)
    want = check_section(engine, Batch([], []), hd, rr.RDBFILE_EOF, 0)
    p = rf.parse(want["data"])
    assert p["cksum_ok"] and p["records"] == [] and len(p["aux"]) == 5


# ---- chaining, determinism, streams ---------------------------------------------------------------
def test_chained_sections_equal_one(engine):
    n = 30
    pays = [rf.ref.save_raw_string(rand(int(k))) for k in RNG.integers(0, 3000, n)]   # Strings: the parser walks them
    keys = [b"chain:%d" % i for i in range(n)]
    ex = [(-1 if i % 3 else 1000 + i) for i in range(n)]
    hd = rf.head("6.0.20", 1, 2, None) + rf.selectdb(3, n, 10)
    whole = Batch(pays, keys, expires=ex).want(hd, rr.RDBFILE_EOF, 0)
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = b""
    for lo, hi, h, fl in ((0, 11, hd, 0), (11, 12, b"", 0), (12, n, b"", rr.RDBFILE_EOF)):
        B = Batch(pays[lo:hi], keys[lo:hi], expires=ex[lo:hi])
        cap = rr.rdbfile_bound(B.n, B.key_data.size, B.pay_data.size, len(h))
        out, ro, rs, _, res = section_buffers(B.n, cap, 0)
        engine.rdbfile_section(out=out[:cap], rec_offsets=ro[:B.n + 1], rec_status=rs[:B.n], state=state, result=res[:24],
                               head=_dev(np.frombuffer(h, np.uint8)) if h else None, flags=fl, **B.device())
        torch.cuda.synchronize()                                                # (only to read the section's size)
        got += out[:int(state[1].item())].cpu().numpy().tobytes()
    assert got == whole["data"] and int(state.cpu().numpy().view(np.uint64)[0]) == whole["crc"]
    assert rf.parse(got)["cksum_ok"]


def test_deterministic_across_runs_and_streams(engine):
    B = key_form_batch()
    hd = rand(13)
    want = B.want(hd, rr.RDBFILE_EOF, C1)
    dev = B.device()
    for stream in (None, torch.cuda.Stream(), torch.cuda.Stream()):
        for _ in range(2):
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
            check_section(engine, B, hd, rr.RDBFILE_EOF, C1, stream=stream, dev=dev, want=want)


def test_eof_and_no_checksum(engine):
    B = Batch([rf.ref.save_raw_string(b"value-%d" % i) for i in range(20)], [b"key:%d" % i for i in range(20)])
    hd = rf.head("6.0.20", 1700000000, 99999, (0, "f" * 40, 12)) + rf.selectdb(0, 20, 0)
    want = check_section(engine, B, hd, rr.RDBFILE_EOF, 0)
    p = rf.parse(want["data"])
    assert p["cksum_ok"] and [r[1] for r in p["records"]] == [b"key:%d" % i for i in range(20)]
    assert [r[6] for r in p["records"]] == [rf.ref.save_raw_string(b"value-%d" % i) for i in range(20)]
    nock = check_section(engine, B, hd, rr.RDBFILE_EOF | rr.RDBFILE_NO_CKSUM, 0)
    assert nock["data"][-9:] == b"\xFF" + bytes(8) and nock["crc"] == 0
    kept = check_section(engine, B, hd, rr.RDBFILE_EOF | rr.RDBFILE_NO_CKSUM, C1)
    assert kept["crc"] == C1 and kept["data"][-8:] == struct.pack("<Q", C1)


# ---- skips and capacity ------------------------------------------------------------------------------
def test_skips(engine):
    kd = rand(64)
    koffs = [0, 10, 4, 20, 100, 30, 64, 64]       # ok, reversed, ok, past the cap, reversed, ok to the last byte, empty
    n = len(koffs) - 1
    pays = [rand(20 + 11 * i) for i in range(n)]
    B = Batch(pays, kd, status=[0, 0, 12, 0, 0, 0, 0], key_offs=koffs, expires=[5] * n)
    want = check_section(engine, B, b"HD", rr.RDBFILE_EOF, C1)
    assert want["rec_status"].tolist() == [0, rr.RDBFILE_E_KEY, rr.RDBFILE_E_VALUE, rr.RDBFILE_E_KEY, rr.RDBFILE_E_KEY, 0, 0]
    assert want["n_bad"] == 4 and np.diff(want["rec_offsets"].astype(np.int64))[[1, 2, 3, 4]].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("flags", [0, rr.RDBFILE_EOF])
def test_capacity(engine, flags):
    B = key_form_batch()
    short = check_section(engine, B, b"head", flags, C1, slack=-1)              # one byte short: nothing written
    assert short["status"] == rf.E_CAPACITY and short["data"] is None and short["crc"] == C1
    exact = check_section(engine, B, b"head", flags, C1, slack=0)
    assert exact["status"] == 0 and exact["bytes"] == short["bytes"]


# ---- the CRC pass alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, R + 1, P + 1, 3 * P + 5])
def test_crc64_device(engine, n):
    d = rand(n + 3)
    t = _dev(np.frombuffer(d, np.uint8))
    for mis in (0, 3):
        state = torch.from_numpy(np.array([C1, 0, 0x77], np.uint64).view(np.int64).copy()).cuda()
        engine.crc64_device(t[mis:], n, state[:2])
        st = state.cpu().numpy().view(np.uint64)
        assert (int(st[0]), int(st[1]), int(st[2])) == (rf.crc64(C1, d[mis:mis + n]), n, 0x77)


# ---- DUMP payloads -----------------------------------------------------------------------------------------
def run_dump(engine, pays, types, status, short=0):
    data, offs = pack(pays)
    n = len(pays)
    vals, woffs, wst, wbad = rf.dump_batch(data, offs, types, status)
    total = int(woffs[-1])
    cap = total - short
    if short:
        vals, woffs, wst, wbad = rf.dump_batch(data, offs, types, status, out_cap=cap)
    out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    oo = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    os_ = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((24 + 8,), CANARY, dtype=torch.uint8, device="cuda")
    engine.rdbdump(_dev(data), _dev(offs, np.uint64), _dev(np.asarray(types, np.uint8)), _dev(np.asarray(status, np.uint8)),
                   out, oo[:n + 1], os_[:n], res[:24], out_cap=cap)
    torch.cuda.synchronize()
    got_oo = oo.cpu().numpy()
    assert np.array_equal(got_oo[:n + 1].view(np.uint64), woffs) and (got_oo[n + 1:] == 7).all()
    got_st = os_.cpu().numpy()
    assert np.array_equal(got_st[:n], wst) and (got_st[n:] == CANARY).all()
    r = res.cpu().numpy()
    assert struct.unpack("<QQI", r[:20].tobytes()) == (total, wbad, 0) and (r[24:] == CANARY).all()
    exp = np.full(total + 64, CANARY, np.uint8)
    for v, o in zip(vals, woffs):
        if v is not None:
            exp[int(o):int(o) + len(v)] = np.frombuffer(v, np.uint8)
    got = out.cpu().numpy()
    if not np.array_equal(got, exp):
        at = int(np.nonzero(got != exp)[0][0])
        raise AssertionError(f"DUMP byte {at} (value {int(np.searchsorted(woffs, at, side='right')) - 1}): got {got[at]:#x}, want {exp[at]:#x}")
    return vals, woffs, wst


DUMP_SIZES = [0, 1, R - 1, R, R + 1, P - 2, P - 1, P, P + 1, 3 * P + 5]


def test_dump_sizes(engine):
    pays = [rand(k) for k in DUMP_SIZES] + [rand(9), rand(300)]
    n = len(pays)
    status = [0] * n
    status[3], status[n - 2] = 12, 1                                            # unsaveable values among them
    _, _, st = run_dump(engine, pays, RNG.integers(0, 15, n), status)
    assert st.tolist().count(rr.RDBFILE_E_VALUE) == 2
    _, _, st = run_dump(engine, pays, RNG.integers(0, 15, n), status, short=1)  # the last value one byte short
    assert st[-1] == rf.E_CAPACITY and (st[:-2] != rf.E_CAPACITY).all()
    assert rf.dump(0, b"\x01a") == bytes.fromhex("00016109006f0cbe57dbb01e05")
    vals, _, _ = run_dump(engine, [b"\x01a"], [0], [0])
    assert vals == [bytes.fromhex("00016109006f0cbe57dbb01e05")]


def test_dump_one_grid_stride_plus_one(engine):
    n = rr.RDBDUMP_MAX_WAVES + 1
    pays = [rand(int(k)) for k in RNG.integers(0, 4, n)]
    run_dump(engine, pays, RNG.integers(0, 15, n), [0] * n)


def run_verify(engine, dumps, cap=None):
    data, offs = pack(dumps)
    n = len(dumps)
    want = [rf.dump_verify(d) for d in dumps]
    woffs = np.zeros(n + 1, np.uint64)
    np.cumsum([len(w[2]) if w[0] == 0 else 0 for w in want], out=woffs[1:])
    total = int(woffs[-1])
    cap = total if cap is None else cap
    out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    oo = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    ty = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((24 + 8,), CANARY, dtype=torch.uint8, device="cuda")
    engine.rdbdump_verify(_dev(data), _dev(offs, np.uint64), out[:cap], oo[:n + 1], ty[:n], st[:n], res[:24])
    torch.cuda.synchronize()
    got_oo = oo.cpu().numpy()
    assert np.array_equal(got_oo[:n + 1].view(np.uint64), woffs) and (got_oo[n + 1:] == 7).all()
    wst = np.array([w[0] for w in want], np.uint8)
    exp = np.full(total + 64, CANARY, np.uint8)
    for i, w in enumerate(want):
        if w[0] == 0 and int(woffs[i + 1]) > cap:
            wst[i] = rf.E_CAPACITY
        elif w[0] == 0:
            exp[int(woffs[i]):int(woffs[i + 1])] = np.frombuffer(w[2], np.uint8)
    got_st, got_ty = st.cpu().numpy(), ty.cpu().numpy()
    assert np.array_equal(got_st[:n], wst) and (got_st[n:] == CANARY).all()
    assert got_ty[:n].tolist() == [w[1] for w in want] and (got_ty[n:] == CANARY).all()
    r = res.cpu().numpy()
    assert struct.unpack("<QQI", r[:20].tobytes()) == (total, int((wst != 0).sum()), 0) and (r[24:] == CANARY).all()
    assert np.array_equal(out.cpu().numpy(), exp)
    return wst


def test_verify_reference_dumps(engine):
    dumps = [rf.dump(int(t), rand(k)) for k, t in zip(DUMP_SIZES, RNG.integers(0, 15, len(DUMP_SIZES)))]
    assert (run_verify(engine, dumps) == 0).all()
    st = run_verify(engine, dumps, cap=sum(DUMP_SIZES) - 1)                      # the last payload does not fit
    assert st[-1] == rf.E_CAPACITY and (st[:-1] == 0).all()


def test_verify_bit_flips_versions_and_lengths(engine):
    good = rf.dump(4, rand(300))
    L = len(good)
    dumps, exp = [good], [0]
    for at in [1, 150, L - 11] + list(range(L - 10, L)):                        # payload first / middle / last, footer, CRC
        for bit in range(8):
            d = bytearray(good)
            d[at] ^= 1 << bit
            dumps.append(bytes(d))
            ver = struct.unpack_from("<H", d, L - 10)[0]
            exp.append(rf.E_VERSION if ver > 9 else rf.E_CRC)
    for ver in (0, 9, 10):                                                      # a matching CRC under each version
        b = b"\x00" + rand(40) + struct.pack("<H", ver)
        dumps.append(b + struct.pack("<Q", rf.crc64(0, b)))
        exp.append(0 if ver <= 9 else rf.E_VERSION)
    for k in (0, 9, 10, 11):
        b = rand(k)
        if k == 11:
            b = b[:1] + struct.pack("<H", 9)
            b += struct.pack("<Q", rf.crc64(0, b))                              # the shortest valid one: an empty payload
        dumps.append(b)
        exp.append(0 if k == 11 else rf.E_SHORT)
    assert [rf.dump_verify(d)[0] for d in dumps] == exp
    assert run_verify(engine, dumps).tolist() == exp


# ---- end to end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lzf_flag", [False, True])
def test_end_to_end_golden(engine, lzf_flag):
    from test_gpu_rdbload import ZERO, models
    from test_rdbload import HASH, HZL, ISET, L as LIST, S, SET, ZSET, ZZL
    g = golden()
    blobs = [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]
    data, offs = batch_from_blobs(blobs)
    v1, e1, a1, _ = engine.decode_host(data, offs)
    first = models(v1, e1, a1)
    types, pdata, poffs, pst, _ = engine.rdbsave_host(v1, e1, a1, lzf=lzf_flag)
    n = len(types)
    keys = [b"key:%d" % i if i % 4 else str(1000 * i - 7).encode() for i in range(n)]
    expires = [-1 if i % 2 else 1700000000000 + i for i in range(n)]
    B = Batch([bytes(pdata[int(poffs[i]):int(poffs[i + 1])]) for i in range(n)], keys, types=types, status=pst, expires=expires)
    hd = rf.head("6.0.20", 1700000000, 1 << 33, (0, "a" * 40, 1)) + rf.selectdb(0, n, n // 2)
    want = check_section(engine, B, hd, rr.RDBFILE_EOF, 0)
    p = rf.parse(want["data"])
    good = [i for i in range(n) if pst[i] == 0]
    assert p["cksum_ok"] and len(p["records"]) == len(good) and len(good) > 20
    assert [(r[1], r[2], r[5]) for r in p["records"]] == [(keys[i], expires[i], int(types[i])) for i in good]
    big = ld.options(set_max_intset_entries=32767, hash_max_ziplist_entries=32767, zset_max_ziplist_entries=32767)
    rec = {i: r for i, r in zip(good, p["records"])}
    n_checked = 0
    for opts, kinds in ((big, (S, LIST, ISET, HZL, ZZL)), (ZERO, (SET, HASH, ZSET))):
        sel = [i for i in good if types[i] in kinds and not (types[i] in (SET, HASH, ZSET) and int(v1["n_elems"][i]) == 0)]
        ty = np.array([types[i] for i in sel], np.uint8)
        for source in ("stream", "dump"):
            if source == "stream":
                pays = [rec[i][6] for i in sel]
            else:                                                               # DUMP -> verify -> the same payloads
                dd, do, ds, dr = engine.rdbdump_host(*pack([rec[i][6] for i in sel]), ty, np.zeros(len(sel), np.uint8))
                assert (ds == 0).all() and dr["n_bad"] == 0
                vd, vo, vt, vs, vr = engine.rdbdump_verify_host(dd, do)
                assert (vs == 0).all() and np.array_equal(vt, ty)
                pays = [bytes(vd[int(vo[k]):int(vo[k + 1])]) for k in range(len(sel))]
                assert pays == [rec[i][6] for i in sel]
            bdata, boffs, bst, _ = engine.rdbload_host(*ld.pack(pays), ty, ld.c_opts(opts))
            assert (bst == 0).all()
            pad = np.zeros((len(bdata) + 15) & ~15, np.uint8)
            pad[:len(bdata)] = bdata
            second = models(*engine.decode_host(pad, boffs)[:3])
            assert second == [first[i] for i in sel] and None not in second
        n_checked += len(sel)
    assert n_checked > 20


# ---- the host entry points -------------------------------------------------------------------------------
def test_host_entry_points(engine):
    B = key_form_batch()
    hd = rand(7)
    want = B.want(hd, rr.RDBFILE_EOF, C1)
    data, ro, rs, crc, res = engine.rdbfile_section_host(B.pay_data, B.pay_offs, B.types, B.status, B.key_data, B.key_offs,
                                                         head=hd, flags=rr.RDBFILE_EOF, crc_in=C1)
    assert data.tobytes() == want["data"] and np.array_equal(ro, want["rec_offsets"]) and np.array_equal(rs, want["rec_status"])
    assert crc == want["crc"] and res == {"bytes": want["bytes"], "n_bad": 0, "status": 0}
    data, ro, rs, crc, res = engine.rdbfile_section_host(B.pay_data, B.pay_offs, B.types, B.status, B.key_data, B.key_offs,
                                                         head=hd, flags=rr.RDBFILE_EOF, crc_in=C1, out_cap=want["bytes"] - 1)
    assert res == {"bytes": want["bytes"], "n_bad": 0, "status": rf.E_CAPACITY} and crc == C1 and data.size == 0
    status = np.zeros(B.n, np.uint8)
    status[2] = 12
    vals, woffs, wst, wbad = rf.dump_batch(B.pay_data, B.pay_offs, B.types, status)
    dd, do, ds, dr = engine.rdbdump_host(B.pay_data, B.pay_offs, B.types, status)
    assert dd.tobytes() == b"".join(v for v in vals if v is not None) and np.array_equal(do, woffs) and np.array_equal(ds, wst)
    assert dr == {"bytes": int(woffs[-1]), "n_bad": wbad, "status": 0}
    vd, vo, vt, vs, vr = engine.rdbdump_verify_host(dd, do)
    assert vs.tolist() == [rf.E_SHORT if i == 2 else 0 for i in range(B.n)] and vr["n_bad"] == 1
    assert vd.tobytes() == b"".join(bytes(B.pay_data[int(B.pay_offs[i]):int(B.pay_offs[i + 1])]) for i in range(B.n) if i != 2)


# ---- graph capture -------------------------------------------------------------------------------------------
def test_graph_capture_save_then_section():
    eng = rr.Engine(0)
    try:
        n = 3000
        data, offs = rr.gen_batch(4, n, seed=777)
        v, e, a = rr.host_decode(data, offs)[:3]
        types, pdata, poffs, pst, _ = eng.rdbsave_host(v, e, a)
        keys = [b"graph:key:%d" % i for i in range(n)]
        B = Batch([bytes(pdata[int(poffs[i]):int(poffs[i + 1])]) for i in range(n)], keys, types=types, status=pst)
        want = B.want(b"HEAD", rr.RDBFILE_EOF, C1)
        d_v, d_e, d_a = _dev(v.view(np.uint8)), _dev(e.view(np.uint8)), _dev(a)
        cap = int(rr.rdbsave_bound(v, e)) + 16
        pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        p_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        p_ty, p_st = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        kd, ko = _dev(B.key_data), _dev(B.key_offs, np.uint64)
        head = _dev(np.frombuffer(b"HEAD", np.uint8))
        scap = want["bytes"] + 32
        bufs = section_buffers(n, scap, C1)

        def chain(stream):
            eng.rdbsave_device(d_v, d_e, d_a, pay, p_off, p_ty, p_st, tot, stream=stream)
            eng.rdbfile_section(pay, p_off, p_ty, p_st, kd, ko, bufs[0], bufs[1][:n + 1], bufs[2][:n], bufs[3][:2], bufs[4][:24],
                                head=head, flags=rr.RDBFILE_EOF, stream=stream, out_cap=scap)

        def reset():
            fresh = section_buffers(n, scap, C1)
            for dst, src in zip(bufs, fresh):
                dst.copy_(src)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain(s)                                                            # the warm call: scratch is sized
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        compare_section(bufs, n, want, scap, C1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                               # one stream, the launches in a line
            chain(torch.cuda.current_stream())
        for _ in range(2):
            reset()
            g.replay()
            torch.cuda.synchronize()
            compare_section(bufs, n, want, scap, C1)
    finally:
        eng.close()
