"""rr_d2string_batch and rr_rdbzset_batch on the GPU, byte-exact against tests/rdbzset_reference.py: every
text and length with the rest of each slot untouched, every status, offset, blob byte and total with a
canary behind every buffer the calls write.  The convert_status a batch is given comes from a real
rr_rdbconvert_batch call on the same input unless a test says otherwise.  The shapes are the smallest
that reach the kernels' paths: one wave's 64 scores and one past, the rank sort and the 64-rank text
rounds at 63 / 64 / 65 / 128 / 512 members, ties the members decide, the longest text, a 5-byte prevlen
in front of a printed score, every stay, capacity, a stream, and the chain from a written RDB stream
to decoded ZSets."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr
from oracle import cpu

import rdb_reference as ref
import rdbconvert_reference as cv
import rdbfile_reference as rf
import rdbload_reference as ld
import rdbzset_reference as zr
from flat_forge import Flat
from rdbload_mutants import lz
from test_rdbzset import ZSET, ZZL, dbl, literal_cases, raw, zset

pytestmark = pytest.mark.gpu

CANARY = 0xA5
S, L, SET, HASH, ISET = rr.T_STRING, rr.T_LIST_QUICKLIST, rr.T_SET_HT, rr.T_HASH_HT, rr.T_SET_INTSET
OPTS = ld.options(set_max_intset_entries=1000, zset_max_ziplist_entries=1000, zset_max_ziplist_value=300)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


# ---- rr_d2string_batch ------------------------------------------------------------------------------------
def expect_texts(bits):
    texts = [zr.d2string(int(b)) for b in bits.tolist()]
    want = np.full((len(bits), rr.D2STRING_SLOT), CANARY, np.uint8)
    for i, t in enumerate(texts):
        want[i, :len(t)] = np.frombuffer(t, np.uint8)
    return want, np.array([len(t) for t in texts], np.uint8)


def test_d2string_edge_list(engine):
    bits = zr.edge_scores()
    want, wlen = expect_texts(bits)
    text, ln = engine.d2string_host(bits, fill=CANARY)
    assert np.array_equal(ln, wlen) and int(ln.max()) == rr.D2STRING_MAX
    bad = np.nonzero((text != want).any(axis=1))[0]
    assert len(bad) == 0, (hex(int(bits[bad[0]])), text[bad[0]].tobytes(), want[bad[0]].tobytes())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_d2string_device_entry(engine, n):
    """The device entry on a side stream, canaries behind both outputs; n == 0 writes nothing."""
    rng = np.random.default_rng(n)
    edge = zr.edge_scores()
    bits = edge[rng.integers(0, len(edge), n)]
    want, wlen = expect_texts(bits)
    d_bits = torch.from_numpy(bits.view(np.int64).copy()).cuda()
    d_text = torch.full((32 * n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_len = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        engine.d2string(d_bits, d_text[:32 * n], d_len[:n], stream=st)
    torch.cuda.synchronize()
    text, ln = d_text.cpu().numpy(), d_len.cpu().numpy()
    assert np.array_equal(ln[:n], wlen) and (ln[n:] == CANARY).all()
    assert np.array_equal(text[:32 * n].reshape(n, 32), want) and (text[32 * n:] == CANARY).all()


# ---- rr_rdbzset_batch -------------------------------------------------------------------------------------
def run_device(engine, types, data, offsets, conv, opts, cap, room, stream=None):
    n = len(types)
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4 + 2,), -3, dtype=torch.int64, device="cuda")
    d_data = _dev(data) if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")   # exactly data_cap bytes
    d_in_off = torch.from_numpy(np.ascontiguousarray(offsets, np.uint64).view(np.int64).copy()).cuda()
    d_types = _dev(np.asarray(types, np.uint8)) if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_conv = _dev(np.asarray(conv, np.uint8)) if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    engine.rdbzset(d_data, d_in_off, d_types, d_conv, out[:cap], d_off[:n + 1], d_status[:n], d_tot[:4],
                   opts=ld.c_opts(opts) if opts else None, stream=stream)
    return out, d_off, d_status, d_tot


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


def check(engine, types, payloads, opts=None, data_cap=None, host=False, conv=None, stream=None):
    """The device call on canary-filled buffers against the reference; host: the host entry too.  conv None:
    what rr_rdbload_batch and then rr_rdbconvert_batch say about this input."""
    data, offsets = ld.pack(payloads)
    n = len(types)
    nt = np.asarray(types, np.uint8)
    co = ld.c_opts(opts) if opts else None
    if conv is None:
        lst = engine.rdbload_host(data, offsets, nt, co)[2]
        conv = engine.rdbconvert_host(data, offsets, nt, lst, co)[3]
    want = zr.zset_batch(types, data, offsets, conv, opts, data_cap)
    total = int(want[1][-1])
    cap = total + 40 if data_cap is None else data_cap
    room = max(cap, total) + 64
    if stream is not None:
        with torch.cuda.stream(stream):
            bufs = run_device(engine, types, data, offsets, conv, opts, cap, room, stream)
    else:
        bufs = run_device(engine, types, data, offsets, conv, opts, cap, room)
    torch.cuda.synchronize()
    compare(bufs, n, want, room)
    if host:
        hd, ho, hs, ht = engine.rdbzset_host(data, offsets, nt, conv, co, data_cap)
        assert np.array_equal(ho, want[1]) and np.array_equal(hs, want[2]) and ht == want[3]
        if data_cap is None:
            assert np.array_equal(hd, want[0])
    return conv, want[2], want[3]


FRAC = lambda k: (k * 37 % 101) / 8 + 0.0625 + (k % 7) * 1e-9 - 3.0   # never an integer


def zset_of(n, score=FRAC, member=lambda k: b"m%d" % k):
    return zset([(member(k), score(k)) for k in range(n)])


def mixed_batch():
    """About 300 (type, payload, what the third stage must say: 0, E_CONVERT or SKIP)."""
    rng = np.random.default_rng(12)
    edge = zr.edge_scores()
    edge = edge[(edge & np.uint64(0x7FFFFFFFFFFFFFFF)) <= np.uint64(0x7FF0000000000000)]   # no NaN
    pick = lambda: zr.to_double(int(edge[int(rng.integers(0, len(edge)))]))
    c = []
    for n in (1, 2, 63, 64, 65, 128):
        c.append((ZSET, zset_of(n), 0))
        c.append((ZSET, zset_of(n, lambda k: pick()), 0))
    c.append((ZSET, zset_of(512, lambda k: pick() if k % 3 else 2.5), 0))              # under zset_max_ziplist_entries >= 512
    c.append((ZSET, zset_of(513), zr.E_CONVERT))                                       # above RR_RDBCONVERT_MAX_N
    ties = [b"x" * 70 + b"y" * (k % 5) for k in range(10)] + [b"", b"x", b"xx", b"-12", b"7"]
    c.append((ZSET, zset([(m, 0.25) for m in ties] + [(b"\xC0", 0.25)]), 0))           # tied scores: lengths decide
    c.append((ZSET, b"\x03" + b"\xC0\x07" + dbl(0.25) + raw(b"7") + dbl(0.25) + b"\xC1\x00\x01" + dbl(0.25), 0))   # integer-form members
    c.append((ZSET, zset([(b"p", 5e-324), (b"z", 0.0), (b"n", -0.0), (b"a", -5e-324), (b"q", 0.0)]), 0))
    c.append((ZSET, zset([(b"L" * 64, -5e-324), (b"M" * 64, -2.2250738585072014e-308)]), 0))   # 24-byte texts behind 64-byte members
    c.append((ZSET, zset([(b"w" * 300, 1.5), (b"v" * 249, 2.5), (b"u" * 250, 0.1)]), 0))       # a 5-byte prevlen in front of a printed score
    c.append((ZSET, zset([(b"a", 2.0**52), (b"b", 2.0**53), (b"c", 1e16), (b"d", 1e17), (b"e", -2.0**52)]), 0))   # 0xE0 entries, and "1e+17"
    c.append((ZSET, zset([(b"a", 1.5), (b"m", float("nan"))]), zr.E_CONVERT))
    c.append((ZSET, zset([(b"m", zr.to_double(0xFFF0000000000001))]), zr.E_CONVERT))   # a NaN with the sign set
    c.append((ZSET, b"\x01" + lz(b"ab" * 18) + dbl(1.5), zr.E_CONVERT))                # an LZF member
    c.append((ZSET, zset([(b"w" * 301, 1.5)]), zr.SKIP))                               # thresholds not met: the loader's own, status 0
    c.append((ZSET, zset([(b"a", 1.5)])[:-3], zr.SKIP))                                # truncated: the loader's E_TRUNC
    c.append((ZSET, zset([(b"a", 17.0), (b"b", float("inf")), (b"c", -0.0)]), zr.SKIP))   # rr_rdbconvert_batch's own
    # values of every other type and status
    c.append((SET, b"\x02" + raw(b"3") + raw(b"1"), zr.SKIP))                           # converted by the second stage
    c.append((HASH, b"\x01" + raw(b"f") + raw(b"1.5"), zr.SKIP))
    c.append((SET, ref.save_len(513) + b"".join(raw(b"%d" % k) for k in range(513)), zr.SKIP))   # E_CONVERT there, not a ZSet
    c.append((ZZL, raw(cv.ziplist_of([b"a", b"1.5"] * 1001)), zr.SKIP))                 # a reverse conversion: E_CONVERT, type 12
    for t, p in ((S, raw(b"hello")), (S, b"\x05abc"), (L, b"\x00"), (1, b"\x00"), (ISET, raw(struct.pack("<II", 2, 0))), (255, b"")):
        c.append((t, p, zr.SKIP))
    while len(c) < 300:                                                                 # small ZSets between all of these
        k = len(c)
        c.insert(int(rng.integers(0, len(c))), (ZSET, zset_of(k % 9 + 1, lambda j: pick() if (j + k) % 2 else FRAC(j + k)), 0))
    # a ZSet whose picked scores all happen to print without %.17g is the second stage's
    c = [(t, p, zr.SKIP if t == ZSET and e == 0 and cv.convert_blob(t, p, OPTS)[0] == 0 else e) for t, p, e in c]
    assert sum(e == 0 for _, _, e in c) > 250
    return c


def test_mixed_batch(engine):
    cases = mixed_batch()
    types, pays = [c[0] for c in cases], [c[1] for c in cases]
    conv, st, tot = check(engine, types, pays, OPTS, host=True)
    assert st.tolist() == [c[2] for c in cases]
    nt = np.asarray(types)
    assert (st[conv == 0] == zr.SKIP).all() and (conv == 0).sum() >= 3            # what the second stage converted
    assert (st[(conv == zr.E_CONVERT) & (nt == ZSET)] != zr.SKIP).all()           # the ZSets it left: attempted
    assert (st[nt != ZSET] == zr.SKIP).all() and ((conv == zr.E_CONVERT) & (nt != ZSET)).sum() >= 2
    assert tot["n_bad"] == int((st == zr.E_CONVERT).sum()) == 4 and set(st.tolist()) == {0, zr.E_CONVERT, zr.SKIP}


def test_literals_and_claimed_status(engine):
    """The CPU file's literals, each under its options, and values claimed E_CONVERT that the loader would
    not have passed on: thresholds not met, malformed payloads, bad slices."""
    groups = {}
    for p, o, st, blob in literal_cases():
        groups.setdefault(tuple(sorted((o or ld.DEFAULTS).items())), []).append((p, st))
    for key, cases in groups.items():
        pays = [c[0] for c in cases]
        conv = np.full(len(pays), zr.E_CONVERT, np.uint8)
        _, st, _ = check(engine, [ZSET] * len(pays), pays, dict(key), conv=conv, host=True)
        assert st.tolist() == [c[1] for c in cases]
    good = zset([(b"a", 1.5)])
    cases = [good, zset([(b"w" * 301, 1.5)]), good, zset_of(3)[:-1], good, b"\x02" + raw(b"a") + dbl(1.5), good, b"", b"\x81" + b"\xFF" * 8,
             b"\x01\xC4\x00\x01a" + dbl(1.5), zset_of(1001), good]
    two = dict(OPTS)
    conv = np.full(len(cases), zr.E_CONVERT, np.uint8)
    _, st, tot = check(engine, [ZSET] * len(cases), cases, two, conv=conv)
    want = [0 if c is good else zr.E_CONVERT for c in cases]
    assert st.tolist() == want and tot["n_bad"] == want.count(zr.E_CONVERT)
    data, offs = ld.pack(cases)                                          # bad slices: reversed, and past data_cap
    offs2 = offs.copy()
    offs2[2], offs2[-1] = offs[1] - 1, offs[-1] + 5
    w = zr.zset_batch([ZSET] * len(cases), data, offs2, conv, two)
    room = int(w[1][-1]) + 64
    bufs = run_device(engine, [ZSET] * len(cases), data, offs2, conv, two, room - 24, room)
    torch.cuda.synchronize()
    compare(bufs, len(cases), w, room)
    assert w[2][1] == zr.E_CONVERT and w[2][-1] == zr.E_CONVERT


def test_integer_scores_give_the_second_stage_bytes(engine):
    pays = [zset_of(n, lambda k: float((k * 7) % 50 - 25)) for n in (1, 5, 64, 100)]
    pays.append(zset([(b"a", float("inf")), (b"b", -0.0), (b"c", float(2**52 - 1)), (b"d", float("-inf"))]))
    data, offsets = ld.pack(pays)
    nt = np.full(len(pays), ZSET, np.uint8)
    claim = np.full(len(pays), zr.E_CONVERT, np.uint8)
    cd, co, cot, cst, ctot = engine.rdbconvert_host(data, offsets, nt, claim)
    zd, zo, zst, ztot = engine.rdbzset_host(data, offsets, nt, claim)
    assert (cst == 0).all() and (zst == 0).all() and np.array_equal(cd, zd) and np.array_equal(co, zo) and ctot == ztot


def test_capacity(engine):
    small = [c for c in mixed_batch() if len(c[1]) < 400]
    cases = [c for c in small if c[2] != 0] + [c for c in small if c[2] == 0][:60]
    types, pays = [c[0] for c in cases], [c[1] for c in cases]
    conv, st, tot = check(engine, types, pays, OPTS, data_cap=0)                        # sizes only, data NULL
    assert set(st.tolist()) == {zr.SKIP, zr.E_CONVERT, zr.E_CAPACITY}
    _, full, _ = check(engine, types, pays, OPTS, data_cap=tot["bytes"], conv=conv)
    assert zr.E_CAPACITY not in full.tolist()
    _, less, _ = check(engine, types, pays, OPTS, data_cap=tot["bytes"] - 1, host=True, conv=conv)
    last = max(i for i, s in enumerate(full.tolist()) if s == 0)
    assert less[last] == zr.E_CAPACITY and np.array_equal(np.delete(less, last), np.delete(full, last))
    check(engine, [], [], host=True, conv=np.zeros(0, np.uint8))


def test_on_a_stream(engine):
    cases = [c for c in mixed_batch() if len(c[1]) < 2000]
    check(engine, [c[0] for c in cases], [c[1] for c in cases], OPTS, stream=torch.cuda.Stream())


# ---- the chain a loader runs ------------------------------------------------------------------------------------
def pk(xs):
    offs = np.zeros(len(xs) + 1, np.uint64)
    np.cumsum([len(x) for x in xs], out=offs[1:])
    return np.frombuffer(b"".join(xs), np.uint8), offs


def test_chain_from_a_written_stream_to_decoded_zsets(engine):
    """Skiplist ZSets with fractional scores, written by rr_rdbsave_batch and rr_rdbfile_section, then index ->
    split -> rdbload -> rdbconvert -> rdbzset -> decode: the decoded ZSets are the oracle's decode of the
    reference's blobs."""
    f = Flat(21)
    rng = np.random.default_rng(21)
    edge = zr.edge_scores()
    edge = edge[(edge & np.uint64(0x7FFFFFFFFFFFFFFF)) < np.uint64(0x7FF0000000000000)]
    n = 48
    for i in range(n):
        pairs = sorted(((zr.to_double(int(edge[int(rng.integers(0, len(edge)))])) if j % 2 else (j * 13 % 17) / 16 + i, b"m%d" % j)
                        for j in range(i % 12 + 1)), reverse=True)     # serZset's order
        items = []
        for sc, m in pairs:
            items += [m, ("score", zr.to_bits(sc))]
        f.add(rr.T_ZSET_SKIPLIST, 0, items, lru=0)
    v, e, a = f.done()
    types, pdata, poffs, pst, _ = engine.rdbsave_host(v, e, a)
    assert (pst == 0).all() and (types == ZSET).all()
    keys = [b"z:%d" % i for i in range(n)]
    hd = rf.head("6.0.20", 1700000000, 1 << 33, None) + rf.selectdb(0, n, 0)
    sec, ro, rs, crc, res = engine.rdbfile_section_host(pdata, poffs, types, pst, *pk(keys), head=hd, flags=rr.RDBFILE_EOF)
    ix = rr.rdbread_index(sec)
    assert ix["rc"] == rr.RDBREAD_DONE and len(ix["rec_start"]) == n
    assert engine.rdbread_verify_host(sec, ix["eof_at"]) == (0, crc)
    sp = engine.rdbread_split_host(sec, ix["rec_start"], ix["rec_end"], ix["state"].version)
    assert (sp["status"] == 0).all() and (sp["types"] == ZSET).all()
    pd, po, pt = sp["pay_data"], sp["pay_offsets"], sp["types"]
    lst = engine.rdbload_host(pd, po, pt)[2]
    assert (lst == ld.E_CONVERT).all()
    cst = engine.rdbconvert_host(pd, po, pt, lst)[3]
    zd, zo, zst, ztot = engine.rdbzset_host(pd, po, pt, cst)
    assert ((cst == 0) == (zst == zr.SKIP)).all() and (zst[cst != 0] == 0).all() and (zst == 0).sum() > 40
    want = zr.zset_batch(pt, pd, po, cst)
    assert np.array_equal(zd, want[0]) and np.array_equal(zo, want[1]) and ztot == want[3]
    gv, ge, ga, gt = engine.decode_host(zd, zo)
    ov, oe, oa, ot = cpu.decode(want[0], want[1])
    assert np.array_equal(gv, ov) and np.array_equal(ge, oe) and np.array_equal(ga, oa)
    done = np.nonzero(zst == 0)[0]
    assert (gv["type"][done] == ZZL).all() and (gv["status"][done] == 0).all()
    pb = pd.tobytes()
    for i in done.tolist():                                             # and they hold what the stream's payloads hold
        _, items = ref.load(ZSET, pb[int(po[i]):int(po[i + 1])])
        blob = zd[int(zo[i]):int(zo[i + 1])].tobytes()
        got = ref.walk_ziplist(blob[13:])
        assert sorted(zip(got[0::2], got[1::2])) == sorted((m, zr.d2string(b)) for m, b in zip(items[0::2], items[1::2]))
