"""rr_aof_batch on the GPU against tests/aof_reference.py: every byte, offset, status and total, with a
canary behind and between what the call may write.

The batches are the smallest that reach the kernels' edges: 0 / 1 / 63 / 64 / 65 / 128 / 129 items of
each aggregate encoding (a command is one wave round of 64), the key lengths where "$len" grows, empty
and long members, every edge score, ziplist score entries as texts and integers, the refused texts,
expiries, the statuses, the capacity rule, one value more than a launch's waves, and a side stream."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr
from oracle import cpu, pyoracle

import aof_reference as ar
import flat_forge as ff
from aof_shapes import AGGREGATES, _bits, _word, add_aggregate, capacity_batch   # noqa: F401  (shared with the edge tests)
import rdb_reference as ref
import rdbzset_reference as zr

pytestmark = pytest.mark.gpu

CANARY = 0xA5
COUNTS = (0, 1, 63, 64, 65, 128, 129)
REFUSED = [b"nan", b"0x10", b"+1", b" 1", b"1e", b"", b"123456789012345678", b"1" * 41, b"infinity", b"1.2.3"]
NONCANON = [b"1.50", b".5", b"5.", b"1E5", b"1e309", b"-1e309", b"1e-400", b"-1e-400", b"0.1", b"00012.5000", b"9007199254740993",
            b"4.9406564584124654e-324", b"2.4703282292062328e-324", b"2.4703282292062327e-324", b"2.4703282292062329e-324",
            b"1.7976931348623158e308", b"100000000000000000000", b"0.00000000000000000000000000000000000001", b"-0", b"inf",
            b"-inf", b"12345678901234567e-340"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def check(engine, values, elems, arena, names, expires=None, data_cap=None, key_offsets=None, key_cap=None, stream=None):
    """Run the device call on canary-filled buffers and compare everything with the restatement."""
    n = len(values)
    kd, ko = ar.keys_of(names)
    if key_offsets is not None:
        ko = np.asarray(key_offsets, np.uint64)
    exp = None if expires is None else np.asarray(expires, np.int64)
    data, offsets, status, totals, slices = ar.aof_batch(values, elems, arena, kd, ko, exp, data_cap, key_cap)
    total = int(offsets[-1])
    cap = total if data_cap is None else data_cap
    room = ((max(cap, total) + 15) & ~15) + 64
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    d_exp = None if exp is None else torch.from_numpy(exp.copy()).cuda()
    d_ko = torch.from_numpy(ko.view(np.int64).copy()).cuda()
    args = (_dev(values), _dev(elems), _dev(arena), _dev(kd), d_ko, out[:cap], d_off, d_status[:n], d_tot)
    if stream is None:
        engine.aof(*args, expires=d_exp, key_cap=key_cap)
        torch.cuda.synchronize()
    else:
        torch.cuda.synchronize()                     # the uploads above ran on the default stream
        with torch.cuda.stream(stream):
            engine.aof(*args, expires=d_exp, key_cap=key_cap, stream=stream)
        stream.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), offsets)
    gs = d_status.cpu().numpy()
    if not np.array_equal(gs[:n], status):
        i = int(np.nonzero(gs[:n] != status)[0][0])
        raise AssertionError(f"status of value {i} (type {values['type'][i]}): got {gs[i]}, want {status[i]}")
    assert (gs[n:] == CANARY).all()
    t = d_tot.cpu().numpy().view(np.uint64)
    assert {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])} == totals
    want = np.full(room, CANARY, np.uint8)
    for i, s in enumerate(slices):
        if status[i] == 0:
            o = int(offsets[i])
            want[o:o + len(s)] = np.frombuffer(s, np.uint8)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        i = int(np.searchsorted(offsets, at, side="right")) - 1
        raise AssertionError(f"byte {at} (value {i}, type {values['type'][min(i, n - 1)] if n else None}, offset "
                             f"{at - int(offsets[min(i, n)])}): got {got[at]:#x}, want {want[at]:#x}")
    ne = pay = 0
    for _, descs in ref.flat_values(values, elems, arena):
        if descs is not None:
            ne += len(descs)
            pay += sum(d[2] for d in descs if d[0] == rr.K_STR)
    assert total <= rr.aof_bound(n, ne, pay, sum(len(k) for k in names))
    return status, totals, slices


def test_items_per_aggregate(engine):
    f = ff.Flat(11)
    for typ in AGGREGATES:
        for cnt in COUNTS:
            add_aggregate(f, typ, cnt)
    v, e, a = f.done()
    names = [b"k%d" % i for i in range(len(v))]
    st, _, slices = check(engine, v, e, a, names, expires=[-1 if i % 2 else 1700000000000 + i for i in range(len(v))])
    assert (st == 0).all()
    i = AGGREGATES.index(rr.T_SET_HT) * len(COUNTS) + COUNTS.index(129)
    assert slices[i].count(b"SADD") == 3 and slices[i].startswith(b"*66\r\n$4\r\nSADD\r\n")


def test_keys_and_members(engine):
    f = ff.Flat(12)
    names = []
    for kl in (0, 9, 10, 99, 100):
        for typ in (rr.T_STRING, rr.T_LIST_QUICKLIST, rr.T_HASH_HT):
            if typ == rr.T_STRING:
                f.add(typ, 0, [_word(f.rng, 5)])
            else:
                add_aggregate(f, typ, 70)
            names.append(_word(f.rng, kl))
    f.add(rr.T_SET_HT, 0, [b"", b"a", b""])                   # members of 0 bytes
    f.add(rr.T_LIST_QUICKLIST, 0, [b"", b"", _word(f.rng, 16384), b"z", _word(f.rng, 33), _word(f.rng, 32)])
    f.add(rr.T_HASH_HT, 0, [b"f", b"", b"", _word(f.rng, 9999)])
    names += [b"empties", _word(f.rng, 3000), b"h"]
    for a in range(16):                                       # every source alignment of a long body
        f.arena += bytes((a - len(f.arena)) % 16)
        at = len(f.arena)
        f.arena += _word(f.rng, 100)
        f.add(rr.T_STRING, 0, [("raw", rr.K_STR, at, 100, 0, 0)])
        names.append(_word(f.rng, a))
    st, _, _ = check(engine, *f.done(), names, expires=[1 if i % 4 == 0 else -1 for i in range(len(names))])
    assert (st == 0).all()


def test_scores(engine):
    f = ff.Flat(13)
    edge = [int(b) for b in zr.edge_scores().tolist() if zr.d2string(int(b)) != b"nan"]
    f.add(rr.T_ZSET_SKIPLIST, 0, [x for j, b in enumerate(edge) for x in (b"m%d" % j, ("score", b))])
    canon = [zr.d2string(b) for b in edge[::7]]               # ziplist score entries as canonical texts
    zl = ("zl", b"x" * 30)
    f.add(rr.T_ZSET_ZIPLIST, 0, [zl] + [x for j, t in enumerate(canon) for x in (b"c%d" % j, t)])
    ints = [-2**63, 2**63 - 1, 2**53 + 1, 2**53 + 3, 0, -1, 2**53, 10**17, -(2**53 + 1)]
    f.add(rr.T_ZSET_ZIPLIST, 0, [zl] + [x for j, v in enumerate(ints) for x in (b"i%d" % j, v)])
    f.add(rr.T_ZSET_ZIPLIST, 0, [zl] + [x for j, t in enumerate(NONCANON) for x in (b"n%d" % j, t)])
    names = [b"edge", b"canon", b"ints", b"noncanon"]
    st, _, slices = check(engine, *f.done(), names)
    assert (st == 0).all()
    assert b"$16\r\n9007199254740992\r\n$2\r\ni2\r\n" in slices[2] and b"$22\r\n9.2233720368547758e+18\r\n$2\r\ni1\r\n" in slices[2]
    assert b"$3\r\n1.5\r\n$2\r\nn0\r\n" in slices[3] and b"$3\r\ninf\r\n$2\r\nn4\r\n" in slices[3]


def test_refused_scores_leave_neighbours_alone(engine):
    f = ff.Flat(14)
    zl = ("zl", b"x" * 30)
    names = []
    for j, t in enumerate(REFUSED):
        f.add(rr.T_ZSET_ZIPLIST, 0, [zl, b"before", b"1.5"] + [x for k in range(70) for x in (b"m%d" % k, t if k == 66 else b"2")])
        f.add(rr.T_STRING, 0, [b"neighbour %d" % j])
        names += [b"bad%d" % j, b"good%d" % j]
    f.add(rr.T_ZSET_SKIPLIST, 0, [b"m", ("score", 0x7FF8000000000000)])       # a NaN score
    names.append(b"nan")
    st, tot, _ = check(engine, *f.done(), names, expires=[5] * len(names))
    assert (st[0:-1:2] == rr.AOF_E_CPU).all() and (st[1::2] == 0).all() and st[-1] == rr.AOF_E_CPU
    assert tot["n_bad"] == len(REFUSED) + 1


def test_strings_and_expiries(engine):
    f = ff.Flat(15)
    for x in (0, -1, 12, 2**63 - 1, -2**63, 10**9):
        f.add(rr.T_STRING, 1, [x])
    for ln in (0, 1, 44):
        f.add(rr.T_STRING, 8, [_word(f.rng, ln)])
    for ln in (0, 45, 70000):
        f.add(rr.T_STRING, 0, [_word(f.rng, ln)])
    f.add(rr.T_LIST_QUICKLIST, 0, [])                         # an expiry on an empty List
    f.add(rr.T_LIST_QUICKLIST, 0, [])                         # and none: size 0, status 0
    v, e, a = f.done()
    names = [b"key%d" % i for i in range(len(v))]
    exp = [(-1, 0, 1700000000000, -5, 2**63 - 1)[i % 5] for i in range(len(v) - 2)] + [1700000000000, -1]
    st, _, slices = check(engine, v, e, a, names, expires=exp)
    assert (st == 0).all() and slices[-1] == b"" and slices[-2].startswith(b"*3\r\n$9\r\nPEXPIREAT\r\n")
    check(engine, v, e, a, names)                              # expires NULL


def test_stays(engine):
    """A ZLRAW-only value, bad key slices, non-zero statuses, forged descriptors: each refused alone."""
    blobs = []
    for typ, items in ((rr.T_HASH_ZIPLIST, [b"f", b"v"]), (rr.T_ZSET_ZIPLIST, [b"m", b"1.5"]), (rr.T_ZSET_ZIPLIST, [])):
        z = pyoracle.build_ziplist(items)
        blobs.append(bytes([typ]) + struct.pack("<IQ", 0, len(z)) + z)
    blobs.append(bytes([rr.T_STRING]) + struct.pack("<I", 0) + b"\x00plain")
    blobs.append(bytes([rr.T_STRING]) + struct.pack("<I", 0) + b"\x07bad enc")
    from helpers import batch_from_blobs
    data, offs = batch_from_blobs(blobs)
    v, e, a, _ = rr.host_decode_ex(data, offs, rr.CTX_ZL_RAW)
    names = [b"a", b"bb", b"ccc", b"dddd", b"eeeee"]
    st, _, _ = check(engine, v, e, a, names, expires=[7] * 5)
    assert st.tolist() == [rr.AOF_E_CPU, rr.AOF_E_CPU, 0, 0, rr.E_ENCODE]
    v2, e2, a2, _ = rr.host_decode(data, offs)                # decoded in full: all but the bad blob are written
    st, _, _ = check(engine, v2, e2, a2, names)
    assert st.tolist() == [0, 0, 0, 0, rr.E_ENCODE]
    # key slices: reversed, past the cap, and a bad key on an unsaveable value (RR_E_ENCODE comes first)
    ko = np.array([0, 1, 3, 2, 6, 15], np.uint64)
    st, _, _ = check(engine, v2, e2, a2, names, key_offsets=ko, key_cap=15)
    assert st.tolist() == [0, 0, rr.RDBFILE_E_KEY, 0, rr.E_ENCODE]
    st, _, _ = check(engine, v2, e2, a2, names, key_offsets=np.array([0, 1, 3, 6, 10, 15], np.uint64), key_cap=9)
    assert st.tolist() == [0, 0, 0, rr.RDBFILE_E_KEY, rr.E_ENCODE]
    # forged: entry descriptors of a ziplist that do not fit, an odd entry count, a STR outside the arena
    f = ff.Flat(16)
    zl = ("zl", b"x" * 30)
    f.add(rr.T_HASH_ZIPLIST, 0, [zl, b"f", ("score", 5)])
    f.add(rr.T_ZSET_ZIPLIST, 0, [zl, b"m", b"1", b"odd"])
    f.add(rr.T_ZSET_ZIPLIST, 0, [zl, b"m", ("raw", rr.K_STR, 1 << 40, 3, 0, 0)])
    f.add(rr.T_ZSET_ZIPLIST, 0, [zl, b"m", b"nan", b"n", ("raw", 9, 0, 0, 0, 0)])   # a bad kind after a refused text
    f.add(rr.T_SET_HT, 0, [b"ok"], status=3)
    f.add(rr.T_SET_HT, 0, [b"ok"])
    st, _, _ = check(engine, *f.done(), [b"k"] * 6)
    assert st.tolist() == [rr.E_ENCODE] * 5 + [0]


@pytest.mark.parametrize("seed", [101])
def test_unsaveable_values(engine, seed):
    v, e, a, classes = ff.forge_mutations(*ff.well_formed(seed, 600), seed)
    names = [b"k%d" % i for i in range(len(v))]
    st, tot, _ = check(engine, v, e, a, names)
    assert (st == rr.E_ENCODE).any() and (st == 0).any() and tot["n_bad"] == int((st != 0).sum())


def test_capacity(engine):
    v, e, a = capacity_batch()[:3]
    names = [b"k%d" % i for i in range(len(v))]
    total = int(ar.aof_batch(v, e, a, *ar.keys_of(names))[1][-1])
    st, _, _ = check(engine, v, e, a, names, data_cap=0)
    assert st[0] == 0 and (st[1:] == rr.E_CAPACITY).all()
    st, _, _ = check(engine, v, e, a, names, data_cap=total)
    assert (st == 0).all()
    st, _, _ = check(engine, v, e, a, names, data_cap=total - 1)
    assert (st[:-1] == 0).all() and st[-1] == rr.E_CAPACITY
    check(engine, v[:0], e, a, [])


def test_past_the_wave_cap_and_on_a_stream(engine):
    n = rr.AOF_MAX_WAVES + 1
    f = ff.Flat(18)
    at = f.put(b"v")
    f.elems.append((at, 1, rr.K_STR, 0, 0))
    f.elems.append((7, 0, rr.K_INT, 0, 0))
    f.values = [(rr.T_STRING, (0, 1)[i % 2], 0, 0, 1, i % 2) for i in range(n)]
    v, e, a = f.done()
    names = [b"%d" % (i % 10) for i in range(n)]
    st, _, slices = check(engine, v, e, a, names)
    assert (st == 0).all() and slices[-1] == b"*3\r\n$3\r\nSET\r\n$1\r\n4\r\n$1\r\nv\r\n"
    g = ff.Flat(19)
    for typ in AGGREGATES:
        add_aggregate(g, typ, 130, k=3)
    v, e, a = g.done()
    st, _, _ = check(engine, v, e, a, [b"s%d" % i for i in range(len(v))], expires=[9] * len(v), stream=torch.cuda.Stream())
    assert (st == 0).all()


def test_round_trip_through_replay(engine):
    """decode -> rr_aof_batch -> RESP replay equals the oracle's objects, on a mixed generated batch."""
    data, offs = rr.gen_batch(rr.CONFIG_MIXED, 3000)
    n = len(offs) - 1
    v, e, a, t = engine.decode_host(data, offs)
    assert t["n_bad"] == 0
    names = [b"key:%d" % i for i in range(n)]
    kd, ko = ar.keys_of(names)
    exp = np.array([-1 if i % 5 else 1650000000000 + i for i in range(n)], np.int64)
    out, ooffs, st, tot = engine.aof_host(v, e, a, kd, ko, exp)
    assert (st == 0).all() and tot["n_bad"] == 0 and int(ooffs[-1]) == len(out)
    ov, oe, oa, _ = cpu.decode(data, offs)
    want = ar.aof_batch(ov, oe, oa, kd, ko, exp)
    assert np.array_equal(out, want[0]) and np.array_equal(ooffs, want[1]) and tot == want[3]
    db, expd = ar.replay(out)
    ab = oa.tobytes()
    for i, (val, descs) in enumerate(ref.flat_values(ov, oe, oa)):
        assert db.get(names[i]) == ar.model(val, descs, ab), i
        assert expd.get(names[i], -1) == int(exp[i])
    assert rr.aof_select(0) + bytes(out) == b"*2\r\n$6\r\nSELECT\r\n$1\r\n0\r\n" + b"".join(want[4])
