"""rr_rdbconvert_batch on the GPU against tests/rdbconvert_reference.py: every status, new type,
offset, blob byte and total, with a canary behind every buffer the call writes.  The load_status a
batch is given is the one the load rule gives (tests/rdbload_reference.py) unless a test says
otherwise; the payload bytes sit in an allocation of exactly data_cap bytes.  The batches are the
smallest that reach the kernels' paths: the compaction with none, some and all values attempted, the
thresholds at and one past their limits, the sort at its shapes, the prevlen chain and the string
headers at their borders, LZF fields round the window and the 64-byte reloads, capacity, input the
loader would not have passed on, one stride of the grid, a stream, the host entry, and the save ->
load -> convert -> decode round trip."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import lzf_reference as lzf
import rdb_reference as ref
import rdbconvert_reference as cv
import rdbload_reference as ld
from rdbload_mutants import lz, lzf_str
from test_rdbconvert import BIG, HASH, HZL, ISET, L, S, SET, ZSET, ZZL, dbl, literal_cases, over_max_n, raw

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def loader_status(types, payloads, opts):
    return np.array([ld.load_blob(t, p, opts)[0] for t, p in zip(types, payloads)], np.uint8)


def run_device(engine, types, data, offsets, load_status, opts, cap, room, stream=None):
    n = len(types)
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_otypes = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4 + 2,), -3, dtype=torch.int64, device="cuda")
    d_data = _dev(data) if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")   # exactly data_cap bytes
    d_in_off = torch.from_numpy(np.ascontiguousarray(offsets, np.uint64).view(np.int64).copy()).cuda()
    d_types = _dev(np.asarray(types, np.uint8)) if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_load = _dev(np.asarray(load_status, np.uint8)) if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
    engine.rdbconvert(d_data, d_in_off, d_types, d_load, out[:cap], d_off[:n + 1], d_otypes[:n], d_status[:n], d_tot[:4],
                      opts=ld.c_opts(opts) if opts else None, stream=stream)
    return out, d_off, d_otypes, d_status, d_tot


def compare(bufs, n, want, room):
    out, d_off, d_otypes, d_status, d_tot = bufs
    data, offsets, out_types, status, totals, blobs = want
    got_off = d_off.cpu().numpy()
    assert np.array_equal(got_off[:n + 1].view(np.uint64), offsets) and (got_off[n + 1:] == 7).all()
    st = d_status.cpu().numpy()
    if not np.array_equal(st[:n], status):
        i = int(np.nonzero(st[:n] != status)[0][0])
        raise AssertionError(f"status of value {i}: got {st[i]}, want {status[i]}")
    assert (st[n:] == CANARY).all()
    ot = d_otypes.cpu().numpy()
    assert np.array_equal(ot[:n], out_types) and (ot[n:] == CANARY).all()
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


def check(engine, types, payloads, opts=None, data_cap=None, host=False, load_status=None, stream=None):
    """The device call on canary-filled buffers against the reference; host: the host entry too."""
    data, offsets = ld.pack(payloads)
    n = len(types)
    if load_status is None:
        load_status = loader_status(types, payloads, opts)
    want = cv.convert_batch(types, data, offsets, load_status, opts, data_cap)
    total = int(want[1][-1])
    cap = total + 40 if data_cap is None else data_cap
    room = max(cap, total) + 64
    if stream is not None:
        with torch.cuda.stream(stream):
            bufs = run_device(engine, types, data, offsets, load_status, opts, cap, room, stream)
    else:
        bufs = run_device(engine, types, data, offsets, load_status, opts, cap, room)
    torch.cuda.synchronize()
    compare(bufs, n, want, room)
    if host:
        hd, ho, hot, hs, ht = engine.rdbconvert_host(data, offsets, np.asarray(types, np.uint8), load_status,
                                                     ld.c_opts(opts) if opts else None, data_cap)
        assert np.array_equal(ho, want[1]) and np.array_equal(hot, want[2]) and np.array_equal(hs, want[3]) and ht == want[4]
        if data_cap is None:
            assert np.array_equal(hd, want[0])
    return want[3], want[4]


FILL = [(S, raw(b"hello")), (S, b"\x05abc"), (L, b"\x00"), (1, b"\x00"), (ISET, raw(struct.pack("<II", 2, 0))), (S, b"\xC0\x07")]


def mixed(cases):
    """The cases interleaved with values of status 0 and of error statuses."""
    types, pays = [], []
    for k, (t, p) in enumerate(cases):
        ft, fp = FILL[k % len(FILL)]
        types += [ft, t]
        pays += [fp, p]
    return types, pays


# ---- 1. the literals of the CPU file, SKIP and the compaction ---------------------------------------
def test_literals_interleaved(engine):
    groups = {}
    for t, p, o, st, blob in literal_cases():
        groups.setdefault(tuple(sorted((o or ld.DEFAULTS).items())), []).append((t, p, st))
    seen = set()
    for key, cases in groups.items():
        types, pays = mixed([(c[0], c[1]) for c in cases])
        st, _ = check(engine, types, pays, dict(key), host=True)
        assert st[1::2].tolist() == [c[2] for c in cases] and (st[0::2] == cv.SKIP).all()
        seen |= set(st.tolist())
    assert seen == {0, cv.E_CONVERT, cv.SKIP}


def test_none_attempted_all_attempted_empty(engine):
    st, tot = check(engine, [f[0] for f in FILL] * 50, [f[1] for f in FILL] * 50, host=True)
    assert (st == cv.SKIP).all() and tot == {"n_elems": 0, "bytes": 0, "n_bad": 0, "payload": 0}
    cases = [(t, p) for t, p, o, s, _ in literal_cases() if o is None]
    st, tot = check(engine, [c[0] for c in cases] * 9, [c[1] for c in cases] * 9)
    assert (st != cv.SKIP).all() and tot["n_bad"] == int((st != 0).sum()) > 0
    check(engine, [], [], host=True)


# ---- 2. thresholds ------------------------------------------------------------------------------------
def set_of(n, f=lambda k: str(k).encode()):
    return ref.save_len(n) + b"".join(raw(f(k)) for k in range(n))


def hash_of(n, vlen=1):
    return ref.save_len(n) + b"".join(raw(b"f%d" % k) + raw(b"v" * vlen) for k in range(n))


def zset_of(n, mlen=1, score=lambda k: float(k)):
    return ref.save_len(n) + b"".join(raw((b"%d" % k).rjust(mlen, b"m")) + dbl(score(k)) for k in range(n))


@pytest.mark.parametrize("small", [True, False])
def test_thresholds_at_and_past(engine, small):
    if small:
        o = ld.options(set_max_intset_entries=2, hash_max_ziplist_entries=2, hash_max_ziplist_value=3,
                       zset_max_ziplist_entries=2, zset_max_ziplist_value=3)
        e = (2, 2, 3, 2, 3)
    else:
        o = None
        e = (512, 512, 64, 128, 64)
    cases = []
    for d in (0, 1):
        cases += [(SET, set_of(e[0] + d)), (HASH, hash_of(e[1] + d)), (HASH, hash_of(2, e[2] + d)), (ZSET, zset_of(e[3] + d)),
                  (ZSET, zset_of(2, e[4] + d))]
    types, pays = mixed(cases)
    claim = np.full(len(types), cv.E_CONVERT, np.uint8)                 # one past: claimed, and refused
    claim[0::2] = loader_status(types[0::2], pays[0::2], o)
    st, _ = check(engine, types, pays, o, load_status=claim)
    assert st[1::2].tolist() == [0] * 5 + [cv.E_CONVERT] * 5
    st, _ = check(engine, types, pays, o)                               # as the loader hands them on: the five past are status 0 there
    assert st[1::2].tolist() == [0] * 5 + [cv.SKIP] * 5


def test_max_n(engine):
    o, over = over_max_n()
    at = [(SET, set_of(cv.MAX_N)), (ZSET, zset_of(cv.MAX_N))]
    st, _ = check(engine, [c[0] for c in at + over], [c[1] for c in at + over], o)
    assert st.tolist() == [0, 0, cv.E_CONVERT, cv.E_CONVERT]


# ---- 3. sort shapes -----------------------------------------------------------------------------------
def test_sort_shapes(engine):
    o = ld.options(zset_max_ziplist_entries=512, zset_max_ziplist_value=200)
    rng = np.random.default_rng(5)
    cases = []
    for n in (1, 2, 63, 64, 65, 511, 512):
        perm = rng.permutation(n)
        for order in (lambda k: k, lambda k: n - 1 - k, lambda k: 7, lambda k: int(perm[k])):
            cases.append((SET, set_of(n, lambda k: str((order(k) - n // 2) * 40000).encode())))
            if n <= 65 or order(0) != 7:
                cases.append((ZSET, zset_of(n, 1, lambda k: float(order(k) % 50))))
    cases.append((ZSET, zset_of(130, 1, lambda k: 7.0)))                # every score ties: the members decide
    long_ = [b"x" * 70 + bytes([97 + (k * 7) % 26]) + b"y" * (k % 3) for k in range(40)]   # ties past byte 64, and in length
    long_ += [b"x" * 70, b"x" * 71, b"x" * 69]
    cases.append((ZSET, ref.save_len(len(long_)) + b"".join(raw(m) + dbl(3.0) for m in long_)))
    cases.append((ZSET, b"\x06" + b"".join(m + dbl(s) for m, s in (          # integer-form members among the ties
        (b"\xC0\x0C", 1.0), (raw(b"100"), 1.0), (b"\xC1\xE8\x03", 1.0), (raw(b"1"), 1.0), (b"\xC0\xFB", 1.0), (raw(b"-"), 1.0)))))
    st, _ = check(engine, [c[0] for c in cases], [c[1] for c in cases], o)
    assert (st == 0).all()


# ---- 4. the prevlen chain and the string headers ----------------------------------------------------------
def test_prevlen_chain_and_string_headers(engine):
    o = ld.options(hash_max_ziplist_value=1 << 31)
    body = lambda total: b"q" * (total - 1 - (1 if total - 2 < 64 else 2 if total - 3 < 16384 else 5))   # a 1-byte prevlen entry of `total`
    cases = []
    for a in (253, 254, 255):
        assert len(ref.zip_entry(0, body(a))) == a
        for b in (249, 250, 251, 252, 253):
            cases.append((HASH, b"\x02" + raw(body(a)) + raw(b"w" * b) + raw(b"k") + raw(b"z" * b)))
    for n in (63, 64, 16383, 16384):
        cases.append((HASH, b"\x01" + raw(b"f") + raw(b"s" * n)))
    st, _ = check(engine, [c[0] for c in cases], [c[1] for c in cases], o)
    assert (st == 0).all()


# ---- 5. LZF fields and values ----------------------------------------------------------------------------
def test_lzf_fields(engine):
    o = ld.options(hash_max_ziplist_value=1 << 20)
    cases = []
    for n in (21, 31, 32, 64):
        cases.append((HASH, b"\x02" + lz(b"ab" * (n // 2) + b"a" * (n % 2)) + lz(b"7" * n) + raw(b"k") + lz(b"z" * n)))
    cases.append((HASH, b"\x01" + lzf_str(b"\x001" + b"\x20\x00" * 5 + b"\x0123", 18) + lzf_str(b"\x02-12", 3)))   # integers through the window
    big = bytes((k * 131 + (k >> 8)) & 0xFF for k in range(20000))
    comp = lzf.compress(big + big, 2 * len(big) - 4)
    cases.append((HASH, b"\x01" + raw(b"big") + lzf_str(comp, 2 * len(big))))
    for pad in range(58, 68):                                           # a stream whose sequences straddle the 64-byte reloads
        text = bytes(range(33, 33 + pad % 29 + 4)) + b"abcabcabcabc" * 9 + bytes(range(60, 120)) + b"abcabc" * 5
        cases.append((HASH, b"\x01" + raw(b"p" * pad) + lz(text)))
    cases.append((SET, b"\x02" + lz(b"1" * 19) + raw(b"5")))   # an LZF Set member of 19 digits
    st, _ = check(engine, [c[0] for c in cases], [c[1] for c in cases], o)
    assert (st == 0).all()


def test_zset_deviations(engine):
    cases = [(ZSET, b"\x01" + lz(b"ab" * 18) + dbl(1.0))]
    cases += [(ZSET, b"\x02" + raw(b"a") + dbl(2.0) + raw(b"m") + dbl(s)) for s in (1.5, float(2**52), float("nan"), -BIG)]
    cases += [(ZSET, b"\x02" + raw(b"a") + dbl(2.0) + raw(b"m") + dbl(s)) for s in (BIG, -BIG + 1, -0.0)]
    st, _ = check(engine, *mixed(cases))
    assert st[1::2].tolist() == [cv.E_CONVERT] * 5 + [0] * 3


# ---- 6. capacity -----------------------------------------------------------------------------------------
def test_capacity(engine):
    cases = [(t, p) for t, p, o, s, _ in literal_cases() if o is None]
    types, pays = mixed(cases)
    st, tot = check(engine, types, pays, data_cap=0)                    # sizes only, data NULL
    assert set(st.tolist()) == {cv.SKIP, cv.E_CONVERT, cv.E_CAPACITY}
    full, _ = check(engine, types, pays, data_cap=tot["bytes"])
    assert cv.E_CAPACITY not in full.tolist()
    less, _ = check(engine, types, pays, data_cap=tot["bytes"] - 1, host=True)
    last = max(i for i, s in enumerate(full.tolist()) if s == 0)
    assert less[last] == cv.E_CAPACITY and np.array_equal(np.delete(less, last), np.delete(full, last))


# ---- 7. a load_status the loader would not have given --------------------------------------------------
def test_wrong_load_status(engine):
    two = ld.options(set_max_intset_entries=2, hash_max_ziplist_entries=2, hash_max_ziplist_value=3,
                     zset_max_ziplist_entries=2, zset_max_ziplist_value=3)
    good = (HASH, b"\x01" + raw(b"a") + raw(b"12"))
    cases = [good,
             (HASH, b"\x02" + raw(b"a") + raw(b"12")),                   # truncated: the next value's bytes are behind it
             good,
             (SET, b"\x02" + raw(b"1") + b"\x40"),                       # truncated inside a length
             good,
             (ZSET, b"\x01" + raw(b"m") + dbl(1.0)[:5]),                 # truncated inside the score
             good,
             (HASH, b"\x01" + raw(b"a") + raw(b"1234")),                 # above hash_max_ziplist_value
             (SET, b"\x03" + raw(b"1") + raw(b"2") + raw(b"3")),         # above set_max_intset_entries
             (SET, b"\x02" + raw(b"1") + raw(b"x")),                     # not an integer
             (HASH, b"\x01" + raw(b"a") + raw(b"b") + b"\x00"),          # a byte left over
             (L, b"\x00"), (S, raw(b"hello")), (ISET, raw(struct.pack("<II", 2, 0))), (1, b"\x00"), (255, b""),
             (HASH, b"\x81" + b"\xFF" * 8), (SET, b"\x82"), (HASH, b"\x01\xC4\x00\x01a"),
             good]
    types, pays = [c[0] for c in cases], [c[1] for c in cases]
    claim = np.full(len(cases), cv.E_CONVERT, np.uint8)
    st, tot = check(engine, types, pays, two, load_status=claim)
    want = [0 if c is good else cv.E_CONVERT for c in cases]
    assert st.tolist() == want and tot["n_bad"] == want.count(cv.E_CONVERT)
    data, offs = ld.pack(pays)                                           # bad slices: reversed, and past data_cap
    offs2 = offs.copy()
    offs2[2], offs2[-1] = offs[1] - 1, offs[-1] + 5
    want = cv.convert_batch(types, data, offs2, claim, two)
    room = int(want[1][-1]) + 64
    bufs = run_device(engine, types, data, offs2, claim, two, room - 24, room)
    torch.cuda.synchronize()
    compare(bufs, len(types), want, room)
    assert want[3][1] == cv.E_CONVERT and want[3][-1] == cv.E_CONVERT


# ---- 8. more attempted values than one launch has waves; a stream ------------------------------------------
def test_past_the_wave_cap(engine):
    n = cv.MAX_WAVES + 3
    types = [HASH] * n
    pays = [b"\x02" + raw(b"f") + raw(b"%d" % k) + raw(b"g") + raw(b"v%d" % (k % 97)) for k in range(n)]
    data, offsets = ld.pack(pays)
    claim = np.full(n, cv.E_CONVERT, np.uint8)
    want = cv.convert_batch(types, data, offsets, claim)
    room = int(want[1][-1]) + 64
    bufs = run_device(engine, types, data, offsets, claim, None, room - 24, room)
    torch.cuda.synchronize()
    compare(bufs, n, want, room)
    assert (want[3] == 0).all()


def test_on_a_stream(engine):
    cases = [(t, p) for t, p, o, s, _ in literal_cases() if o is None]
    types, pays = mixed(cases * 8)
    check(engine, types, pays, stream=torch.cuda.Stream())


# ---- 9. save -> load -> convert -> decode ------------------------------------------------------------------
def rewrite(t, p):
    """A small ziplist Hash / ZSet or an intset payload in its RDB_TYPE_HASH / ZSET_2 / SET form: (new type,
    new payload, what the value holds, whether that is already in the converted order), or None.  A score
    only %.17g prints is replaced by the integer below it, so that every rewritten value converts."""
    if t == ISET:
        _, w, vals = ref.load(t, p)
        return SET, ref.save_len(len(vals)) + b"".join(ref.save_raw_string(str(v).encode()) for v in vals), vals, vals == sorted(vals)
    if t not in (HZL, ZZL):
        return None
    ents = ref.walk_ziplist(ref.load(t, p)[1])
    if t == HZL:
        return HASH, ref.save_len(len(ents) // 2) + b"".join(ref.save_raw_string(e) for e in ents), ents, True
    out, keys, held = ref.save_len(len(ents) // 2), [], []
    for m, s in zip(ents[0::2], ents[1::2]):
        x = float(s)
        if cv.d2string(struct.unpack("<Q", dbl(x))[0]) is None:
            x = float(int(max(-2.0**40, min(2.0**40, x)))) if x == x else 0.0
        out += ref.save_raw_string(m) + dbl(x)
        keys.append((x, m))
        held += [m, cv.d2string(struct.unpack("<Q", dbl(x))[0])]
    return ZSET, out, held, keys == sorted(keys)


def test_save_load_convert_decode(engine):
    data, offs = rr.gen_batch(4, 2000)
    v, e, a, _ = engine.decode_host(data, offs)
    types, pdata, poffs, pst, _ = engine.rdbsave_host(v, e, a)
    assert (pst == 0).all()
    pb = pdata.tobytes()
    new_t, new_p, orig, sorted_ = [], [], {}, {}
    for i, t in enumerate(types.tolist()):
        p = pb[int(poffs[i]):int(poffs[i + 1])]
        r = rewrite(t, p)
        if r is None:
            new_t.append(t); new_p.append(p)
        else:
            new_t.append(r[0]); new_p.append(r[1])
            orig[i], sorted_[i] = (t, r[2]), r[3]
    kinds = {new_t[i] for i in orig}
    assert kinds == {SET, HASH, ZSET} and len(orig) > 100, (kinds, len(orig))
    nd, no = ld.pack(new_p)
    nt = np.asarray(new_t, np.uint8)
    want_load = ld.load_batch(nt, nd, no)
    want = cv.convert_batch(nt, nd, no, want_load[2])
    attempted = want_load[2] == ld.E_CONVERT
    assert set(np.nonzero(attempted)[0].tolist()) == set(orig)
    assert int((want[3][attempted] != 0).sum()) == 0                    # the reference first: nothing stays E_CONVERT
    _, lo, lst, _ = engine.rdbload_host(nd, no, nt)
    assert np.array_equal(lst, want_load[2])
    cd, co, cot, cst, ctot = engine.rdbconvert_host(nd, no, nt, lst)
    assert np.array_equal(cst, want[3]) and np.array_equal(co, want[1]) and np.array_equal(cd, want[0])
    assert int((cst[attempted] != 0).sum()) == 0 and ctot["n_bad"] == 0
    v2, e2, a2, t2 = engine.decode_host(cd, co)
    assert (v2["status"][attempted] == 0).all()
    ab2 = a2.tobytes()
    for i, (val, descs) in enumerate(ref.flat_values(v2, e2, a2)):
        if i not in orig:
            continue
        t, was = orig[i]
        assert val["type"] == t == cot[i]
        if t == ISET:
            got = [ref._signed(d[1]) for d in descs]
            assert got == sorted(set(was)) and (not sorted_[i] or got == was)
        else:
            got = ref.walk_ziplist(ab2[descs[0][1]:descs[0][1] + descs[0][2]])
            pairs = lambda x: sorted(zip(x[0::2], x[1::2]))
            assert pairs(got) == pairs(was) and (not sorted_[i] or got == was)
