"""rr_rdbmerge_batch and rr_rdbloadall_batch on the GPU, byte for byte against tests/rdbloadall_reference.py, with
a canary behind every buffer the calls write.  The rule batch runs the primitive behind the three public stage
calls and the one call beside it; the emit kernel's seams, alignments and source patterns run the primitive over
stage batches forged on the device, so every size, offset and status is the test's own.  S is the span of
out->data a wave owns (RR_RDBMERGE_SPAN)."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr
from oracle import cpu

import flat_forge as ff
import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbloadall_reference as la
import rdbzset_reference as zr
from rdbmerge_shapes import forge
from test_gpu_rdbzset import OPTS, mixed_batch
from test_rdbzset import ZSET, raw, zset

pytestmark = pytest.mark.gpu

CANARY = 0xA5
S = rr.RDBMERGE_SPAN
CAP, CONV, SLICE = la.E_CAPACITY, la.E_CONVERT, la.E_SLICE
SKIP2, SKIP3 = cv.SKIP, zr.SKIP
HASH, SET, ISET, ZZL, HZL = rr.T_HASH_HT, rr.T_SET_HT, rr.T_SET_INTSET, rr.T_ZSET_ZIPLIST, rr.T_HASH_ZIPLIST


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda() if a.size else torch.zeros(0, dtype=torch.uint8, device="cuda")


def _offs(o):
    return torch.from_numpy(np.ascontiguousarray(o, np.uint64).view(np.int64).copy()).cuda()


def _totals(t):
    t = t.cpu().numpy()[:4].view(np.uint64)
    return {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])}


class Out:
    """The buffers a call writes, canaries behind each: out (cap bytes of room), offsets, out_types, status, totals,
    stage_bytes."""

    def __init__(self, n, cap, room):
        self.n, self.cap, self.room = n, cap, room
        self.data = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
        self.offs = torch.full((n + 1 + 4,), 7, dtype=torch.int64, device="cuda")
        self.types = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
        self.status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
        self.tot = torch.full((4 + 2,), -3, dtype=torch.int64, device="cuda")
        self.sb = torch.full((3 + 2,), -5, dtype=torch.int64, device="cuda")

    def args(self):
        n = self.n
        return self.data[:self.cap], self.offs[:n + 1], self.types[:n], self.status[:n]

    def compare(self, want, stage_bytes=None):
        n = self.n
        data, offsets, out_types, status, totals, blobs = want[:6]
        got_off = self.offs.cpu().numpy()
        assert np.array_equal(got_off[:n + 1].view(np.uint64), offsets) and (got_off[n + 1:] == 7).all()
        st, ty = self.status.cpu().numpy(), self.types.cpu().numpy()
        if not np.array_equal(st[:n], status):
            i = int(np.nonzero(st[:n] != status)[0][0])
            raise AssertionError(f"status of value {i}: got {st[i]}, want {status[i]}")
        assert np.array_equal(ty[:n], out_types), np.nonzero(ty[:n] != out_types)[0][:5]
        assert (st[n:] == CANARY).all() and (ty[n:] == CANARY).all()
        t = self.tot.cpu().numpy()
        assert (t[4:] == -3).all() and _totals(self.tot) == totals, (_totals(self.tot), totals)
        sb = self.sb.cpu().numpy()
        assert (sb[3:] == -5).all() and (sb[:3].tolist() == list(stage_bytes) if stage_bytes is not None else (sb == -5).all())
        exp = blobs                                                              # rdbmerge_shapes.fast_merge: the room's image itself
        if not isinstance(blobs, np.ndarray):
            exp = np.full(self.room, CANARY, np.uint8)
            for i, b in enumerate(blobs):
                if b is not None:
                    o = int(offsets[i])
                    exp[o:o + len(b)] = np.frombuffer(b, np.uint8)
        got = self.data.cpu().numpy()
        if not np.array_equal(got, exp):
            at = int(np.nonzero(got != exp)[0][0])
            i = int(np.searchsorted(offsets, at, side="right")) - 1
            raise AssertionError(f"byte {at} (value {i}, offset {at - int(offsets[min(i, n)])}): got {got[at]:#x}, want {exp[at]:#x}")


def merge_device(engine, stages, types, conv_types, data_cap=None, stream=None, want=None):
    """The primitive over three (data, offsets, status, data_cap) stage batches, against the reference."""
    n = len(stages[0][1]) - 1
    if want is None:
        want = la.merge(*stages, types, conv_types, data_cap)
    total = int(want[1][-1])
    cap = total + 40 if data_cap is None else data_cap
    o = Out(n, cap, max(cap, total) + 64)
    dev = [(_dev(d[:c]), _offs(of), _dev(s)) for d, of, s, c in stages]
    assert all(t[0].numel() == st[3] for t, st in zip(dev, stages))          # exactly data_cap bytes exist
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    engine.rdbmerge(*dev, _dev(np.asarray(conv_types, np.uint8)), _dev(np.asarray(types, np.uint8)), *o.args(), o.tot[:4], stream=stream)
    torch.cuda.synchronize()
    o.compare(want)
    return want


def forged(engine, items, seed=0, lead=(0, 0, 0), data_cap=None, stream=None):
    n = len(items)
    types = (np.arange(n) % 251).astype(np.uint8)
    conv = ((np.arange(n) + 7) % 251).astype(np.uint8)
    return merge_device(engine, forge(items, seed, lead), types, conv, data_cap, stream)


# ---- the rule ----------------------------------------------------------------------------------------------------
def rule_batch():
    """A few hundred values for every row of the table: the zset test's mixed batch (Strings, a List, an intset,
    integer Sets and ZSets for the second stage, fractional ZSets for the third, LZF and NaN ZSets that stay
    E_CONVERT, a truncated payload, bad types) and what it lacks."""
    c = [(t, p) for t, p, _ in mixed_batch()]
    extra = [(HASH, b"\x02" + raw(b"f") + raw(b"12") + raw(b"g" * 9) + raw(b"hello")),           # a Hash that shrank
             (HASH, b"\x00"), (SET, b"\x03" + raw(b"-7") + raw(b"70000") + raw(b"12")),
             (ZSET, zset([(b"a", 3.0), (b"b", -1.0)])), (ZSET, zset([(b"a", 1.5)])),
             (ISET, raw(struct.pack("<IIhh", 2, 2, -3, 9))), (ZZL, raw(cv.ziplist_of([b"m", b"1.5"]))),
             (HZL, raw(cv.ziplist_of([b"f", b"v"]))), (rr.T_LIST_QUICKLIST, b"\x01" + raw(cv.ziplist_of([b"x", b"12"]))),
             (rr.T_STRING, raw(b"s" * 100)), (rr.T_STRING, b"\xC0\x07"), (rr.T_STRING, raw(b"t" * 70000)[:-1]), (3, b"\x00")]
    for k, e in enumerate(extra):
        c.insert(17 * k + 5, e)
    return [x[0] for x in c], [x[1] for x in c]


def rule_input():
    types, pays = rule_batch()
    data, offs = ld.pack(pays)
    offs = offs.copy()
    rev = REV = next(i for i in range(40, len(types)) if types[i] == ZSET and types[i + 1] == ZSET)
    offs[rev + 1] = offs[rev] - np.uint64(1)                                  # a reversed input slice: E_TRUNC, not read
    return np.asarray(types, np.uint8), data, offs, REV


def stage_calls(engine, types, data, offs, opts, caps=None):
    """The three public stage calls on the device: [(data, offsets, status)] x 3 and conv_types."""
    n = len(types)
    full = la.expected_batch(types, data, offs, opts)[6]
    caps = full if caps is None else caps
    d_in, d_off, d_ty = _dev(data), _offs(offs), _dev(types)
    co = ld.c_opts(opts)
    out = [(torch.zeros(c, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
            torch.zeros(n, dtype=torch.uint8, device="cuda")) for c in caps]
    tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    conv_types = torch.zeros(n, dtype=torch.uint8, device="cuda")
    engine.rdbload(d_in, d_off, d_ty, *out[0], tot, opts=co)
    engine.rdbconvert(d_in, d_off, d_ty, out[0][2], out[1][0], out[1][1], conv_types, out[1][2], tot, opts=co)
    engine.rdbzset(d_in, d_off, d_ty, out[1][2], *out[2], tot, opts=co)
    return out, conv_types, d_ty


def loadall(engine, types, data, offs, opts, stage_cap, data_cap, want, stream=None, room=None):
    n = len(types)
    total = int(want[1][-1])
    o = Out(n, data_cap, room or max(data_cap, total) + 64)
    need = rr.rdbloadall_ws_bytes(n, stage_cap)
    ws = torch.full((need + 32,), CANARY, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    engine.rdbloadall(_dev(data), _offs(offs), _dev(types), ws[:need], stage_cap, *o.args(), o.sb[:3], o.tot[:4],
                      opts=ld.c_opts(opts), stream=stream)
    torch.cuda.synchronize()
    assert (ws[need:] == CANARY).all()
    o.compare(want, want[6])
    return o


def test_rule_batch_primitive_and_one_call(engine):
    types, data, offs, rev = rule_input()
    n = len(types)
    want = la.expected_batch(types, data, offs, OPTS)
    st = want[3]
    assert 300 < n < 400 and {0, CONV, ld.E_TRUNC, ld.E_TYPE} <= set(st.tolist()) and st[rev] == ld.E_TRUNC
    held = [want[2][(st == 0)].tolist().count(t) for t in (rr.T_STRING, rr.T_LIST_QUICKLIST, ISET, ZZL, HZL)]
    assert all(h >= 1 for h in held) and want[4]["n_elems"] > 250
    stages, conv_types, d_ty = stage_calls(engine, types, data, offs, OPTS)
    total = int(want[1][-1])
    o = Out(n, total + 40, total + 104)
    engine.rdbmerge(*stages, conv_types, d_ty, *o.args(), o.tot[:4])
    torch.cuda.synchronize()
    o.compare(want)
    s1, s2, s3 = (s[2].cpu().numpy() for s in stages)                          # every row of the table was there
    assert ((s1 == CONV) & (s2 == 0)).sum() >= 5 and ((s2 == CONV) & (s3 == 0)).sum() > 200 and ((s2 == CONV) & (s3 == CONV)).sum() >= 3
    assert ((s1 == CONV) & (s2 == CONV) & (s3 == SKIP3)).sum() >= 2
    one = loadall(engine, types, data, offs, OPTS, want[6], total + 40, want)
    for a, b in ((one.data, o.data), (one.offs, o.offs), (one.types, o.types), (one.status, o.status), (one.tot, o.tot)):
        assert torch.equal(a, b)


def test_workspace_checks(engine):
    """RR_API_EINVAL for a short and for a misaligned workspace, before anything is launched (the canaries stay)."""
    types, data, offs, rev = rule_input()
    n = len(types)
    want = la.expected_batch(types, data, offs, OPTS)
    need = rr.rdbloadall_ws_bytes(n, want[6])
    o = Out(n, 64, 128)
    ws = torch.full((need + 32,), CANARY, dtype=torch.uint8, device="cuda")
    call = lambda w, nb: engine.rdbloadall(_dev(data), _offs(offs), _dev(types), w, want[6], *o.args(), o.sb[:3], o.tot[:4],
                                           opts=ld.c_opts(OPTS), ws_bytes=nb)
    for w, nb, word in ((ws[:need], need - 1, "ws_bytes"), (ws[8:], need, "aligned"), (ws[1:], need, "aligned")):
        with pytest.raises(rr.RRError, match=word):
            call(w, nb)
    with pytest.raises(rr.RRError, match="aligned"):                            # out->data of the primitive and the one call
        engine.rdbloadall(_dev(data), _offs(offs), _dev(types), ws, want[6], o.data[8:72], o.offs[:n + 1], o.types[:n], o.status[:n],
                          o.sb[:3], o.tot[:4], opts=ld.c_opts(OPTS))
    torch.cuda.synchronize()
    assert (ws == CANARY).all() and (o.data == CANARY).all() and (o.status == CANARY).all() and (o.tot == -3).all()


# ---- the seams of the emit kernel ----------------------------------------------------------------------------------
def test_span_seams(engine):
    sizes = [6, 15, 16, 17, S - 1, S, S + 1, 3 * S + 5]
    items, at = [], 0

    def add(k, size):
        nonlocal at
        items.append((k, size))
        at += size if k in (1, 2, 3) else 0

    for j, sz in enumerate(sizes):
        add(1 + j % 3, sz)
    add(2, (-at - 1) % S)                                                     # the next value starts on the last byte of a span
    add(3, 50)
    assert (at - 50) % S == S - 1
    add(1, (-at) % S)                                                         # ends exactly on a span's start
    assert at % S == 0
    for j in range(70):                                                       # a run of bad, empty values across that start
        add(ld.E_TRUNC if j % 2 else ld.E_LEN, 0)
    add(2, 70000)                                                             # spans that begin and end inside one value
    add(3, 0)                                                                 # a held blob of size 0
    add(1, 33)                                                                # the last span partial
    assert at % S not in (0, S - 1)
    want = forged(engine, items, seed=1)
    assert want[4]["bytes"] == at and want[4]["n_bad"] == 70


@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single(engine, n):
    want = forged(engine, [(2, 21)] * n, seed=2)
    assert want[4]["bytes"] == 21 * n
    forged(engine, [(ld.E_TRUNC, 0)] * n, seed=2)                             # nothing to write at all


def test_more_spans_than_one_grid(engine):
    """Merged bytes past RR_RDBMERGE_MAX_WAVES x S, from three large Strings with small values between: the
    second stride of the span loop.  Generated and compared on the device."""
    big = rr.RDBMERGE_MAX_WAVES * S // 3 + 4097
    sizes = [(1, 19), (1, big), (2, 77), (1, big + 3), (3, 100), (ld.E_TRUNC, 0), (1, big + 7), (2, 5)]
    n = len(sizes)
    g = torch.Generator(device="cuda").manual_seed(3)
    st = np.zeros((3, n), np.uint8)
    offs = np.zeros((3, n + 1), np.uint64)
    for i, (k, sz) in enumerate(sizes):
        st[:, i] = [(0, SKIP2, SKIP3), (CONV, 0, SKIP3), (CONV, CONV, 0)][k - 1] if k in (1, 2, 3) else (k, SKIP2, SKIP3)
        for j in range(3):
            offs[j, i + 1] = offs[j, i] + np.uint64(sz if j + 1 == k else 0)
    data = [torch.randint(0, 256, (int(offs[j, n]),), dtype=torch.uint8, device="cuda", generator=g) for j in range(3)]
    mo = np.zeros(n + 1, np.uint64)
    np.cumsum([sz for _, sz in sizes], out=mo[1:])
    total = int(mo[n])
    assert total > rr.RDBMERGE_MAX_WAVES * S
    o = Out(n, total, total + 64)
    types = np.arange(n, dtype=np.uint8)
    engine.rdbmerge(*[(data[j], _offs(offs[j]), _dev(st[j])) for j in range(3)], _dev(types + 50), _dev(types), *o.args(), o.tot[:4])
    torch.cuda.synchronize()
    assert np.array_equal(o.offs.cpu().numpy()[:n + 1].view(np.uint64), mo)
    assert _totals(o.tot) == {"n_elems": 3, "bytes": total, "n_bad": 1, "payload": total}
    for i, (k, sz) in enumerate(sizes):
        if k in (1, 2, 3):
            a, b = int(offs[k - 1, i]), int(mo[i])
            assert torch.equal(o.data[b:b + sz], data[k - 1][a:a + sz]), f"value {i}"
    assert bool((o.data[total:] == CANARY).all())


# ---- alignment ---------------------------------------------------------------------------------------------------------
def test_alignment_matrix(engine):
    """A 100-byte blob at every (source mod 16) x (destination mod 16), from each of the three stages: a padding
    value of the same stage in front moves both, one of another stage moves the destination alone."""
    items, src, dst, seen = [], [3, 5, 11], 0, set()
    for k in (1, 2, 3):
        for s in range(16):
            for d in range(16):
                a = (s - src[k - 1]) % 16 or 16
                b = (d - dst - a) % 16 or 16
                other = k % 3 + 1
                items += [(k, a), (other, b), (k, 100)]
                src[k - 1] += a
                src[other - 1] += b
                dst += a + b
                seen.add((k, src[k - 1] % 16, dst % 16))
                src[k - 1] += 100
                dst += 100
    assert len(seen) == 768
    forged(engine, items, seed=4, lead=(3, 5, 11))


# ---- source patterns -----------------------------------------------------------------------------------------------------
def test_source_patterns(engine):
    rng = np.random.default_rng(5)
    size = lambda: int(rng.integers(6, 200))
    forged(engine, [(1 + i % 3, size()) for i in range(600)], seed=5)           # alternating 1, 2, 3
    runs = []
    for r, ln in enumerate((63, 64, 65, 63, 64, 65, 1, 64)):
        runs += [(1 + r % 3, size()) for _ in range(ln)]
    forged(engine, runs, seed=6)
    forged(engine, [(3, size()) for _ in range(300)], seed=7)                   # everything from the third stage


# ---- capacity ------------------------------------------------------------------------------------------------------------
def test_out_capacity(engine):
    rng = np.random.default_rng(8)
    items = [(1 + int(rng.integers(0, 3)), int(rng.integers(6, 300))) for _ in range(200)] + [(ld.E_TRUNC, 0), (2, 40), (ld.E_LEN, 0)]
    full = forged(engine, items, seed=8)
    total = full[4]["bytes"]
    exact = forged(engine, items, seed=8, data_cap=total)
    assert np.array_equal(exact[3], full[3])
    short = forged(engine, items, seed=8, data_cap=total - 1)                  # only the last value, the offsets as they were
    last = len(items) - 2
    assert short[3][last] == CAP and np.array_equal(np.delete(short[3], last), np.delete(full[3], last))
    assert np.array_equal(short[1], full[1]) and short[4]["payload"] == total - 40
    none = forged(engine, items, seed=8, data_cap=0)                            # sizes only, data NULL
    assert np.array_equal(none[1], full[1]) and none[4]["payload"] == 0 and set(none[3].tolist()) == {CAP, ld.E_TRUNC, ld.E_LEN}


def test_stage_capacity(engine):
    types, data, offs, rev = rule_input()
    full = la.expected_batch(types, data, offs, OPTS)
    total = int(full[1][-1])
    sizing = la.expected_batch(types, data, offs, OPTS, stage_cap=(0, 0, 0), data_cap=0)
    assert sizing[6] == full[6] and np.array_equal(sizing[1], full[1])
    o = loadall(engine, types, data, offs, OPTS, (0, 0, 0), 0, sizing, room=64)   # d_stage_bytes and offsets[n] of the full run
    assert int(o.offs[len(types)]) == total
    caps = (full[6][0], full[6][1] - 1, full[6][2])
    short = la.expected_batch(types, data, offs, OPTS, stage_cap=caps)
    s1 = ld.load_batch(types, data, offs, OPTS)[2]
    s2 = cv.convert_batch(types, data, offs, s1, OPTS)[3]
    last = int(np.nonzero(s2 == 0)[0][-1])
    assert short[3][last] == CAP and np.array_equal(np.delete(short[3], last), np.delete(full[3], last))
    assert np.array_equal(short[1], full[1]) and short[2][last] == full[2][last]
    loadall(engine, types, data, offs, OPTS, caps, total, short)


# ---- refused slices ------------------------------------------------------------------------------------------------------
def test_refused_slices(engine):
    items = [(1, 40), (2, 50), (3, 60), (2, 70), (1, 80), (2, 90), (3, 15)]
    stages = forge(items, seed=9)
    types, conv = np.arange(7, dtype=np.uint8), np.arange(7, dtype=np.uint8) + 20
    d2, o2, s2, c2 = stages[1]
    rev = o2.copy()
    rev[1], rev[2] = o2[2], o2[1]                                              # value 1 reversed (values 0 and 2 hold nothing there)
    want = merge_device(engine, [stages[0], (d2, rev, s2, c2), stages[2]], types, conv)
    assert want[3].tolist() == [0, SLICE, 0, 0, 0, 0, 0] and want[5][0] is not None and want[5][2] is not None
    past = o2.copy()
    past[6:] += np.uint64(1)                                                   # value 5 ends one byte past data_cap
    want = merge_device(engine, [stages[0], (d2, past, s2, c2), stages[2]], types, conv)
    assert want[3].tolist() == [0, 0, 0, 0, 0, SLICE, 0] and int(want[1][-1]) == sum(s for _, s in items) - 90
    want = merge_device(engine, [stages[0], (d2[:c2 - 1], o2, s2, c2 - 1), stages[2]], types, conv)   # the batch itself one byte shorter
    assert want[3].tolist() == [0, 0, 0, 0, 0, SLICE, 0]


# ---- offsets past 2^32 ---------------------------------------------------------------------------------------------------
def test_offsets_past_4gib(engine):
    """Five 900 MiB values alternating between stages 1 and 2, then small ones at 64-bit offsets.  Generated
    (a random block repeated) and compared on the device."""
    free = torch.cuda.mem_get_info()[0]
    if free < 12 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the batch needs 12 GiB")
    big = 900 << 20
    sizes = [(1, big + 1), (2, big), (1, big + 5), (2, big + 2), (1, big), (3, 37), (1, 6), (2, 100)]
    n = len(sizes)
    st = np.zeros((3, n), np.uint8)
    offs = np.zeros((3, n + 1), np.uint64)
    for i, (k, sz) in enumerate(sizes):
        st[:, i] = [(0, SKIP2, SKIP3), (CONV, 0, SKIP3), (CONV, CONV, 0)][k - 1]
        for j in range(3):
            offs[j, i + 1] = offs[j, i] + np.uint64(sz if j + 1 == k else 0)
    g = torch.Generator(device="cuda").manual_seed(11)
    data = []
    for j in range(3):                                                        # random bytes of a period that is no power of two
        nb, period = int(offs[j, n]), (1 << 26) + 13 + 2 * j
        block = torch.randint(0, 256, (min(period, nb),), dtype=torch.uint8, device="cuda", generator=g)
        data.append(block.repeat(nb // period + 1)[:nb].contiguous())
    mo = np.zeros(n + 1, np.uint64)
    np.cumsum([sz for _, sz in sizes], out=mo[1:])
    total = int(mo[n])
    assert int(mo[5]) > 1 << 32
    o = Out(n, total, total + 64)
    types = np.arange(n, dtype=np.uint8)
    engine.rdbmerge(*[(data[j], _offs(offs[j]), _dev(st[j])) for j in range(3)], _dev(types + 50), _dev(types), *o.args(), o.tot[:4])
    torch.cuda.synchronize()
    assert np.array_equal(o.offs.cpu().numpy()[:n + 1].view(np.uint64), mo)
    assert _totals(o.tot) == {"n_elems": 4, "bytes": total, "n_bad": 0, "payload": total}
    assert not o.status.cpu().numpy()[:n].any()
    for i, (k, sz) in enumerate(sizes):
        a, b = int(offs[k - 1, i]), int(mo[i])
        assert torch.equal(o.data[b:b + sz], data[k - 1][a:a + sz]), f"value {i} at {b}"
    assert bool((o.data[total:] == CANARY).all())


# ---- a stream, a graph -----------------------------------------------------------------------------------------------------
def test_one_call_on_a_side_stream(engine):
    types, data, offs, rev = rule_input()
    want = la.expected_batch(types, data, offs, OPTS)
    loadall(engine, types, data, offs, OPTS, want[6], int(want[1][-1]) + 24, want, stream=torch.cuda.Stream())


def decode_buffers(n, nb):
    cap = rr.elem_bound(n, nb)
    z = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")
    return z(16 * n), z(16 * cap), z(nb), torch.zeros(4, dtype=torch.int64, device="cuda")


def flat_of(bufs, n):
    v, e, a, t = bufs
    ne = int(t.cpu().numpy().view(np.uint64)[0])
    return v.cpu().numpy().view(rr.VALUE_DT)[:n], e.cpu().numpy().view(rr.ELEM_DT)[:ne], a.cpu().numpy()


def test_graph_replay_over_a_second_batch():
    """Warm call, then rr_rdbloadall_batch + rr_decode_batch captured and replayed: over canaries, and over a second
    batch of the same shapes (the same sizes, other bytes and scores) copied into the same input buffer."""
    eng = rr.Engine(0)
    try:
        rng = np.random.default_rng(10)
        batches = []
        for b in range(2):
            pays, types = [], []
            for i in range(1500):
                k = i % 5
                if k == 0:
                    types.append(rr.T_STRING), pays.append(raw(bytes(rng.integers(97, 123, 30 + i % 200, dtype=np.uint8))))
                elif k == 1:
                    types.append(HASH), pays.append(b"\x02" + raw(b"f%03d" % (i % 1000)) + raw(b"v" * (i % 9) + bytes([97 + b])) + raw(b"g") + raw(b"%d" % (5000 + i + b)))
                elif k == 2:
                    types.append(ZSET), pays.append(zset([(b"m%d" % j, i % 7 + j + 0.25 + b / 2) for j in range(i % 6 + 1)]))
                elif k == 3:
                    types.append(SET), pays.append(b"\x02" + raw(b"%d" % (10000 + i + b)) + raw(b"%d" % (50000 + i)))
                else:
                    types.append(ZSET), pays.append(zset([(b"k%d" % j, float(20 + j + b)) for j in range(3)]))
            batches.append((np.asarray(types, np.uint8),) + ld.pack(pays))
        assert np.array_equal(batches[0][2], batches[1][2]) and not np.array_equal(batches[0][1], batches[1][1])
        wants = [la.expected_batch(t, d, o) for t, d, o in batches]
        assert wants[0][6] == wants[1][6] and all((w[3] == 0).all() for w in wants)
        n = 1500
        caps = wants[0][6]
        total = int(wants[0][1][-1])
        nb = (total + 15) & ~15
        d_in, d_off, d_ty = _dev(batches[0][1]), _offs(batches[0][2]), _dev(batches[0][0])
        ws = torch.zeros(rr.rdbloadall_ws_bytes(n, caps), dtype=torch.uint8, device="cuda")
        o = Out(n, nb, nb + 64)
        dec = decode_buffers(n, nb)
        eng.reserve(n, nb)

        def chain(stream):
            eng.rdbloadall(d_in, d_off, d_ty, ws, caps, *o.args(), o.sb[:3], o.tot[:4], stream=stream)
            eng.decode_device(o.data[:nb], o.offs[:n + 1], dec[0], dec[1], dec[2], dec[3], stream=stream)

        def canaries():
            o.data.fill_(CANARY), o.offs.fill_(7), o.types.fill_(CANARY), o.status.fill_(CANARY), o.tot.fill_(-3), o.sb.fill_(-5)
            ws.fill_(CANARY)
            for t in dec[:3]:
                t.zero_()

        def verify(k, what):
            o.compare(wants[k], wants[k][6])
            pad = np.concatenate([wants[k][0], np.zeros(nb - total, np.uint8)])
            ov, oe, oa, ot = cpu.decode(pad, wants[k][1])
            gv, ge, ga = flat_of(dec, n)
            assert np.array_equal(gv, ov) and np.array_equal(ge, oe) and np.array_equal(ga[:total], oa[:total]), what
            assert (gv["status"] == 0).all()

        canaries()
        chain(None)                                                            # the warm call: the scratch for every step
        torch.cuda.synchronize()
        verify(0, "warm")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            chain(torch.cuda.current_stream())
        for r in range(2):
            canaries()
            g.replay()
            torch.cuda.synchronize()
            verify(0, f"replay {r}")
        d_in.copy_(torch.from_numpy(batches[1][1].copy()))
        canaries()
        g.replay()
        torch.cuda.synchronize()
        verify(1, "second batch")
    finally:
        eng.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def objects(values, elems, arena):
    """A flat batch as position-free objects: the record without elem_base, the descriptors with their bytes."""
    out = []
    for v in values:
        b, k = int(v["elem_base"]), int(v["n_elems"])
        ds = []
        for e in elems[b:b + k] if int(v["status"]) == 0 else []:
            body = arena[int(e["data"]):int(e["data"]) + int(e["len"])].tobytes() if e["kind"] in (rr.K_STR, rr.K_ZLRAW) else int(e["data"])
            ds.append((int(e["kind"]), int(e["zenc"]), int(e["len"]), body))
        out.append((int(v["type"]), int(v["enc"]), int(v["status"]), int(v["lru"]), k if int(v["status"]) == 0 else 0, ds))
    return out


def test_end_to_end_from_saved_payloads(engine):
    """3,000 mixed values saved by rr_rdbsave_batch, among them Hashes, integer Sets and ZSets with integer and
    fractional scores that convert on load: the one call and one decode give the oracle's objects, and value by
    value the record the three-decode rule picks from the three stage batches."""
    f = ff.Flat(31)
    rng = f.rng
    for i in range(3000):
        k = i % 10
        if k == 0:
            f.add(SET, 0, [b"%d" % int(x) for x in set(rng.integers(-10**6, 10**6, int(rng.integers(1, 9))).tolist())])
        elif k == 1:
            pairs = sorted(((float(int(x)) if i % 20 == 1 else int(x) / 8 + 0.0625, b"m%d" % j)
                            for j, x in enumerate(rng.integers(-99, 99, int(rng.integers(1, 9))))), reverse=True)
            items = []
            for sc, m in pairs:
                items += [m, ("score", zr.to_bits(sc))]
            f.add(rr.T_ZSET_SKIPLIST, 0, items)
        else:
            ff.add_accepted(f, 1)
    v, e, a = f.done()
    types, pdata, poffs, pst, _ = engine.rdbsave_host(v, e, a)
    keep = np.nonzero(pst == 0)[0]                                             # (a ZLRAW-only ziplist is not saveable)
    assert len(keep) > 2700
    pb = pdata.tobytes()
    types = np.ascontiguousarray(types[keep])
    pdata, poffs = ld.pack([pb[int(poffs[i]):int(poffs[i + 1])] for i in keep])
    n = len(types)
    want = la.expected_batch(types, pdata, poffs)
    data, offs, ot, st, sb, tot = engine.rdbloadall_host(pdata, poffs, types)
    assert np.array_equal(data, want[0]) and np.array_equal(offs, want[1]) and np.array_equal(ot, want[2]) and np.array_equal(st, want[3])
    assert tot == want[4] and sb.tolist() == want[6] and tot["n_elems"] > 700 and min(want[6]) > 1000
    got = engine.decode_host(data, offs)
    ora = cpu.decode(want[0], want[1])
    assert np.array_equal(got[0], ora[0]) and np.array_equal(got[1], ora[1]) and np.array_equal(got[2], ora[2])
    merged = objects(*got[:3])
    # the three-decode rule: three stage batches, three decodes over all n values, picked by status
    s1d, s1o, s1s, _ = engine.rdbload_host(pdata, poffs, types)
    s2d, s2o, s2t, s2s, _ = engine.rdbconvert_host(pdata, poffs, types, s1s)
    s3d, s3o, s3s, _ = engine.rdbzset_host(pdata, poffs, types, s2s)
    flats = [objects(*engine.decode_host(d, o)[:3]) for d, o in ((s1d, s1o), (s2d, s2o), (s3d, s3o))]
    picked = [0, 0, 0]
    for i in range(n):
        k = 0 if s1s[i] == 0 else 1 if s2s[i] == 0 else 2
        if (s1s[i], s2s[i], s3s[i])[k] != 0:                                   # no stage holds it: the CPU path's, or corrupt
            assert st[i] != 0 and offs[i] == offs[i + 1]
            continue
        assert st[i] == 0 and merged[i] == flats[k][i], i
        picked[k] += 1
    assert picked[0] > 1000 and picked[1] > 300 and picked[2] > 200, picked   # every stage holds hundreds


# ---- the host form ---------------------------------------------------------------------------------------------------------
def test_host_form(engine):
    types, data, offs, rev = rule_input()
    want = la.expected_batch(types, data, offs, OPTS)
    total = int(want[1][-1])
    co = ld.c_opts(OPTS)
    d, o, ot, st, sb, tot = engine.rdbloadall_host(data, offs, types, co)       # asks for the size first
    assert np.array_equal(d, want[0]) and np.array_equal(o, want[1]) and np.array_equal(ot, want[2]) and np.array_equal(st, want[3])
    assert tot == want[4] and sb.tolist() == want[6]
    d, o, ot, st, sb, tot = engine.rdbloadall_host(data, offs, types, co, out_cap=total)
    assert np.array_equal(d, want[0]) and np.array_equal(st, want[3])
    short = la.expected_batch(types, data, offs, OPTS, data_cap=total - 1)
    d, o, ot, st, sb, tot = engine.rdbloadall_host(data, offs, types, co, out_cap=total - 1)
    last = int(np.nonzero(want[3] == 0)[0][-1])                                # (its bytes in the staging buffer are the call's before)
    cut = int(o[last])
    assert np.array_equal(d[:cut], short[0][:cut]) and len(d) == total - 1 and np.array_equal(o, short[1])
    assert np.array_equal(st, short[3]) and tot == short[4] and (st != want[3]).sum() == 1 and st[last] == CAP
    d, o, ot, st, sb, tot = engine.rdbloadall_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8))
    assert len(d) == 0 and tot == {"n_elems": 0, "bytes": 0, "n_bad": 0, "payload": 0}
