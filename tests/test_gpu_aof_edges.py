"""rr_aof_batch on the batches of tests/aof_shapes.py, against tests/aof_reference.py through
test_gpu_aof.check: every byte, offset, status and total, canaries behind and between what the call
may write, and the bound.  What the shapes are for: the device build of the score parser on a different
text in every lane; a lane's state words after a long number, inside a value and across the values of
one wave; the 24-bit pieces of scan_costs and sum_lanes; offsets past 2^32; wave_copy at every source x
destination alignment, for bodies and for the key; every digit seam of "$len" and "*argc"; the intset
widths' range rule; RR_E_ENCODE before RR_AOF_E_CPU whatever the round; the host entry point's
arguments; and decode -> rr_aof_batch captured in a graph and replayed on the same scratch.
tests/test_aof_shapes.py holds the shapes to account on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import aof_reference as ar
import aof_shapes as sh
from helpers import batch_from_blobs
from test_gpu_aof import CANARY, _dev, check
from test_gpu_rdbsave_scale import _mixed_with_rejects

pytestmark = pytest.mark.gpu


def run(engine, s, **kw):
    return check(engine, s.values, s.elems, s.arena, s.names, expires=s.expires, **kw)


# ---- A ----------------------------------------------------------------------------------------------------
def test_score_texts_in_every_lane(engine):
    st, _, _ = run(engine, sh.score_text_batch())
    assert (st == 0).all()


def test_score_integers(engine):
    st, _, _ = run(engine, sh.score_int_batch())
    assert (st == 0).all()


def test_every_refused_text(engine):
    s = sh.refused_batch()
    st, tot, slices = run(engine, s)
    assert (st[0::2] == rr.AOF_E_CPU).all() and (st[1::2] == 0).all() and tot["n_bad"] == len(sh.REFUSED)
    assert all(c.startswith(b"*3\r\n$3\r\nSET\r\n") for c in slices[1::2])


# ---- B ----------------------------------------------------------------------------------------------------
def test_stale_state_across_rounds(engine):
    st, _, _ = run(engine, sh.stale_rounds_batch())
    assert (st == 0).all()


def test_stale_state_across_values(engine):
    st, _, _ = run(engine, sh.stale_values_batch())
    assert (st == 0).all()


# ---- C ----------------------------------------------------------------------------------------------------
def test_costs_past_24_bits(engine):
    st, tot, _ = run(engine, sh.seam24_batch())
    assert (st == 0).all() and tot["payload"] > sh.SEAM


# ---- D ----------------------------------------------------------------------------------------------------
def test_offsets_past_4gib(engine):
    """NBIG Strings of 65,536 bytes over one shared descriptor, then every aggregate encoding with 130 items
    and an expiry at offsets past 2^32.  The 4.3 GB are compared on the device against row 0."""
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the batch needs 8 GiB")
    s = sh.past_4gib_batch()
    nbig, ntail = sh.NBIG, len(s.values) - 1
    data1, offs1, status1, tot1, _ = sh.reference(s)
    tot_big = sh.reference(sh.Shape(s.values[:1], s.elems, s.arena, s.names[:1], s.expires[:1], {}))[3]
    offsets, totals = sh.past_4gib_expect(offs1, tot1, tot_big, ntail)
    n, row, total = nbig + ntail, int(offs1[1]), int(offsets[-1])
    assert int(offsets[nbig]) > 1 << 32 and (status1 == 0).all()
    values = np.concatenate([np.tile(s.values[:1], nbig), s.values[1:]])
    kd = np.frombuffer(b"k" * nbig + b"".join(s.names[1:]), np.uint8)
    ko = np.arange(n + 1, dtype=np.int64)
    exp = np.concatenate([np.full(nbig, -1, np.int64), np.asarray(s.expires[1:], np.int64)])
    room = ((total + 15) & ~15) + 64
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    engine.aof(_dev(values), _dev(s.elems), _dev(s.arena), _dev(kd), torch.from_numpy(ko).cuda(), out[:total], d_off,
               d_status[:n], d_tot, expires=torch.from_numpy(exp).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), offsets)
    t = d_tot.cpu().numpy().view(np.uint64)
    assert {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])} == totals
    gs = d_status.cpu().numpy()
    assert not gs[:n].any() and (gs[n:] == CANARY).all()
    rows = out[:nbig * row].view(nbig, row)
    assert np.array_equal(rows[0].cpu().numpy(), data1[:row])
    for r0 in range(0, nbig, 8192):                            # (in pieces: the comparison's result is a byte an element)
        same = (rows[r0:r0 + 8192] == rows[0]).all(dim=1)
        assert bool(same.all()), f"row {r0 + int((~same).nonzero()[0])} differs from row 0"
    tail = out[nbig * row:].cpu().numpy()
    want = np.full(room - nbig * row, CANARY, np.uint8)
    want[:len(data1) - row] = data1[row:]
    if not np.array_equal(tail, want):
        at = int(np.nonzero(tail != want)[0][0])
        raise AssertionError(f"byte {nbig * row + at} (tail offset {at}): got {tail[at]:#x}, want {want[at]:#x}")
    assert total <= rr.aof_bound(n, int(values["n_elems"].sum()), nbig * sh.BIG_LEN + int(s.elems["len"].sum()), n)


# ---- E ----------------------------------------------------------------------------------------------------
def test_body_alignment_matrix(engine):
    st, _, _ = run(engine, sh.body_alignment())
    assert (st == 0).all()


def test_key_alignment_matrix(engine):
    st, _, _ = run(engine, sh.key_alignment_batch())
    assert (st == 0).all()


# ---- F ----------------------------------------------------------------------------------------------------
def test_digit_seams(engine):
    st, _, slices = run(engine, sh.digit_seam_batch())
    s = sh.digit_seam_batch()
    assert (st == 0).all() and slices[0].endswith(b"PEXPIREAT\r\n$2\r\nk0\r\n$20\r\n-9223372036854775808\r\n")
    assert all(ar.parse_resp(c)[-1] == [b"PEXPIREAT", k, b"%d" % x] for c, k, x in zip(slices, s.names, s.expires))


# ---- G ----------------------------------------------------------------------------------------------------
def test_intset_width_limits(engine):
    s = sh.intset_batch()
    st, tot, _ = run(engine, s)
    bad = s.meta["bad"]
    assert (st[bad] == rr.E_ENCODE).all() and tot["n_bad"] == len(bad) == int((st != 0).sum())


# ---- H ----------------------------------------------------------------------------------------------------
def test_precedence_across_rounds(engine):
    s = sh.precedence_batch()
    st, _, _ = run(engine, s)
    assert (st[s.meta["encode"]] == rr.E_ENCODE).all() and (st[s.meta["cpu"]] == rr.AOF_E_CPU).all()
    assert int((st != 0).sum()) == len(s.meta["encode"]) + len(s.meta["cpu"])


# ---- I ----------------------------------------------------------------------------------------------------
def host_equals(engine, s, data_cap=None, key_bytes=None, expires="own"):
    kd, ko = ar.keys_of(s.names)
    exp = s.expires if expires == "own" else expires
    exp = None if exp is None else np.asarray(exp, np.int64)
    data, offs, status, totals, slices = ar.aof_batch(s.values, s.elems, s.arena, kd, ko, exp, data_cap, key_bytes)
    out, ooffs, st, tot = engine.aof_host(s.values, s.elems, s.arena, kd, ko, exp, data_cap=data_cap, key_bytes=key_bytes)
    assert np.array_equal(ooffs, offs) and np.array_equal(st, status) and tot == totals
    assert len(out) == len(data) == min(int(offs[-1]), int(offs[-1]) if data_cap is None else data_cap)
    for i, c in enumerate(slices):                             # up to the cap: what the values that fit wrote
        o = int(offs[i])
        assert bytes(out[o:o + len(c)]) == c, i
    return status


def test_host_entry_capacities_and_keys(engine):
    s = sh.capacity_batch()._replace(expires=[1700000000000 + i if i % 2 else -1 for i in range(9)])
    total = int(sh.reference(s)[1][-1])
    st = host_equals(engine, s, data_cap=0)
    assert st[0] == 0 and (st[1:] == rr.E_CAPACITY).all()
    st = host_equals(engine, s, data_cap=total - 1)
    assert (st[:-1] == 0).all() and st[-1] == rr.E_CAPACITY
    assert (host_equals(engine, s, data_cap=total) == 0).all()
    assert (host_equals(engine, s) == 0).all()
    assert (host_equals(engine, s, expires=None) == 0).all()
    keys = sum(len(k) for k in s.names)
    st = host_equals(engine, s, key_bytes=keys - 1)
    assert (st[:-1] == 0).all() and st[-1] == rr.RDBFILE_E_KEY
    empty = sh.Shape(s.values[:0], s.elems, s.arena, [], None, {})
    out, offs, st, tot = engine.aof_host(empty.values, empty.elems, empty.arena, *ar.keys_of([]))
    assert len(out) == 0 and offs.tolist() == [0] and len(st) == 0 and tot == {"n_elems": 0, "bytes": 0, "n_bad": 0, "payload": 0}


def test_refused_arguments_write_nothing(engine):
    """The NULL-argument and misaligned out->data refusals of rr_aof_batch: RR_API_EINVAL, nothing written."""
    L = rr.lib()
    s = sh.capacity_batch()
    n = len(s.values)
    kd, ko = ar.keys_of(s.names)
    d = [_dev(s.values), _dev(s.elems), _dev(s.arena), _dev(kd), torch.from_numpy(ko.view(np.int64).copy()).cuda()]
    out = torch.full((4096 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    assert out.data_ptr() % 16 == 0
    inb = rr.FlatBatch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, len(s.elems), len(s.arena))
    kb = rr.BlobBatch(d[3].data_ptr(), d[4].data_ptr(), n, len(kd))
    vp = C.c_void_p
    ctx, st, tot = engine._ctx, vp(d_status.data_ptr()), vp(d_tot.data_ptr())

    def outb(data=out.data_ptr(), offsets=d_off.data_ptr(), count=n, cap=4096):
        return C.byref(rr.BlobBatch(data, offsets, count, cap))

    torch.cuda.synchronize()
    EINVAL = rr.API_EINVAL
    calls = [(None, C.byref(inb), C.byref(kb), outb(), st, tot),
             (ctx, None, C.byref(kb), outb(), st, tot),
             (ctx, C.byref(inb), None, outb(), st, tot),
             (ctx, C.byref(inb), C.byref(kb), None, st, tot),
             (ctx, C.byref(inb), C.byref(kb), outb(), st, None),
             (ctx, C.byref(inb), C.byref(kb), outb(), None, tot),                          # status, n != 0
             (ctx, C.byref(inb), C.byref(kb), outb(offsets=None), st, tot),
             (ctx, C.byref(inb), C.byref(rr.BlobBatch(d[3].data_ptr(), None, n, len(kd))), outb(), st, tot),
             (ctx, C.byref(inb), C.byref(kb), outb(data=None), st, tot),                   # data_cap without data
             (ctx, C.byref(inb), C.byref(kb), outb(count=n - 1), st, tot),
             (ctx, C.byref(inb), C.byref(kb), outb(data=out.data_ptr() + 8), st, tot),     # misaligned
             (ctx, C.byref(inb), C.byref(kb), outb(data=out.data_ptr() + 1), st, tot)]
    for k, (c, i, ky, o, s_, t_) in enumerate(calls):
        assert L.rr_aof_batch(c, i, ky, None, o, s_, t_, None) == EINVAL, k
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (d_off == 7).all() and (d_status == CANARY).all() and (d_tot == -3).all()
    # the control: the arguments every refused call was one step away from are taken
    assert L.rr_aof_batch(ctx, C.byref(inb), C.byref(kb), None, outb(), st, tot, None) == 0
    torch.cuda.synchronize()
    want = ar.aof_batch(s.values, s.elems, s.arena, kd, ko, None, 4096)
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want[1]) and np.array_equal(d_status.cpu().numpy()[:n], want[2])
    assert (want[2] == 0).any() and (out[4096:] == CANARY).all()
    hv, he, ha = (np.ascontiguousarray(x) for x in s[:3])
    offs, stat, data = np.full(n + 1, 7, np.uint64), np.full(n, CANARY, np.uint8), np.full(64, CANARY, np.uint8)
    p = lambda a: a.ctypes.data_as(vp)
    full = [ctx, p(hv), p(he), len(he), p(ha), ha.size, n, p(kd), p(ko), len(kd), None, p(data), 64, p(offs), p(stat), None]
    for k in (0, 1, 2, 4, 7, 8, 11, 13, 14):                   # each pointer the call needs, NULL in turn
        args = list(full)
        args[k] = None
        assert L.rr_aof_batch_host(*args) == EINVAL, k
    assert (offs == 7).all() and (stat == CANARY).all() and (data == CANARY).all()
    assert L.rr_aof_batch_host(*full) == 0                     # the control
    want = ar.aof_batch(s.values, s.elems, s.arena, kd, ko, None, 64)
    assert np.array_equal(offs, want[1]) and np.array_equal(stat, want[2]) and (want[2] == 0).any()


def test_side_stream_and_graph_replay():
    """decode -> rr_aof_batch on one non-default stream, then the two calls captured in a graph and replayed:
    over canaries, and over a second batch (another config, malformed blobs and ZSets with refused score
    texts among it) copied into the same input buffers.  The size kernel zeroes the scan's look-back words,
    the error word and the totals, so every replay equals the reference on the host decode."""
    eng = rr.Engine(0)
    try:
        n = 3000
        data, offs = rr.gen_batch(4, n, seed=6161)
        d2, o2 = _mixed_with_rejects(1, n, 6162)
        blobs = [bytes(d2[o2[i]:o2[i + 1]]) for i in range(n)]
        extra = sh.refused_blobs()
        for k, b in enumerate(extra * 5):
            blobs[11 + 97 * k] = b
        data2, offs2 = batch_from_blobs(blobs)
        names = [b"key:%d" % i for i in range(n)]
        kd, ko = ar.keys_of(names)
        exp = np.array([-1 if i % 3 else 1650000000000 + i for i in range(n)], np.int64)
        nb = (max(int(offs[-1]), int(offs2[-1])) + 15) & ~15
        cap = max(rr.elem_bound(n, int(offs[-1])), rr.elem_bound(n, int(offs2[-1])))
        hosts = [rr.host_decode(d, o)[:3] for d, o in ((data, offs), (data2, offs2))]
        refs = [ar.aof_batch(v, e, a, kd, ko, exp) for v, e, a in hosts]
        assert (refs[0][2] == 0).all() and len(set(refs[1][2].tolist())) == 3 and (refs[1][2] == rr.AOF_E_CPU).sum() == 15
        room = ((max(int(r[1][-1]) for r in refs) + 15) & ~15) + 64
        dev = torch.device("cuda:0")
        d_data = torch.zeros(nb, dtype=torch.uint8, device=dev)
        d_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_vals = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_elems = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
        d_arena = torch.zeros(nb, dtype=torch.uint8, device=dev)
        d_tot = torch.zeros(4, dtype=torch.int64, device=dev)
        d_kd, d_ko, d_exp = _dev(kd), torch.from_numpy(ko.view(np.int64).copy()).to(dev), torch.from_numpy(exp).to(dev)
        out = torch.zeros(room, dtype=torch.uint8, device=dev)
        o_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        o_st = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
        o_tot = torch.zeros(4, dtype=torch.int64, device=dev)
        eng.reserve(n, nb)

        def load(dd, oo):
            d_data.zero_()
            d_data[:dd.size].copy_(torch.from_numpy(dd))
            d_offs.copy_(torch.from_numpy(oo.view(np.int64)))

        def canaries():
            for t in (out, o_st):
                t.fill_(CANARY)
            d_vals.zero_()
            d_elems.zero_()
            o_off.fill_(7)
            o_tot.fill_(-3)

        def verify(k, what):
            _, offsets, status, totals, slices = refs[k]
            assert np.array_equal(o_off.cpu().numpy().view(np.uint64), offsets), what
            gs = o_st.cpu().numpy()
            assert np.array_equal(gs[:n], status) and (gs[n:] == CANARY).all(), what
            t = o_tot.cpu().numpy().view(np.uint64)
            assert {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])} == totals, what
            want = np.full(room, CANARY, np.uint8)
            for i, c in enumerate(slices):
                o = int(offsets[i])
                want[o:o + len(c)] = np.frombuffer(c, np.uint8)
            got = out.cpu().numpy()
            assert np.array_equal(got, want), f"{what}: first at byte {int(np.nonzero(got != want)[0][0])}"

        def chain(stream):
            eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=stream)
            eng.aof(d_vals, d_elems, d_arena, d_kd, d_ko, out[:room - 64], o_off, o_st[:n], o_tot, expires=d_exp, stream=stream)

        load(data, offs)
        canaries()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain(s)                                           # the eager call that warms the context's scratch
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        verify(0, "side stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                              # one stream, the launches in a line
            chain(torch.cuda.current_stream())
        for r in range(2):
            canaries()
            g.replay()
            torch.cuda.synchronize()
            verify(0, f"replay {r}")
        load(data2, offs2)
        for r in range(2):
            canaries()
            g.replay()
            torch.cuda.synchronize()
            verify(1, f"second batch, replay {r}")
    finally:
        eng.close()
