"""rr_rdbsave_batch where tests/test_gpu_rdbsave.py's small synchronous batches do not reach: the
second grid-stride step of every kernel, the rdbSaveLen widths of a List's node count and of a
node's own size, the size parked in the last 8 bytes of the buffer, offsets past 2^32, wave_copy
across source x destination alignment, a side stream and graph replay, and the host entry with a
short data_cap.

Everything is held to tests/rdb_reference.py: directly (check(), from tests/test_gpu_rdbsave.py), or
through flat_forge.tile_expect, which repeats the reference's answer for a 61-value base batch and
is itself held to the reference on the CPU (tests/test_rdbsave.py)."""
import functools

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import flat_forge as ff
import rdb_reference as ref
from helpers import batch_from_blobs, structured_mutations
from test_gpu_rdbsave import CANARY, _dev, check, list_edge_batch

pytestmark = pytest.mark.gpu

WPB = 4             # rr_rdbsave.hip, waves (values in flight) per workgroup
GRID_CAP = 16384    # rr_rdbsave.hip, the grid's cap in workgroups
LIST_GROUP = 8      # rr_rdbsave.hip, values a wave of rdb_list_kernel looks at per step
SHORT_BODY = 32     # rr_stage_device.h, longer bodies go through wave_copy
STRIDE_PLAIN = GRID_CAP * WPB               # values one step of rdb_size_kernel / rdb_emit_kernel covers
STRIDE_LISTS = GRID_CAP * WPB * LIST_GROUP  # and one step of rdb_list_kernel<1> / <2>
L = rr.T_LIST_QUICKLIST


def _letters(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))    # never an integer


@functools.lru_cache(maxsize=None)
def _base():
    """The base batch and the reference's answer for it, computed once."""
    values, elems, arena = ff.tiling_base()
    base_ref, pays = ff.tiling_reference(values, elems, arena)
    for a in (values, elems, arena, *base_ref[:4]):
        a.setflags(write=False)
    return values, elems, arena, base_ref, pays


def _totals(d_tot):
    t = d_tot.cpu().numpy().view(np.uint64)
    return {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])}


def _first_diff(got, want):
    return int(np.nonzero(got != want)[0][0])


def run_tiled(engine, n, cut_at=None):
    """n tiled values through the device call against tile_expect; cut_at: data_cap in the middle of
    that value.  Returns the expected status and types."""
    bv, be, ba, base_ref, pays = _base()
    cap = None
    if cut_at is not None:
        full = ff.tile_expect(bv, base_ref, pays, n)[2]
        assert int(full[cut_at + 1]) - int(full[cut_at]) >= 2
        cap = (int(full[cut_at]) + int(full[cut_at + 1])) // 2
    types, data, offsets, status, totals = ff.tile_expect(bv, base_ref, pays, n, cap)
    total = int(offsets[n])
    if cap is None:
        cap = total                                   # exactly: no slack behind the last value
    room = ((total + 15) & ~15) + 64
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_types = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    engine.rdbsave_device(_dev(ff.tile_records(bv, n)), _dev(be), _dev(ba), out[:cap], d_off, d_types[:n], d_status[:n],
                          d_tot, list_fill=ff.TILE_FILL)
    torch.cuda.synchronize()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), offsets)
    g_status, g_types = d_status.cpu().numpy(), d_types.cpu().numpy()
    assert np.array_equal(g_status[:n], status), f"status differs first at value {_first_diff(g_status[:n], status)}"
    assert np.array_equal(g_types[:n], types)
    assert (g_types[n:] == CANARY).all() and (g_status[n:] == CANARY).all()
    assert _totals(d_tot) == totals
    # offsets never decrease: what is written is everything before the first value that does not fit
    over = np.nonzero(status == rr.E_CAPACITY)[0]
    end = int(offsets[int(over[0])]) if len(over) else total
    want = np.full(room, CANARY, np.uint8)
    want[:end] = data[:end]
    got = out.cpu().numpy()
    if not np.array_equal(got, want):
        at = _first_diff(got, want)
        i = int(np.searchsorted(offsets, at, side="right")) - 1
        raise AssertionError(f"byte {at} (value {i}, base value {i % ff.TILE_BASE}, type {types[min(i, n - 1)]}, offset "
                             f"{at - int(offsets[min(i, n)])}): got {got[at]:#x}, want {want[at]:#x}")
    return status, types


def _cut_after(n, first):
    """The first value at or after `first` that is a saveable List of at least 2 bytes."""
    bv, _, _, base_ref, _ = _base()
    sizes = np.diff(base_ref[2].astype(np.int64))
    return next(i for i in range(first, n) if bv["type"][i % ff.TILE_BASE] == L and sizes[i % ff.TILE_BASE] >= 2)


@pytest.mark.parametrize("cut", [False, True])
def test_second_stride_plain(engine, cut):
    """61 values past what one step of rdb_size_kernel / rdb_emit_kernel covers (a wave a value)."""
    n = STRIDE_PLAIN + ff.TILE_BASE
    cut_at = _cut_after(n, STRIDE_PLAIN + 20) if cut else None
    status, types = run_tiled(engine, n, cut_at)
    second = slice(STRIDE_PLAIN, n)
    assert len(set(types[second].tolist())) == 8 and (status[second] == rr.E_ENCODE).sum() == 1
    if cut:
        assert STRIDE_PLAIN < cut_at < n - 8 and status[cut_at] == rr.E_CAPACITY
        assert (status[cut_at:] != 0).all() and (status[cut_at:] == rr.E_CAPACITY).sum() >= 8
        assert (status[STRIDE_PLAIN:cut_at] == 0).sum() >= 8 and (types[STRIDE_PLAIN:cut_at] == L).any()
    else:
        assert (status[second] == 0).sum() == ff.TILE_BASE - 1


@pytest.mark.parametrize("cut", [False, True])
def test_second_stride_lists(engine, cut):
    """61 values past what one step of rdb_list_kernel covers (LIST_GROUP values a wave): Lists of
    the second step, the accounting (n_elems, n_bad, RR_E_CAPACITY) of its values."""
    n = STRIDE_LISTS + ff.TILE_BASE
    cut_at = _cut_after(n, STRIDE_LISTS + 20) if cut else None
    status, types = run_tiled(engine, n, cut_at)
    lists = np.nonzero(types == L)[0]
    assert (lists < STRIDE_LISTS).any() and (lists >= STRIDE_LISTS).sum() >= 8
    assert len({int(i) % LIST_GROUP for i in lists}) == LIST_GROUP      # every lane position of a group
    if cut:
        assert STRIDE_LISTS < cut_at < n - 8 and status[cut_at] == rr.E_CAPACITY and (status[cut_at:] != 0).all()
        before = lists[(lists >= STRIDE_LISTS) & (lists < cut_at)]
        after = lists[lists > cut_at]
        assert len(before) and (status[before] == 0).all() and len(after) and (status[after] == rr.E_CAPACITY).all()


@pytest.mark.parametrize("fill,counts", [(1, (63, 64, 65, 16383, 16384, 16385)), (0, (16384, 16385))])
def test_node_count_widths(engine, fill, counts):
    """rdbSaveLen of a List's node count at 1 -> 2 and 2 -> 5 bytes: both walks start at
    len_bytes(nodes), so a wrong width shifts the whole payload."""
    f = ff.Flat(21)
    at = []
    for c in counts:
        at.append(f.add(L, 0, [b"a"] * c))                     # fill 0 or 1: a node an entry
        f.add(rr.T_STRING, 0, [b"between"])
    values, elems, arena = f.done()
    payloads = ref.save_batch(values, elems, arena, fill)[5]
    for i, c in zip(at, counts):
        width = 1 if c < 64 else 2 if c < 16384 else 5
        assert payloads[i][:width] == ref.save_len(c) and len(ref.save_len(c)) == width
        assert len(payloads[i]) == width + 15 * c              # rdbSaveLen(14) | a 14-byte node
    st, _ = check(engine, values, elems, arena, fill=fill)
    assert (st == 0).all()


@pytest.mark.parametrize("fill", [-2, -4, -5])
def test_node_size_widths(engine, fill):
    """rdbSaveLen of a node's own size (the parked size decides it in the second walk) at 63 / 64
    and 16383 / 16384 bytes: a node of one entry, and under fill -4 / -5 a node that a second entry
    joins to end on the same sizes."""
    f = ff.Flat(22)
    rng = f.rng
    expect = []
    for body, size in ((50, 63), (51, 64), (16369, 16383), (16370, 16384)):    # 11 + prevlen 1 + header 1 | 2 + body
        items = [_letters(rng, body)]
        expect.append((f.add(L, 0, items), items, [size]))
    if fill != -2:
        # ("ab": 11 + 1 + 1 + 2 = 15; 100 letters: 11 + 1 + 2 + 100 = 114; the joining entry adds prevlen 1 + header + body)
        for first, body, size in ((2, 46, 63), (2, 47, 64), (100, 16266, 16383), (100, 16267, 16384)):
            items = [_letters(rng, first), _letters(rng, body)]
            expect.append((f.add(L, 0, items), items, [size]))
    f.add(rr.T_STRING, 0, [b"behind"])
    values, elems, arena = f.done()
    payloads = ref.save_batch(values, elems, arena, fill)[5]
    for i, items, sizes in expect:
        nodes = ref.list_nodes(items, fill)
        assert [len(z) for z in nodes] == sizes
        assert payloads[i] == b"\x01" + ref.save_len(sizes[0]) + nodes[0]
        assert len(ref.save_len(sizes[0])) == (1 if sizes[0] < 64 else 2 if sizes[0] < 16384 else 5)
    st, _ = check(engine, values, elems, arena, fill=fill)
    assert (st == 0).all()


@pytest.mark.parametrize("lead", [(), (b"abc",), (b"abc", 77, b"")])
def test_exact_capacity_minimal_last_node(engine, lead):
    """The first List walk parks 8 bytes at every node's place; the smallest node, 13 bytes behind
    its 1-byte prefix, as the last thing in a buffer of exactly offsets[n] bytes, canary behind it.
    One byte less and the List gets RR_E_CAPACITY and nothing is written from its offset on."""
    f = ff.Flat(23)
    f.add(rr.T_STRING, 0, [_letters(f.rng, 40)])
    f.add(L, 0, [5])
    f.add(rr.T_SET_HT, 0, [b"m", b"n"])
    last = f.add(L, 0, list(lead) + [5])                       # fill 1: the last node holds the 5 alone
    values, elems, arena = f.done()
    offsets, payloads = ref.save_batch(values, elems, arena, 1)[2::3]
    node = ref.list_nodes([b"5"], 1)[0]
    assert len(node) == 13 and payloads[last].endswith(b"\x0d" + node)
    total = int(offsets[-1])
    st, _ = check(engine, values, elems, arena, fill=1, data_cap=total)
    assert (st == 0).all()
    st, tot = check(engine, values, elems, arena, fill=1, data_cap=total - 1)
    assert (st[:last] == 0).all() and st[last] == rr.E_CAPACITY and tot["n_bad"] == 1


def test_offsets_past_4gib(engine):
    """66,000 Strings of 65,536 bytes over one shared arena string, then the tiled base: Lists and
    every other type at offsets past 2^32.  The 4.3 GB are compared on the device."""
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the batch needs 8 GiB")
    bv, be, ba, _, _ = _base()
    nbig, blen = 66000, 65536
    big = np.zeros(1, rr.VALUE_DT)
    big["type"], big["enc"], big["n_elems"], big["elem_base"] = rr.T_STRING, 0, 1, len(be)
    elems = np.concatenate([be, np.array([(len(ba), blen, rr.K_STR, 0, 0)], dtype=rr.ELEM_DT)])
    arena = np.concatenate([ba, np.frombuffer(_letters(np.random.default_rng(24), blen), np.uint8)])
    # the reference on one big String and the base; the other 65,999 are the same record
    types1, data1, offs1, status1, tot1, pay1 = ref.save_batch(np.concatenate([big, bv]), elems, arena, ff.TILE_FILL)
    tot_big = ref.save_batch(big, elems, arena, ff.TILE_FILL)[4]
    row = int(offs1[1])
    assert row == 5 + blen and pay1[0][:5] == b"\x80\x00\x01\x00\x00"
    n = nbig + len(bv)
    offsets = np.concatenate([np.arange(nbig - 1, dtype=np.uint64) * np.uint64(row), offs1 + np.uint64((nbig - 1) * row)])
    total = int(offsets[n])
    assert int(offsets[nbig]) > 1 << 32 and total == (nbig - 1) * row + int(offs1[-1])
    totals = {k: tot1[k] + (nbig - 1) * tot_big[k] for k in ("n_elems", "bytes", "payload")}
    totals["n_bad"] = tot1["n_bad"]
    room = ((total + 15) & ~15) + 64
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_types = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    engine.rdbsave_device(_dev(np.concatenate([np.tile(big, nbig), bv])), _dev(elems), _dev(arena), out[:total], d_off,
                          d_types[:n], d_status[:n], d_tot, list_fill=ff.TILE_FILL)
    torch.cuda.synchronize()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), offsets)
    assert _totals(d_tot) == totals
    g_status, g_types = d_status.cpu().numpy(), d_types.cpu().numpy()
    assert not g_status[:nbig].any() and np.array_equal(g_status[nbig:n], status1[1:])
    assert (g_types[:nbig] == rr.T_STRING).all() and np.array_equal(g_types[nbig:n], types1[1:])
    assert (g_types[n:] == CANARY).all() and (g_status[n:] == CANARY).all()
    rows = out[:nbig * row].view(nbig, row)
    assert np.array_equal(rows[0].cpu().numpy(), data1[:row])
    for r0 in range(0, nbig, 8192):                            # (in pieces: the comparison's result is a byte an element)
        same = (rows[r0:r0 + 8192] == rows[0]).all(dim=1)
        assert bool(same.all()), f"row {r0 + int((~same).nonzero()[0])} differs from row 0"
    tail = out[nbig * row:].cpu().numpy()
    want = np.full(room - nbig * row, CANARY, np.uint8)
    want[:len(data1) - row] = data1[row:]
    if not np.array_equal(tail, want):
        at = _first_diff(tail, want)
        raise AssertionError(f"byte {nbig * row + at} (base offset {at}): got {tail[at]:#x}, want {want[at]:#x}")


def _alignment_batch(pads):
    """Bodies that wave_copy moves, in Lists and SET_HTs: source alignment 0..15 (the arena padded)
    x destination shift (a leading filler entry / member of 0..16 letters: 17, since a List node that
    reaches 64 bytes takes a second prefix byte, which moves every longer filler by one more).  A String
    after each value brings the next value's offset to a multiple of 16 (pads: its length per
    value, from a first build without them).  Returns the batch, the value indices and the
    (source alignment, body) of each."""
    f = ff.Flat(25)
    rng = f.rng
    at, meta = [], []
    combos = [(ln, a, s) for ln in (33, 48, 49) for a in range(16) for s in range(17)]
    combos += [(ln, a, s) for ln in (1039, 1040, 1071) for a in (0, 1, 7, 15) for s in range(17)]
    for typ in (L, rr.T_SET_HT):
        for ln, a, s in combos:
            f.arena += bytes((a - len(f.arena)) % 16)
            body = _letters(rng, ln)
            src = len(f.arena)
            f.arena += body
            at.append(f.add(typ, 0, [_letters(rng, s), ("raw", rr.K_STR, src, ln, 0, 0)]))
            meta.append((a, body))
            f.add(rr.T_STRING, 0, [b"p" * (pads[len(at) - 1] if pads else 0)])
    return f.done(), at, meta


def test_wave_copy_alignment_matrix(engine):
    """wave_copy's head / 16-byte body / tail split at every source x destination alignment for the
    lengths around SHORT_BODY and one 16-byte step (33, 48, 49), and its loop's second trip (a body
    of 1024 bytes and more behind the head: 1039, 1040, 1071)."""
    (values, elems, arena), at, _ = _alignment_batch(None)
    sizes = np.diff(ref.save_batch(values, elems, arena)[2].astype(np.int64))
    pads = [int(15 - sizes[i]) % 16 for i in at]               # value | rdbSaveLen 1 + pad letters = 0 mod 16
    (values, elems, arena), at, meta = _alignment_batch(pads)
    offsets, payloads = ref.save_batch(values, elems, arena)[2::3]
    seen = {}
    for i, (a, body) in zip(at, meta):
        assert int(offsets[i]) % 16 == 0 and int(elems["data"][int(values["elem_base"][i]) + 1]) % 16 == a
        dst = int(offsets[i]) + payloads[i].index(body)        # the out tensor is 16-byte aligned, so is the arena
        seen.setdefault((int(values["type"][i]), len(body)), set()).add((a, dst % 16))
    for typ in (L, rr.T_SET_HT):
        for ln in (33, 48, 49):
            assert len(seen[(typ, ln)]) == 256
        for ln in (1039, 1040, 1071):
            assert len(seen[(typ, ln)]) == 64
    st, _ = check(engine, values, elems, arena)
    assert (st == 0).all()


def _mixed_with_rejects(config, n, seed):
    """n blobs of a generated batch, every seventh replaced by a structured mutant of itself."""
    data, offs = rr.gen_batch(config, n, seed=seed)
    blobs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(n)]
    pick = list(range(3, n, 7))
    d7, o7 = batch_from_blobs([blobs[i] for i in pick])
    for i, m in zip(pick, structured_mutations(d7, o7, seed + 1, per_value=1)):
        blobs[i] = m
    return batch_from_blobs(blobs)


def test_side_stream_and_graph_replay():
    """decode -> rdbsave on one non-default stream with nothing between them, then the same two
    calls captured in a graph and replayed: over canaries, and over a second batch (another config,
    malformed blobs among it) copied into the same input buffers.  The size kernel zeroes what the
    other launches rely on, so every replay must equal the reference on the host decode."""
    eng = rr.Engine(0)
    try:
        n = 6000
        data, offs = rr.gen_batch(4, n, seed=5151)
        data2, offs2 = _mixed_with_rejects(1, n, 5152)
        hosts = [rr.host_decode(d, o)[:3] for d, o in ((data, offs), (data2, offs2))]
        refs = [ref.save_batch(*h) for h in hosts]
        assert (refs[0][3] == 0).all() and (refs[1][3] == rr.E_ENCODE).any() and (refs[1][3] == 0).any()
        nb = (max(int(offs[-1]), int(offs2[-1])) + 15) & ~15
        cap = max(rr.elem_bound(n, int(offs[-1])), rr.elem_bound(n, int(offs2[-1])))
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

        def load(dd, oo):
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

        def verify(k, what):
            types, data_ref, offsets, status, totals, _ = refs[k]
            assert np.array_equal(o_off.cpu().numpy().view(np.uint64), offsets), what
            assert np.array_equal(o_st.cpu().numpy()[:n], status), what
            assert np.array_equal(o_ty.cpu().numpy()[:n], types), what
            assert (o_ty.cpu().numpy()[n:] == CANARY).all() and (o_st.cpu().numpy()[n:] == CANARY).all(), what
            assert _totals(o_tot) == totals, what
            got = out.cpu().numpy()
            total = int(offsets[-1])
            assert np.array_equal(got[:total], data_ref), f"{what}: first at byte {_first_diff(got[:total], data_ref)}"
            assert (got[total:] == CANARY).all(), what

        def chain(stream):
            eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=stream)
            eng.rdbsave_device(d_vals, d_elems, d_arena, out[:room - 64], o_off, o_ty[:n], o_st[:n], o_tot, stream=stream)

        load(data, offs)
        canaries()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain(s)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        verify(0, "side stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                              # one stream, the five + decode's launches in a line
            chain(torch.cuda.current_stream())
        for r in range(3):
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


def test_host_entry_short_capacity_and_empty(engine):
    """rr_rdbsave_batch_host with data_cap inside the first, a middle and the last value, and an
    empty batch.  (Bytes of ranges that were not written are unspecified on this path.)"""
    values, elems, arena = list_edge_batch()
    n = len(values)
    full = ref.save_batch(values, elems, arena)[2]
    for i in (0, n // 2, n - 1):
        cut = (int(full[i]) + int(full[i + 1])) // 2
        types, _, offsets, status, totals, payloads = ref.save_batch(values, elems, arena, data_cap=cut)
        assert status[i] == rr.E_CAPACITY and (status[:i] == 0).all()
        g_types, g_data, g_off, g_status, g_tot = engine.rdbsave_host(values, elems, arena, data_cap=cut)
        assert np.array_equal(g_off, offsets) and np.array_equal(g_status, status) and np.array_equal(g_types, types)
        assert g_tot == totals and len(g_data) == cut
        for j in np.nonzero(status == 0)[0]:
            o = int(offsets[j])
            assert bytes(g_data[o:o + len(payloads[j])]) == payloads[j], f"cut in value {i}: value {j}"
    none_e, none_a = np.zeros(0, rr.ELEM_DT), np.zeros(0, np.uint8)
    want = ref.save_batch(values[:0], none_e, none_a)
    assert want[4] == {"n_elems": 0, "bytes": 0, "n_bad": 0, "payload": 0}
    for cap in (None, 0, 100):
        g_types, g_data, g_off, g_status, g_tot = engine.rdbsave_host(values[:0], none_e, none_a, data_cap=cap)
        assert len(g_types) == len(g_status) == len(g_data) == 0
        assert np.array_equal(g_off, want[2]) and g_off.tolist() == [0] and g_tot == want[4]
