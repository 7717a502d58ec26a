"""rr_rdbsave_batch on the GPU against tests/rdb_reference.py: every payload byte for byte, types,
offsets, status and totals, the bound, and a canary behind and between what the call may write.

The batches are the smallest that reach the kernels' edges: the rdbSaveLen widths, the integer rule,
List nodes that close on and past the limit, the prevlen 1 -> 5 step, node boundaries inside and at
the edge of a 64-entry round, and forged values (tests/flat_forge.py) that must be refused."""
import struct

import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import flat_forge as ff
import rdb_reference as ref
from helpers import batch_from_blobs, golden

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INT_RULE = [b"0", b"-0", b"127", b"128", b"-128", b"-129", b"32767", b"32768", b"2147483647", b"2147483648",
            b"-2147483648", b"-2147483649", b"01", b"+1", b" 1", b"1 ", b"", b"12\x00"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def check(engine, values, elems, arena, fill=-2, data_cap=None, bounded=True):
    """Run the device call on a canary-filled buffer and compare everything with the reference."""
    n = len(values)
    types, _, offsets, status, totals, payloads = ref.save_batch(values, elems, arena, fill, data_cap)
    total = int(offsets[-1])
    cap = total + 48 if data_cap is None else data_cap
    room = ((max(cap, total) + 15) & ~15) + 64
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    d_types = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    engine.rdbsave_device(_dev(values), _dev(elems), _dev(arena), out[:cap], d_off, d_types[:n], d_status[:n], d_tot,
                          list_fill=fill)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), offsets)
    assert np.array_equal(d_status.cpu().numpy()[:n], status)
    assert np.array_equal(d_types.cpu().numpy()[:n], types)
    assert (d_types.cpu().numpy()[n:] == CANARY).all() and (d_status.cpu().numpy()[n:] == CANARY).all()
    t = d_tot.cpu().numpy().view(np.uint64)
    assert {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])} == totals
    want = np.full(room, CANARY, np.uint8)
    for i, p in enumerate(payloads):
        if status[i] == 0:
            o = int(offsets[i])
            want[o:o + len(p)] = np.frombuffer(p, np.uint8)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        i = int(np.searchsorted(offsets, at, side="right")) - 1
        raise AssertionError(f"byte {at} (value {i}, type {types[min(i, n - 1)] if n else None}, offset "
                             f"{at - int(offsets[min(i, n)])}): got {got[at]:#x}, want {want[at]:#x}")
    if bounded:
        assert total <= rr.rdbsave_bound(values, elems)
    else:
        # forged values share and overrun descriptor ranges, so len(elems) undercounts: the bound from
        # what a C caller passes, the values' own n_elems and the STR / ZLRAW bytes they name
        ne = pay = 0
        for _, descs in ref.flat_values(values, elems, arena):
            if descs is not None:
                ne += len(descs)
                pay += sum(d[2] for d in descs if d[0] in (rr.K_STR, rr.K_ZLRAW))
        assert total <= int(rr.lib().rr_rdbsave_bound(n, ne, pay))
    return status, totals


def flat_of(blobs, flags=0):
    data, offs = batch_from_blobs(blobs)
    return rr.host_decode_ex(data, offs, flags)[:3]


def golden_blobs():
    g = golden()
    return [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]


def test_goldens(engine):
    st, _ = check(engine, *flat_of(golden_blobs()))
    assert (st == 0).any() and (st == rr.E_ENCODE).any()     # the edges hold malformed blobs too


@pytest.mark.parametrize("config", [1, 2, 3, 4])
def test_generated(engine, config):
    data, offs = rr.gen_batch(config, 4000)
    values, elems, arena, _ = rr.host_decode(data, offs)
    st, _ = check(engine, values, elems, arena)
    assert (st == 0).all()


def test_strings(engine):
    f = ff.Flat(1)
    for s in INT_RULE:
        f.add(rr.T_STRING, 0 if len(s) > 44 else 8, [s])
    for ln in (0, 11, 12, 20, 21, 63, 64, 16383, 16384, 70000):
        f.add(rr.T_STRING, 0, [bytes(f.rng.integers(97, 123, ln, dtype=np.uint8))])
    for a in range(16):                     # every source alignment, short and long bodies
        for ln in (5, 33, 200):
            f.arena += bytes((a - len(f.arena)) % 16)
            at = len(f.arena)
            f.arena += bytes(f.rng.integers(97, 123, ln, dtype=np.uint8))
            f.add(rr.T_STRING, 0, [("raw", rr.K_STR, at, ln, 0, 0)])
    for x in (0, 12, 13, -1, 127, 128, -128, -129, 32767, 32768, 2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**63 - 1, -2**63):
        f.add(rr.T_STRING, 1, [x])
    st, _ = check(engine, *f.done())
    assert (st == 0).all()


def _word(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))    # letters: never an integer


def list_edge_batch():
    f = ff.Flat(2)
    rng = f.rng
    L = rr.T_LIST_QUICKLIST
    f.add(L, 0, [_word(rng, 200), _word(rng, 7971)])          # new_sz 8192: joins
    f.add(L, 0, [_word(rng, 200), _word(rng, 7972)])          # new_sz 8193: a new node
    f.add(L, 0, [_word(rng, 8000), _word(rng, 173), b"", b""])   # the estimate below the real size
    f.add(L, 0, [_word(rng, 9000)])                            # longer than the limit, alone
    f.add(L, 0, [b"a", _word(rng, 9000), b"b", b"c"])          # and mid-list
    for sz in (63, 64, 253, 254, 16383, 16384):
        f.add(L, 0, [b"p", _word(rng, sz), b"q", _word(rng, sz), b"r"])
    for body in range(249, 254):                               # raw length 252..256: prevlen 1 -> 5
        f.add(L, 0, [_word(rng, body), b"s", 5, _word(rng, body), 300, b"t"])
    ints = [0, 12, 13, -1, 127, 128, -128, -129, 32767, 32768, -32768, -32769, 2**23 - 1, 2**23, -2**23, -2**23 - 1,
            2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**63 - 1, -2**63]
    ints += [10**k for k in range(19)] + [-10**k for k in range(19)]   # 1..20 characters
    f.add(L, 0, ints)
    f.add(L, 0, [str(x).encode() for x in ints])               # STR descriptors that zipTryEncoding takes
    f.add(L, 0, [b"007", b"-0", b"1" * 31, b"1" * 32, b"9223372036854775808"])   # and ones it does not
    for cnt in (0, 1, 63, 64, 65):
        f.add(L, 0, [_word(rng, int(rng.integers(1, 40))) for _ in range(cnt)])
    f.add(L, 0, [_word(rng, 126)] * 63 + [b"z"] * 3)          # 63 * 128 + 11 = 8075: the node closes in round 2
    f.add(L, 0, [_word(rng, int(rng.integers(0, 60))) if k % 3 else int(rng.integers(-70000, 70000))
                 for k in range(5000)])
    return f.done()


def test_list_node_edges(engine):
    st, _ = check(engine, *list_edge_batch())
    assert (st == 0).all()


@pytest.mark.parametrize("fill", [-1, -5, 0, 1, 3, 32767, -9, 40000])
def test_list_fill(engine, fill):
    f = ff.Flat(3)
    rng = f.rng
    for cnt, hi in ((300, 40), (40, 600), (9, 9000), (700, 3)):
        f.add(rr.T_LIST_QUICKLIST, 0, [_word(rng, int(rng.integers(0, hi))) if k % 4 else int(rng.integers(-300, 300))
                                       for k in range(cnt)])
    f.add(rr.T_STRING, 0, [b"between"])
    st, _ = check(engine, *f.done(), fill=fill)
    assert (st == 0).all()


def test_hashtables_and_skiplists(engine):
    f = ff.Flat(4)
    rng = f.rng
    for cnt in (0, 1, 63, 64, 65):
        mem = [(_word(rng, int(rng.integers(0, 50))) if k % 5 else INT_RULE[k % len(INT_RULE)]) for k in range(cnt)]
        f.add(rr.T_SET_HT, 0, mem)
        f.add(rr.T_HASH_HT, 0, mem + mem)
        items = []
        for k, m in enumerate(mem):
            items += [m, ("score", struct.unpack("<Q", struct.pack("<d", (-0.0, float("inf"), 1.5, -2e300)[k % 4]))[0])]
        f.add(rr.T_ZSET_SKIPLIST, 0, items)
        f.add(rr.T_SET_INTSET, (2, 4, 8)[cnt % 3], [int(rng.integers(-30000, 30000)) for _ in range(cnt)])
    f.add(rr.T_SET_HT, 0, [_word(rng, 100)] * 20000)           # a count that takes rdbSaveLen's 32-bit form
    f.add(rr.T_HASH_HT, 0, [_word(rng, 40000), _word(rng, 3)])
    st, _ = check(engine, *f.done())
    assert (st == 0).all()
    # a SET_HT whose blob held duplicates: fewer descriptors than slots, the tail zero
    blob = bytes([rr.T_SET_HT]) + struct.pack("<I", 9) + struct.pack("<Q", 3)
    for m in (b"a", b"b", b"a"):
        blob += struct.pack("<Q", len(m)) + m
    values, elems, arena = flat_of([blob])
    assert int(values["n_elems"][0]) == 2
    check(engine, values, elems, arena)


@pytest.mark.parametrize("flags", [0, rr.CTX_ZL_RAW])
def test_ziplists(engine, flags):
    data, offs = rr.gen_batch(3, 300)
    blobs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(300)] + golden_blobs()
    values, elems, arena = flat_of(blobs, flags)
    st, _ = check(engine, values, elems, arena)
    assert (st == 0).sum() >= 300
    f = ff.Flat(5)
    f.add(rr.T_HASH_ZIPLIST, 0, [("zl", b"12")])               # read as a decimal: INT8
    f.add(rr.T_ZSET_ZIPLIST, 0, [("zl", b"-2147483648"), b"ignored", 7])
    f.add(rr.T_HASH_ZIPLIST, 0, [("zl", b"")])
    st, _ = check(engine, *f.done())
    assert (st == 0).all()


@pytest.mark.parametrize("seed", [101, 202])
def test_unsaveable_values(engine, seed):
    v, e, a, classes = ff.forge_mutations(*ff.well_formed(seed, 600), seed)
    st, tot = check(engine, v, e, a, bounded=False)
    assert (st == rr.E_ENCODE).any() and (st == 0).any() and tot["n_bad"] == int((st != 0).sum())
    for cls, (_, can_accept) in ff.MUTATION_CLASSES.items():   # each class that the rule always refuses
        hit = [i for i, c in enumerate(classes) if c == cls]
        if not can_accept:
            assert hit and all(st[i] == rr.E_ENCODE and st[i] != 0 for i in hit), cls


def test_capacity(engine):
    values, elems, arena = list_edge_batch()
    offsets = ref.save_batch(values, elems, arena)[2]
    n = len(values)
    for i in (0, n // 2, n - 1):
        cut = (int(offsets[i]) + int(offsets[i + 1])) // 2     # in the middle of value i
        st, _ = check(engine, values, elems, arena, data_cap=cut)
        assert st[i] == rr.E_CAPACITY and (st[:i] == 0).all() and (st[i:] == rr.E_CAPACITY).all()
    check(engine, values, elems, arena, data_cap=1)
    check(engine, values[:0], elems, arena)


def test_chain_decode_then_save(engine):
    data, offs = rr.gen_batch(4, 3000)
    n, nb = len(offs) - 1, len(data)
    cap = rr.elem_bound(n, int(offs[-1]))
    d_data, d_offs = _dev(data), torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_vals = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_elems = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
    d_arena = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(8, dtype=torch.int64, device="cuda")
    values, elems, arena, _ = rr.host_decode(data, offs)
    room = rr.rdbsave_bound(values, elems)
    out = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    o_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    o_ty = torch.zeros(n, dtype=torch.uint8, device="cuda")
    o_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    engine.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot[:4])
    engine.rdbsave_device(d_vals, d_elems, d_arena, out, o_off, o_ty, o_st, d_tot[4:])
    torch.cuda.synchronize()
    ty, hdata, hoff, hst, htot = engine.rdbsave_host(values, elems, arena)
    assert np.array_equal(o_off.cpu().numpy().view(np.uint64), hoff)
    assert np.array_equal(out.cpu().numpy()[:int(hoff[-1])], hdata)
    assert np.array_equal(o_ty.cpu().numpy(), ty) and np.array_equal(o_st.cpu().numpy(), hst)
    exp = ref.save_batch(values, elems, arena)
    assert np.array_equal(hdata, exp[1]) and htot == exp[4]


def test_fuzz(engine):
    v, e, a, _ = ff.forge_mutations(*ff.well_formed(777, 2000, scale=2), 778, share=0.4)
    check(engine, v, e, a, fill=int(np.random.default_rng(779).integers(-5, 4)), bounded=False)
