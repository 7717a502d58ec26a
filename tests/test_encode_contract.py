"""The encode contract on flat batches no decoder produced (tests/flat_forge.py): the rule stated
in plain Python (tests/encode_expect.py), the C oracle (rro_encode) and the host codec
(rr_host_encode_batch) held to each other three ways — offsets, totals and the bytes in
[0, min(data_cap, offsets[n])).  data_cap is passed explicitly everywhere: encode_bound sums raw
len fields, and a forged len of 2^32 - 1 would make it allocate gigabytes.  The GPU routes are
held to the same Python statement in tests/test_gpu_encode_contract.py."""
import struct

import numpy as np
import pytest

import redrock_old_amd as rr
from oracle import cpu

import flat_forge as ff
from encode_expect import accepted_mask, expect_encode

MUTATION_SEEDS = (101, 202, 303, 404)


def three_ways(v, e, a, cap, what=""):
    """expect_encode == cpu.encode == rr.host_encode on one batch at one data_cap."""
    xb, xo, xt = expect_encode(v, e, a, cap)
    for name, fn in (("oracle", cpu.encode), ("host codec", rr.host_encode)):
        ob, oo, ot = fn(v, e, a, data_cap=cap)
        assert np.array_equal(oo, xo), f"{what} cap {cap}: {name} offsets differ"
        assert ot == xt, f"{what} cap {cap}: {name} totals {ot} != {xt}"
        k = min(cap, int(xo[-1]))
        assert len(ob) >= k and np.array_equal(ob[:k], xb[:k]), f"{what} cap {cap}: {name} bytes differ"
    return xb, xo, xt


def all_caps(v, e, a, what=""):
    acc = accepted_mask(v, e, a)
    _, xo, xt = expect_encode(v, e, a, 1 << 62)
    caps = ff.cap_settings(xo, acc, xt["bytes"])
    for cap in caps:
        three_ways(v, e, a, cap, what)
    return acc, caps


def test_well_formed_values_of_every_type_encode_and_decode_back():
    """Every forged well-formed value encodes (the empty List to 5 bytes, empty sets / hashes /
    skiplists / intsets to 13, empty strings to 6), and cpu.decode of the blobs gives the records
    and descriptors back, arena offsets aside.  Of a ziplist value only descriptor 0 is written,
    so only that one is compared, and a ZLRAW too short to be a ziplist (under 11 bytes) does not
    decode at all: those are checked on their blob bytes alone."""
    v, e, a = ff.well_formed(11, 400)
    acc, _ = all_caps(v, e, a, "well-formed")
    assert all(acc)
    out, offs, t = expect_encode(v, e, a, 1 << 62)
    assert t["n_bad"] == 0
    sizes = np.diff(offs.astype(np.int64))
    empty = v["n_elems"] == 0
    assert (sizes[empty & (v["type"] == rr.T_LIST_QUICKLIST)] == 5).all() and (empty & (v["type"] == rr.T_LIST_QUICKLIST)).any()
    for t_ in (rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST, rr.T_SET_INTSET):
        assert (empty & (v["type"] == t_)).any() and (sizes[empty & (v["type"] == t_)] == 13).all()
    data = np.concatenate([out, np.zeros(16, np.uint8)])
    dv, de, da, dt = cpu.decode(data, offs)
    zl_back = 0
    for i in range(len(v)):
        b, c = int(v["elem_base"][i]), int(v["n_elems"][i])
        zl = v["type"][i] in ff.ZL_TYPES
        if zl:
            ln = int(e["len"][b])
            assert sizes[i] == 13 + ln
            o = int(offs[i])
            assert bytes(out[o + 5:o + 13]) == struct.pack("<Q", ln)
            assert bytes(out[o + 13:o + 13 + ln]) == bytes(a[int(e["data"][b]):int(e["data"][b]) + ln])
            if dv["status"][i] != 0:
                continue
            c = 1
        assert dv["status"][i] == 0, i
        for f in ("type", "enc", "lru"):
            assert dv[f][i] == v[f][i], (i, f)
        db = int(dv["elem_base"][i])
        if not zl:
            assert dv["n_elems"][i] == c, i
        for k in range(c):
            x, y = e[b + k], de[db + k]
            assert (x["kind"], x["len"]) == (y["kind"], y["len"]), (i, k)
            if x["kind"] in (rr.K_STR, rr.K_ZLRAW):
                assert bytes(a[int(x["data"]):int(x["data"]) + int(x["len"])]) == \
                    bytes(da[int(y["data"]):int(y["data"]) + int(y["len"])]), (i, k)
            else:
                assert x["data"] == y["data"], (i, k)
        zl_back += zl
    assert zl_back >= len(v) // 20        # (the well-formed ziplists: 2 shapes of 20)


@pytest.mark.parametrize("seed", MUTATION_SEEDS)
def test_mutants_three_ways(seed):
    v, e, a = ff.well_formed(seed, 1500)
    mv, me, ma, classes = ff.forge_mutations(v, e, a, seed)
    all_caps(mv, me, ma, f"mutants {seed}")


@pytest.mark.parametrize("seed", MUTATION_SEEDS)
def test_mutants_balance(seed):
    """On the Python statement alone: at least 30 % of a mutation batch encodes and at least 20 %
    does not; every mutation class rejects at least one value where the rule can reject such a
    mutant (lru's top byte and zenc / rsv are not looked at: never) and leaves one accepted where
    it can accept one (an unknown type, a nonzero status, an odd pair count, a swapped pair and a
    STRING of 0 or 2 descriptors: never)."""
    v, e, a = ff.well_formed(seed, 1500)
    mv, me, ma, classes = ff.forge_mutations(v, e, a, seed)
    acc = np.array(accepted_mask(mv, me, ma))
    assert acc.mean() >= 0.30 and (~acc).mean() >= 0.20, acc.mean()
    assert acc[[c is None for c in classes]].all()          # the untouched ones still encode
    for name, (can_reject, can_accept) in ff.MUTATION_CLASSES.items():
        mine = np.array([c == name for c in classes])
        assert mine.sum() >= 5, name
        assert (~acc[mine]).any() == can_reject, name
        assert acc[mine].any() == can_accept, name
    # the exact-capacity mutants: a range ending at elem_cap and a payload ending at arena_cap
    ends = mv["elem_base"].astype(np.int64) + mv["n_elems"].astype(np.int64)
    at_ecap = (ends == len(me)) & (mv["n_elems"] > 0) & (mv["n_elems"] < 0xFFFFFFFF)
    assert acc[at_ecap].any() and (~acc[ends == len(me) + 1]).all() and (ends == len(me) + 1).any()
    pend = me["data"].astype(object) + me["len"].astype(object)
    assert (pend == len(ma)).any() and (pend == len(ma) + 1).any() and (pend == 1 << 64).any()


def _placements():
    yield "block edge run", ff.block_edge_run()[0]
    for d in (-1, 0, 1):
        yield f"window edge {d:+d}", ff.window_edge_run(d)[0]
    for w in ("first", "last", "all"):
        yield f"{w} rejected", ff.edges_rejected(w)
    yield "big task block", ff.big_task_block()[0]


@pytest.mark.parametrize("name,batch", list(_placements()), ids=lambda x: x if isinstance(x, str) else "")
def test_placements_three_ways(name, batch):
    v, e, a = batch
    acc, caps = all_caps(v, e, a, name)
    if name == "all rejected":
        xb, xo, xt = expect_encode(v, e, a, 64)
        assert not any(acc) and xt["bytes"] == 0 and xt["n_bad"] == len(v) and not xo.any()
    else:
        assert any(acc) and not all(acc)


def test_placements_are_where_they_claim():
    """The helpers' geometry, on the Python statement: the runs are rejected and cross a 256-value
    block edge, the value after the window run starts at 16 KiB - 1 / + 0 / + 1, the big block
    holds more than 4,096 descriptors in its first 256 values with the defects past task 4,096."""
    (v, e, a), (r0, r1) = ff.block_edge_run()
    acc = accepted_mask(v, e, a)
    assert r1 - r0 >= 300 and not any(acc[r0:r1]) and acc[r0 - 1] and acc[r1]
    assert r0 < ff.E1_BLOCK < r1 and r0 < 2 * ff.E1_BLOCK < r1
    for d in (-1, 0, 1):
        (v, e, a), (r0, r1), at = ff.window_edge_run(d)
        acc = accepted_mask(v, e, a)
        _, offs, _ = expect_encode(v, e, a, 1 << 62)
        assert r1 - r0 >= 300 and not any(acc[r0:r1]) and acc[r0 - 1] and acc[r1]
        assert r0 < ff.E1_BLOCK < r1
        assert int(offs[r0]) == int(offs[r1]) == at == ff.ENC_WINDOW + d
        assert int(offs[r1 + 1]) > at and int(offs[-1]) > 2 * ff.ENC_WINDOW
    (v, e, a), bad = ff.big_task_block()
    acc = accepted_mask(v, e, a)
    first = v["n_elems"][:ff.E1_BLOCK].astype(np.int64)
    assert first[first > 4].sum() > ff.ENC_MAPCAP
    assert [i for i in range(len(v)) if not acc[i]] == bad
    tasks_before = np.concatenate([[0], np.cumsum(np.where(first > 4, first, 0))])
    assert all(i < ff.E1_BLOCK and tasks_before[i] > ff.ENC_MAPCAP for i in bad)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "sparse"])
def test_decimal_lengths(dense):
    """List integers at every digit-count and bit-count edge: the encoded element is str(x) with a
    u32 length prefix, three ways."""
    (v, e, a), lists = ff.decimal_lists(dense)
    assert len(ff.decimal_integers()) == 18 * 6 + 62 * 4 + 2
    want = b""
    for i, items in enumerate(lists):
        want += bytes([rr.T_LIST_QUICKLIST]) + struct.pack("<I", int(v["lru"][i]))
        for x in items:
            s = str(x).encode() if isinstance(x, int) else x
            want += struct.pack("<I", len(s)) + s
    xb, xo, xt = three_ways(v, e, a, len(want) + 16, "decimals")
    assert xt["n_bad"] == 0 and xt["bytes"] == len(want)
    assert bytes(xb) == want
