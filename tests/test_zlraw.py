"""Raw-ziplist decode mode (RR_CTX_ZL_RAW) on the CPU: the host codec's _ex entry points against
the expected output derived from the strict oracle (tests/zlraw_expect.py), the encode round
trip, and the compat shim's ziplist-check switch (tests/c/test_compat_zlraw.c).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import redrock_old_amd as rr
from helpers import assert_flat_equal, batch_from_blobs, golden, structured_mutations
from oracle import cpu
from test_compat import build
from zlraw_expect import (assert_anti_vacuity, corrupt_in_place, expect_raw, good_ziplist, split_blobs,
                          with_len_defects, zl_blob)

G = golden()
FIXTURES = G["kats"] + G["edges"] + G["shapes"]
RAW = rr.CTX_ZL_RAW


def _check_batch(data, offs, what, elem_cap=None, vacuity=True):
    """host_decode_ex(RAW) == the helper's expectation; flags 0 == the plain call; the raw decode
    re-encodes to the input bytes for every accepted value."""
    want_v, want_e, want_t, info = expect_raw(data, offs, elem_cap)
    if vacuity:
        assert_anti_vacuity(info)
    cap = elem_cap if elem_cap is not None else rr.elem_bound(len(offs) - 1, int(offs[-1]))
    v, e, a, t = rr.host_decode_ex(data, offs, RAW, cap)
    assert_flat_equal((v, e), (want_v, want_e), what)
    assert t == want_t, (what, t, want_t)
    assert np.array_equal(a, data[:int(offs[-1])]), what
    # flags 0: the existing function, field for field
    v0, e0, a0, t0 = rr.host_decode_ex(data, offs, 0, cap)
    p = rr.host_decode(data, offs, cap)
    assert_flat_equal((v0, e0), (p[0], p[1]), what + " flags 0")
    assert t0 == p[3] and np.array_equal(a0, p[2])
    # encode(decode_raw(b)) == b for every accepted value (one descriptor, arbitrary bytes)
    if elem_cap is None:
        d, o, t2 = rr.host_encode(v, e, a)
        od, oo, ot2 = cpu.encode(v, e, a)
        assert np.array_equal(o, oo) and np.array_equal(d, od[:len(d)]) and t2 == ot2, what
        ok = np.nonzero(v["status"] == 0)[0]
        for i in ok[info["accepted"][ok]]:
            b = bytes(data[int(offs[i]):int(offs[i + 1])])
            b = b[:1] + (int.from_bytes(b[1:5], "little") & 0xFFFFFF).to_bytes(4, "little") + b[5:]
            assert bytes(d[int(o[i]):int(o[i + 1])]) == b, (what, int(i))
    return v, e, a, t, info


def test_helper_against_literals():
    """The expectation helper itself, on three hand-written values (batch offsets 0, 32 and 64)."""
    zl = good_ziplist([b"f1", b"v1"])
    assert zl.hex() == "13000000" "0e000000" "0200" "00026631" "04027631" "ff"
    good = zl_blob(13, zl, lru=0xAB123456)
    flipped = bytearray(good)
    flipped[13 + 14] = 0x09            # the second entry's prevlen (4 -> 9): entries no longer chain
    empty = zl_blob(12, b"", lru=7)    # Lz = 0: no ziplist at all
    data, offs = batch_from_blobs([good, bytes(flipped), empty])
    v, e, t, info = expect_raw(data, offs)
    sv = info["strict"][0]
    assert [int(x) for x in sv["status"]] == [0, 10, 10] and [int(x) for x in sv["n_elems"]] == [3, 0, 0]
    lit_v = np.array([(13, 0, 0, 0x123456, 1, 0), (13, 0, 0, 0x123456, 1, 1), (12, 0, 0, 7, 1, 2)], rr.VALUE_DT)
    lit_e = np.array([(13, 19, rr.K_ZLRAW, 0, 0), (32 + 13, 19, rr.K_ZLRAW, 0, 0), (64 + 13, 0, rr.K_ZLRAW, 0, 0)],
                     rr.ELEM_DT)
    assert_flat_equal((v, e), (lit_v, lit_e), "literals")
    assert t == {"n_elems": 3, "bytes": 77, "n_bad": 0, "payload": 38}
    assert info["corrupt_accepted"] == 2 and info["len_rejected"] == 0
    # and with a capacity of two slots the last value is cut
    v2, e2, t2, _ = expect_raw(data, offs, elem_cap=2)
    assert [int(x) for x in v2["status"]] == [0, 0, 11] and len(e2) == 2 and t2["n_bad"] == 1 and t2["payload"] == 38


def test_golden_batch():
    blobs = [bytes.fromhex(f["blob"]) for f in FIXTURES]
    data, offs = batch_from_blobs(blobs)
    v, e, a, t, info = _check_batch(data, offs, "golden")
    by_name = {f["name"]: i for i, f in enumerate(FIXTURES)}
    for name in ("bad_ziplist_encoding", "bad_ziplist_odd_entries", "bad_ziplist_zllen"):
        assert int(v[by_name[name]]["status"]) == 0 and int(v[by_name[name]]["n_elems"]) == 1, name
    assert int(v[by_name["bad_ziplist_len"]]["status"]) == 9


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_each_fixture_one_value(fx):
    """rr_host_decode_value_ex: the batch expectation of the one-value batch, base 0."""
    blob = bytes.fromhex(fx["blob"])
    data, offs = batch_from_blobs([blob])
    want_v, want_e, _, info = expect_raw(data, offs)
    st, v, e, need = rr.host_decode_value_ex(blob, RAW, cap=1 << 16)
    assert st == int(want_v[0]["status"])
    for k in ("type", "enc", "status", "lru", "n_elems"):
        assert int(v[k]) == int(want_v[0][k]), (fx["name"], k)
    if st == 0:
        assert np.array_equal(e, want_e[:int(v["n_elems"])]) and need == len(want_e)
    if info["accepted"][0]:
        assert st == 0 and need == 1
        st1, _, _, need1 = rr.host_decode_value_ex(blob, RAW, cap=0)
        assert st1 == 11 and need1 == 1
    st0, v0, e0, need0 = rr.host_decode_value_ex(blob, 0, cap=1 << 16)
    p = rr.host_decode_value(blob, cap=1 << 16)
    assert st0 == p[0] and v0 == p[1] and np.array_equal(e0, p[2]) and need0 == p[3]


@pytest.mark.parametrize("cfg,n", [(3, 2000), (4, 4000), (10, 3000), (11, 60)])
def test_configs(cfg, n):
    rng = np.random.default_rng(100 + cfg)
    data, offs = rr.gen_batch(cfg, n)
    blobs = with_len_defects(corrupt_in_place(split_blobs(data, offs), rng, 0.3), rng)
    data, offs = batch_from_blobs(blobs)
    _check_batch(data, offs, f"cfg {cfg}")


@pytest.mark.parametrize("cfg,n,seed", [(4, 2000, 1), (3, 800, 2), (10, 600, 3), (11, 30, 4), (4, 2000, 11)])
def test_structured_fuzz(cfg, n, seed):
    """The shared structured fuzz corpus (tests/helpers.py): its ziplist mutants are bit flips,
    truncations, header words and inserted bytes — both CORRUPT-but-accepted and ZL_LEN kinds."""
    data, offs = rr.gen_batch(cfg, n)
    fdata, foffs = batch_from_blobs(structured_mutations(data, offs, 1000 + cfg + 7919 * seed))
    _check_batch(fdata, foffs, f"fuzz cfg {cfg} seed {seed}")


def test_hand_built_edges():
    rng = np.random.default_rng(77)
    zl = good_ziplist([b"a", b"1", b"bb", b"22"])
    blobs = []
    for tag in (12, 13):
        hdr = bytes([tag]) + b"\x01\x02\x03\xff"
        blobs += [hdr + b"\0" * 7, hdr + b"\0" * 8]                                # L = 12 (SHORT), 13 (Lz = 0)
        for lz in (1, 10, 11):
            blobs.append(zl_blob(tag, bytes(rng.integers(0, 256, lz, dtype=np.uint8))))
        blobs += [zl_blob(tag, zl, lz=len(zl) + 1), zl_blob(tag, zl, lz=len(zl) - 1), zl_blob(tag, zl)]   # Lz = L - 13 +- 1
        sat = bytearray(zl)
        sat[8:10] = b"\xff\xff"                                                    # zllen = 0xFFFF: the counted form
        blobs.append(zl_blob(tag, bytes(sat)))
        for size in (11, 64, 4096):
            blobs.append(zl_blob(tag, bytes(rng.integers(0, 256, size, dtype=np.uint8))))
        blobs.append(zl_blob(tag, zl[:-1] + b"\x00"))                             # no 0xFF end byte
        blobs.append(zl_blob(tag, good_ziplist([b"a", b"1", b"odd"])))            # odd pair count
        blobs.append(zl_blob(tag, zl, lz=len(zl) + (1 << 32)))                     # a count past 32 bits: ZL_LEN
    blobs += [b"\x00\x00\x00\x00\x00\x00abc", bytes([14]) + b"\0" * 4 + (3).to_bytes(4, "little") + b"xyz"]
    data, offs = batch_from_blobs(blobs)
    v, e, a, t, info = _check_batch(data, offs, "edges")
    st = [int(x) for x in v["status"]]
    assert st[0] == 1 and st[1] == 0 and st[5] == 9 and st[6] == 9 and st[7] == 0
    # every capacity from none to all of it
    for cap in (0, 1, 5, len(e) - 1, len(e)):
        _check_batch(data, offs, f"edges cap {cap}", elem_cap=cap, vacuity=False)


def test_unknown_flag_bits_refused():
    data, offs = batch_from_blobs([b"\x00\x00\x00\x00\x00\x00abc"])
    with pytest.raises(rr.RRError):
        rr.host_decode_ex(data, offs, 4)
    rr.host_decode_ex(data, offs, rr.CTX_NO_SMALL | RAW)   # (a context's flags pass as they are)


def _run(exe, mode, env_val):
    env = {k: v for k, v in os.environ.items() if k != "RR_COMPAT_ZL_CHECK"}
    if env_val is not None:
        env["RR_COMPAT_ZL_CHECK"] = env_val
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
    return r.stdout


def test_compat_shim_ziplist_check(tmp_path):
    """tests/c/test_compat_zlraw.c over the Redis model, host route: the check off (by the call
    and by the environment) accepts the corrupt-ziplist fixtures as the reference does — the
    object's ziplist is the blob's bytes, serObject writes the blob back — a wrong-length fixture
    still panics, the batch form matches the per-key results; the default is today's strict walk."""
    exe = build(str(tmp_path), "test_compat_zlraw")
    assert "strict" in _run(exe, "default", None)
    assert "strict" in _run(exe, "default", "1")
    assert "reference acceptance" in _run(exe, "env-off", "0")
    assert "reference acceptance" in _run(exe, "call-off", None)
    # rr_compat_rdb_load_batch: the check applied is the restoring process's, in both parent modes
    assert "rdb restore" in _run(exe, "rdb", None)
