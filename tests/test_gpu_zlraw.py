"""Raw-ziplist decode mode (RR_CTX_ZL_RAW) on the GPU: every decode route of a context with the
flag set — the one-launch small kernel (wave and lane routes), the pipeline's one-launch and
two-launch forms, the chunked host path — against the expectation derived from the strict oracle
(tests/zlraw_expect.py): records, descriptors, the arena mirror, totals, and
encode(decode_raw(b)) == b for every accepted value.  Every batch holds a value strict mode
rejects as RR_E_ZL_CORRUPT that raw mode accepts and an RR_E_ZL_LEN that stays rejected."""
import numpy as np
import pytest
import torch

import redrock_old_amd as rr
from helpers import assert_flat_equal, batch_from_blobs, golden
from oracle import cpu
from zlraw_expect import (assert_anti_vacuity, corrupt_in_place, expect_raw, good_ziplist, split_blobs,
                          with_len_defects, zl_blob)

pytestmark = pytest.mark.gpu
G = golden()
FIXTURES = G["kats"] + G["edges"] + G["shapes"]
RAW = rr.CTX_ZL_RAW


@pytest.fixture(scope="module")
def raw_pipe():
    """the batch pipeline for every batch size, ziplists kept raw"""
    eng = rr.Engine(0)
    eng.set_options(rr.CTX_NO_SMALL | RAW)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def raw_small():
    """the default routing (small batches take the one-launch kernel), ziplists kept raw"""
    eng = rr.Engine(0)
    eng.set_options(RAW)
    yield eng
    eng.close()


def _accepted_round_trip(eng, v, e, a, data, offs, info, what, stride=1):
    """encode(decode_raw(b)) == b: the whole batch's valid values re-encoded, the accepted ones'
    bytes compared with the input (lru masked to the 24 bits serObject writes)."""
    ok = np.nonzero(v["status"] == 0)[0]
    out, oo, t2 = eng.encode_host(v[ok], e, a)
    assert t2["n_bad"] == 0, what
    acc = info["accepted"][ok]
    for k in np.nonzero(acc)[0][::stride]:
        i = int(ok[k])
        b = bytes(data[int(offs[i]):int(offs[i + 1])])
        b = b[:1] + (int.from_bytes(b[1:5], "little") & 0xFFFFFF).to_bytes(4, "little") + b[5:]
        assert bytes(out[int(oo[k]):int(oo[k + 1])]) == b, (what, i)


def _check(eng, data, offs, what, elem_cap=None, vacuity=True, stride=1):
    want_v, want_e, want_t, info = expect_raw(data, offs, elem_cap)
    if vacuity:
        assert_anti_vacuity(info)
    v, e, a, t = eng.decode_host(data, offs, elem_cap)
    assert_flat_equal((v, e), (want_v, want_e), what)
    assert t == want_t, (what, t, want_t)
    assert np.array_equal(a, data[:int(offs[-1])]), what   # the arena mirrors the blobs: every descriptor's bytes
    if elem_cap is None:
        _accepted_round_trip(eng, v, e, a, data, offs, info, what, stride)
    return v, e, a, t, info


def _device_decode(eng, data, offs, elem_cap):
    """one rr_decode_batch call on device buffers (no chunking): (values, elems, arena, totals)"""
    n, nbytes = len(offs) - 1, int(offs[-1])
    d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    o = torch.from_numpy(offs.astype(np.int64)).cuda()
    vals = torch.zeros(max(n, 1) * 16, dtype=torch.uint8, device="cuda")
    els = torch.zeros(max(elem_cap, 1) * 16, dtype=torch.uint8, device="cuda")
    arena = torch.zeros(d.numel() + 16, dtype=torch.uint8, device="cuda")
    tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    eng.decode_device(d, o, vals, els, arena, tot)
    torch.cuda.synchronize()
    t = [int(x) for x in tot.cpu().numpy().view(np.uint64)]
    totals = {"n_elems": t[0], "bytes": t[1], "n_bad": t[2], "payload": t[3]}
    v = vals.cpu().numpy().view(rr.VALUE_DT)[:n]
    e = els.cpu().numpy().view(rr.ELEM_DT)[:min(t[0], elem_cap)]
    return v, e, arena.cpu().numpy()[:nbytes], totals


DEC_W, ONE_MAX_WINDOWS = 73728, 512   # rr_kernels.hip: RR_DEC_W; the one-launch form's window limit (DEC_NW * 64)


def _golden_blobs():
    return [bytes.fromhex(f["blob"]) for f in FIXTURES]


def _zl_only(n, rng, frac=1 / 3, tiny=False):
    """n ziplist values (hash and zset tags alternating), a third corrupted in place (length kept).
    tiny: one pair of 1-2 byte entries, a blob of at most 32 bytes (the small kernel's lane route)"""
    blobs = []
    for i in range(n):
        k = 2 if tiny else 2 * int(rng.integers(1, 9))
        ent = [bytes(rng.integers(97, 123, int(rng.integers(1, 3 if tiny else 12)), dtype=np.uint8)) for _ in range(k)]
        blobs.append(zl_blob(13 if i & 1 else 12, good_ziplist(ent), lru=i))
    return corrupt_in_place(blobs, rng, frac)


def _wrong_count(b, d):
    return b[:5] + (int.from_bytes(b[5:13], "little") + d).to_bytes(8, "little") + b[13:]


# ---- 1. the option itself ---------------------------------------------------------------------
def test_set_options_accepts_zl_raw():
    eng = rr.Engine(0)
    try:
        eng.set_options(RAW)
        eng.set_options(rr.CTX_NO_SMALL | RAW)
        with pytest.raises(rr.RRError):
            eng.set_options(4)
        with pytest.raises(rr.RRError):
            eng.set_options(RAW | 4)
        eng.set_options(0)
    finally:
        eng.close()


# ---- 2. the golden batch on every route ---------------------------------------------------------
def test_golden_small_kernel(raw_small):
    """(the fixtures of under 4000 bytes: at most 256 values in at most 128 KiB take the one-launch
    kernel's wave-per-value route)"""
    data, offs = batch_from_blobs([b for b in _golden_blobs() if len(b) < 4000])
    assert len(offs) - 1 <= 256 and len(data) <= 128 * 1024
    _check(raw_small, data, offs, "golden, small kernel")


def test_golden_pipeline(raw_pipe):
    _check(raw_pipe, *batch_from_blobs(_golden_blobs()), "golden, pipeline")


def test_golden_one_fixture_per_call(raw_small, raw_pipe):
    for f in FIXTURES:
        blob = bytes.fromhex(f["blob"])
        data, offs = batch_from_blobs([blob])
        if data.size == 0:   # (the empty blob: the entry point wants a buffer all the same)
            data = np.zeros(16, np.uint8)
        _check(raw_small, data, offs, f["name"], vacuity=False)
        if blob and blob[0] in (12, 13):
            _check(raw_pipe, data, offs, f["name"] + " (pipeline)", vacuity=False)


# ---- 3. the small kernel's routes: one wave per value up to 256 values, one lane per value past it
@pytest.mark.parametrize("n", [1, 256, 257, 4096])
def test_small_kernel_route_boundaries(raw_small, n):
    """All-ziplist batches of at most 32-byte values (4096 of them fit 128 KiB).  n = 1 cannot hold
    both kinds the other batches must hold: its one value is a corrupt ziplist raw mode accepts."""
    rng = np.random.default_rng(300 + n)
    blobs = _zl_only(n, rng, tiny=True)
    assert max(len(b) for b in blobs) <= 32
    if n == 1:
        m = bytearray(blobs[0])
        m[13 + 11] = 0x7F   # the first entry's encoding byte: a 63-byte string in a 19-byte ziplist
        data, offs = batch_from_blobs([bytes(m)])
        _, _, _, info = expect_raw(data, offs)
        assert info["corrupt_accepted"] == 1
        _check(raw_small, data, offs, "small n=1", vacuity=False)
        return
    blobs[-3:] = [_wrong_count(b, 1) for b in blobs[-3:]]
    data, offs = batch_from_blobs(blobs)
    assert len(blobs) == n and len(data) <= 128 * 1024
    _check(raw_small, data, offs, f"small n={n}")


# ---- 4. the pipeline: dense windows of ziplists at the lane and sort-chunk edges ------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 512, 513])
def test_pipeline_dense_windows(raw_pipe, n):
    """A first window of exactly n ziplist values: n - 1 values of at most 32 bytes, then a run of
    ziplists with random 64 KiB bodies, the first of which starts in that window.  A batch of at
    most one 72 KiB window per CU gets one window per CU (rr_launch_decode): its window size is its
    bytes over the device's CU count, rounded up to 16.  The run of long values is sized from the
    CU count so that a window is at least 16.5 KiB (513 tiny values and the long one's first byte),
    and the first window's population is counted from the offsets and asserted.  The long values
    fill the other windows, one value or none each.  A third of the tiny bodies are corrupted in
    place; the wrong byte counts come last, in a window of their own.  These are the 64-lane batch
    and the 512-value sort-chunk edges; the first window also ends in a long raw ziplist, of which
    the stage takes the header only."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(400 + n)
    tiny = _zl_only(n - 1, rng, tiny=True)
    long_ = zl_blob(13, bytes(rng.integers(0, 256, 64 * 1024, dtype=np.uint8)))
    fill = -(-cus * 16896 // len(long_)) + 1
    blobs = tiny + [long_] * fill + [_wrong_count(tiny[0] if tiny else long_[:40], -1), _wrong_count(long_, 1)]
    data, offs = batch_from_blobs(blobs)
    assert len(data) <= cus * DEC_W and len(blobs) <= cus * 512   # (the one-window-per-CU sizing applies)
    win = (-(-len(data) // cus) + 15) & ~15
    assert int((offs[:-1] < win).sum()) == n, (cus, win)
    _check(raw_pipe, data, offs, f"dense n={n}", stride=5)


# ---- 5. mixed classes ------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [4, 11])
def test_mixed_classes(raw_pipe, cfg):
    rng = np.random.default_rng(500 + cfg)
    data, offs = rr.gen_batch(cfg, 5000)
    blobs = with_len_defects(corrupt_in_place(split_blobs(data, offs), rng, 0.3), rng)
    data, offs = batch_from_blobs(blobs)
    _check(raw_pipe, data, offs, f"mixed cfg {cfg}", stride=7)


# ---- 6. long raw ziplists ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_long_raw_ziplists(raw_pipe, where):
    """Random 70 KiB (crosses a window boundary and the stage tail) and 200 KiB (longer than a
    window) bodies among small values: only their headers are read."""
    rng = np.random.default_rng(600)
    small = _zl_only(600, rng) + [b"\x00\x00\x00\x00\x00\x00" + bytes(rng.integers(0, 256, 40, dtype=np.uint8))] * 50
    small = with_len_defects(small, rng)
    long_ = [zl_blob(13, bytes(rng.integers(0, 256, 70 * 1024, dtype=np.uint8))),
             zl_blob(12, bytes(rng.integers(0, 256, 200 * 1024, dtype=np.uint8)))]
    blobs = long_ + small if where == "first" else small + long_ if where == "last" else \
        small[:300] + long_[:1] + small[300:500] + long_[1:] + small[500:]
    data, offs = batch_from_blobs(blobs)
    _check(raw_pipe, data, offs, f"long {where}")


# ---- 7. the one-launch form's help path ---------------------------------------------------------------
def test_one_launch_help_path(raw_pipe):
    rng = np.random.default_rng(700)
    data, offs = rr.gen_batch(3, 4000)
    blobs = with_len_defects(corrupt_in_place(split_blobs(data, offs), rng, 0.3), rng)
    data, offs = batch_from_blobs(blobs)
    raw_pipe.debug_one_help()
    _check(raw_pipe, data, offs, "help path", stride=11)
    _check(raw_pipe, data, offs, "the next call", stride=11)


# ---- 8. the two-launch form -------------------------------------------------------------------------
def test_two_launch_form(raw_pipe):
    """The one-launch form takes a batch of at most 512 windows of at most 72 KiB (rr_launch_decode:
    nw <= DEC_NW * RR_WAVE), so config 3 at the smallest n whose bytes pass 512 * 73728 =
    37,748,736 is the first to run count_kernel + decode_kernel: n = 60,252 values of 346 to 1,036
    bytes (computed from the generated offsets and asserted below).  Records sampled at a stride, totals exact."""
    data, offs = rr.gen_batch(3, 61000)
    n = int(np.searchsorted(offs, ONE_MAX_WINDOWS * DEC_W, side="right"))   # the first n with offs[n] past it
    assert n == 60252 and int(offs[n - 1]) <= ONE_MAX_WINDOWS * DEC_W < int(offs[n])
    rng = np.random.default_rng(800)
    # ... and, behind them, windows that end in a long raw ziplist (the stage takes its header only)
    tail = [zl_blob(13, bytes(rng.integers(0, 256, 70 * 1024, dtype=np.uint8))), bytes(data[:int(offs[1])]),
            zl_blob(12, bytes(rng.integers(0, 256, 200 * 1024, dtype=np.uint8))), bytes(data[:int(offs[1])])]
    td, to = batch_from_blobs(tail)
    nb = int(offs[n])
    offs = np.concatenate([offs[:n + 1], to[1:] + np.uint64(nb)])
    data = np.concatenate([data[:nb], td, np.zeros(-(nb + len(td)) % 16, np.uint8)])
    n = len(offs) - 1
    m = data.copy()
    at = rng.choice(n - 12, n // 3, replace=False)
    pos = offs[at].astype(np.int64) + 13 + rng.integers(0, 200, len(at))   # a body byte of a third of the values
    m[pos] ^= 0x10
    for i in (n - 7, n - 6, n - 5):   # wrong byte counts (config-3 values before the long ones)
        m[int(offs[i]) + 5] ^= 1
    want_v, want_e, want_t, info = expect_raw(m, offs)
    assert_anti_vacuity(info)
    cap = int(want_t["n_elems"])
    v, e, a, t = _device_decode(raw_pipe, m, offs, cap)
    assert t == want_t
    assert np.array_equal(v["elem_base"], want_v["elem_base"]) and np.array_equal(v["status"], want_v["status"])
    assert np.array_equal(v[::37], want_v[::37]) and np.array_equal(e[::37], want_e[::37])
    assert np.array_equal(v[-200:], want_v[-200:]) and np.array_equal(e[-3000:], want_e[-3000:])   # (around the long values)
    assert np.array_equal(a[::4099], m[:int(offs[-1])][::4099])


# ---- 9. capacity --------------------------------------------------------------------------------------
def test_capacity_exact_and_one_less(raw_pipe, raw_small):
    rng = np.random.default_rng(900)
    blobs = with_len_defects(_zl_only(700, rng, tiny=True), rng) + _zl_only(5, rng, frac=0.0, tiny=True)
    data, offs = batch_from_blobs(blobs)
    _, _, tot, _ = expect_raw(data, offs)
    need = tot["n_elems"]
    for eng in (raw_pipe, raw_small):
        v, e, a, t, _ = _check(eng, data, offs, "cap exact", elem_cap=need)
        assert (v["status"] != 11).all()
        v, e, a, t, _ = _check(eng, data, offs, "cap - 1", elem_cap=need - 1)
        assert [int(i) for i in np.nonzero(v["status"] == 11)[0]] == [len(blobs) - 1]


# ---- 10. mode isolation on one context ------------------------------------------------------------------
def test_mode_isolation():
    rng = np.random.default_rng(1000)
    data, offs = rr.gen_batch(4, 3000)
    blobs = with_len_defects(corrupt_in_place(split_blobs(data, offs), rng, 0.3), rng)
    data, offs = batch_from_blobs(blobs)
    eng = rr.Engine(0)
    try:
        for base in (rr.CTX_NO_SMALL, 0):
            eng.set_options(base | RAW)
            r1 = _check(eng, data, offs, "raw 1", stride=13)
            eng.set_options(base)
            v, e, a, t = eng.decode_host(data, offs)
            ov, oe, oa, ot = cpu.decode(data, offs)
            assert_flat_equal((v, e), (ov, oe), "strict between two raw calls")
            assert t == ot and np.array_equal(a, oa)
            eng.set_options(base | RAW)
            r2 = eng.decode_host(data, offs)
            assert_flat_equal((r2[0], r2[1]), (r1[0], r1[1]), "raw 2 == raw 1")
            assert r2[3] == r1[3] and np.array_equal(r2[2], r1[2])
            # (second round: small enough for the one-launch kernel; the wrong byte counts are the last three)
            data, offs = batch_from_blobs(blobs[:900] + blobs[-3:])
    finally:
        eng.close()


# ---- 11. the chunked host path ---------------------------------------------------------------------------
def test_chunked_host_decode(raw_pipe):
    """rr_decode_batch_host cuts a batch of more than 16 MiB into chunks: config 3 just past it
    (27,000 values, 16.1 MiB), equal to one rr_decode_batch call on device buffers; and the
    re-decode on overflow (elem_cap one short of the total)."""
    n = 27000
    data, offs = rr.gen_batch(3, n)
    assert (16 << 20) < int(offs[-1]) < (17 << 20)
    rng = np.random.default_rng(1100)
    m = data.copy()
    at = rng.choice(n - 4, n // 3, replace=False)
    m[offs[at].astype(np.int64) + 13 + rng.integers(0, 200, len(at))] ^= 0x04
    for i in (5, n // 2, n - 1):
        m[int(offs[i]) + 5] ^= 1
    want_v, want_e, want_t, info = expect_raw(m, offs)
    assert_anti_vacuity(info)
    cap = want_t["n_elems"]
    hv, he, ha, ht = raw_pipe.decode_host(m, offs, cap)
    dv, de, da, dt = _device_decode(raw_pipe, m, offs, cap)
    assert_flat_equal((hv, he), (dv, de), "chunked host == one device call")
    assert ht == dt == want_t and np.array_equal(ha, da)
    assert_flat_equal((hv, he), (want_v, want_e), "chunked host == expectation")
    _check(raw_pipe, m, offs, "overflow re-decode", elem_cap=cap - 1, vacuity=False)


# ---- 12. shards -------------------------------------------------------------------------------------------
def test_flat_rebase_of_raw_shards(raw_pipe):
    rng = np.random.default_rng(1200)
    data, offs = rr.gen_batch(4, 4000)
    blobs = with_len_defects(corrupt_in_place(split_blobs(data, offs), rng, 0.3), rng)
    data, offs = batch_from_blobs(blobs)
    want_v, want_e, want_t, info = expect_raw(data, offs)
    assert_anti_vacuity(info)
    plan = rr.shard_plan(offs, 2)
    vs, es, eadd = [], [], 0
    for v0, v1, b0, b1 in [[int(x) for x in row] for row in plan]:
        so = offs[v0:v1 + 1] - np.uint64(b0)
        sd = np.zeros((b1 - b0 + 15) & ~15, np.uint8)
        sd[:b1 - b0] = data[b0:b1]
        v, e, a, t = raw_pipe.decode_host(sd, so)
        dv = torch.from_numpy(v.view(np.uint8).copy()).cuda()
        de = torch.from_numpy(e.view(np.uint8).copy()).cuda() if len(e) else torch.zeros(16, dtype=torch.uint8, device="cuda")
        raw_pipe.flat_rebase(dv, de[:len(e) * 16], eadd, b0)
        torch.cuda.synchronize()
        vs.append(dv.cpu().numpy().view(rr.VALUE_DT))
        es.append(de.cpu().numpy()[:len(e) * 16].view(rr.ELEM_DT))
        eadd += t["n_elems"]
    assert_flat_equal((np.concatenate(vs), np.concatenate(es)), (want_v, want_e), "rebased raw shards")
    assert eadd == want_t["n_elems"]


# ---- the compat shim's GPU route ----------------------------------------------------------------------------
def test_compat_shim_check_off_on_gpu_route(tmp_path):
    """tests/c/test_compat_zlraw.c, gpu-off: with the ziplist check off rr_compat_des_batch on the
    GPU route (RR_CTX_ZL_RAW on the shim's context) builds the objects the host route builds, and a
    wrong byte count still panics there."""
    import os
    import subprocess

    from test_compat import build
    exe = build(str(tmp_path), "test_compat_zlraw")
    env = {k: v for k, v in os.environ.items() if k != "RR_COMPAT_ZL_CHECK"}
    r = subprocess.run([exe, "gpu-off"], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "reference acceptance" in r.stdout
