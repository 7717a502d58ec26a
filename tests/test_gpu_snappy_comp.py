"""GPU snappy compression on the compressor's own paths and edges (snz_comp_kernel and
snz_pack_kernel in redrock_old_amd/csrc/rr_snappy.hip): every lane, candidate source and stride
regime of a 16-probe round, same-round hash collisions at both table sizes, step 3's repeats and
exits, copy lengths x offsets, literal lengths x destination x source alignment, every size around a
threshold with the last block ending at data_cap, the pack kernel's head / body / tail split at every
out_offs & 15, the grid-stride loops past 4 x 2^20 blocks and an arena past 4 GiB.  Every comparison
is byte equality with cpu.snappy_compress, plus the offsets.  The inputs come from
tests/snappy_comp_streams.py; tests/test_snappy_comp_streams.py (CPU) proves which cells they hold
and that each modelled kernel defect changes the bytes of one of them."""
import functools

import numpy as np
import pytest
import torch

import redrock_old_amd as rr
import snappy_comp_streams as cs
import snappy_reference as sref
from oracle import cpu

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
ROOM = 256


@functools.lru_cache(None)
def batch(family):
    """(names, blocks, the oracle's streams) of a family, the literals behind their fillers."""
    fam = getattr(cs, "family_" + family)()
    if family == "literals":
        blocks, real = cs.place([b for _, b, _ in fam], [al for _, _, al in fam])
        names = ["filler"] * len(blocks)
        for r, (n, _, _) in zip(real, fam):
            names[r] = n
        st = cs.starts(blocks)
        assert [(st[r][0] & 15, st[r][1] & 3) for r in real] == [al for _, _, al in fam]
    else:
        names, blocks = [n for n, _ in fam], [b for _, b in fam]
    want = [cpu.snappy_compress(b) for b in blocks]
    return names, blocks, want


def compare(got, goffs, family, what):
    names, blocks, want = batch(family)
    woffs = np.zeros(len(want) + 1, np.uint64)
    woffs[1:] = np.cumsum([len(w) for w in want])
    bad = [(names[i], len(blocks[i])) for i, w in enumerate(want)
           if got[int(goffs[i]):int(goffs[i + 1])].tobytes() != w]
    assert not bad, f"{family}, {what}: {len(bad)} of {len(want)} blocks differ from the oracle, first {bad[:6]}"
    assert np.array_equal(goffs, woffs), f"{family}, {what}: offsets"


def compress_device(engine, data, offs, shift):
    """The device entry point with out->data at a 256-byte aligned address + 256 + shift, sentinel
    bytes in front of it and behind.  Returns (the bytes from out->data on, offsets)."""
    n = len(offs) - 1
    cap = int(rr.lib().rr_snappy_compress_bound(n, data.size))
    buf = torch.full((ROOM + shift + cap + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d, o = torch.from_numpy(data).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    engine.snappy_compress_device(d, o, buf[ROOM + shift:ROOM + shift + cap], oo)
    torch.cuda.synchronize()
    got, goffs = buf.cpu().numpy(), oo.cpu().numpy().view(np.uint64)
    assert (got[:ROOM + shift] == SENTINEL).all(), f"shift {shift}: bytes in front of out->data"
    assert (got[ROOM + shift + int(goffs[-1]):] == SENTINEL).all(), f"shift {shift}: bytes past out_offsets[n]"
    return got[ROOM + shift:], goffs


FAMILIES = ("rounds", "collisions", "step3", "copies", "literals", "sizes", "pack")


@pytest.mark.parametrize("family", FAMILIES)
def test_family(engine, family):
    """The family through snappy_compress_host and through snappy_compress_device at an output
    address = 0..3 mod 4 (snz_pack_kernel's 16-byte stores at every address mod 4) with sentinels
    around the output; the sizes family's last block ends exactly at data_cap.  Then the GPU's
    bytes back through snappy_decompress_device and through pyarrow's snappy."""
    import pyarrow as pa
    names, blocks, want = batch(family)
    data, offs = cs.pack(blocks)
    assert family != "sizes" or data.size == int(offs[-1])
    got, goffs = engine.snappy_compress_host(data, offs)
    compare(got, goffs, family, "host")
    for shift in range(4):
        got, goffs = compress_device(engine, data, offs, shift)
        compare(got, goffs, family, f"device, shift {shift}")
    total, n = int(goffs[-1]), len(blocks)
    z16 = np.zeros((total + 15) & ~15, np.uint8)
    z16[:total] = got[:total]
    d_z = torch.from_numpy(z16).cuda()
    d_zo = torch.from_numpy(goffs.view(np.int64)).cuda()
    d_back = torch.full((int(offs[-1]) + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.snappy_decompress_device(d_z, d_zo, d_back[:int(offs[-1])], d_bo, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    assert np.array_equal(d_bo.cpu().numpy().view(np.uint64), offs)
    back = d_back.cpu().numpy()
    assert back[:int(offs[-1])].tobytes() == b"".join(blocks) and (back[int(offs[-1]):] == SENTINEL).all()
    for i, b in enumerate(blocks):
        z = got[int(goffs[i]):int(goffs[i + 1])].tobytes()
        assert pa.decompress(z, decompressed_size=len(b), codec="snappy", asbytes=True) == b, names[i]


def test_grid_strides(engine):
    """4 x 2^20 + 3001 blocks of 0..3 bytes through the device entry point: snz_comp_kernel (2^20
    workgroups of a wave) takes up to five blocks a wave, snz_pack_kernel (2^20 workgroups of four
    waves) a second one.  Expected bytes and offsets: the oracle's for the 61-block base, tiled
    (tests/test_snappy_comp_streams.py holds the tiling to the oracle), compared on the device."""
    base = cs.grid_base()
    n, t = cs.GRID_N, -(-cs.GRID_N // cs.GRID_BASE)
    assert n > cs.PACK_WPB * cs.GRID_CAP
    want = [cpu.snappy_compress(b) for b in base]
    bin_, bout = np.zeros(len(base) + 1, np.uint64), np.zeros(len(base) + 1, np.uint64)
    bin_[1:], bout[1:] = np.cumsum([len(b) for b in base]), np.cumsum([len(w) for w in want])
    ioffs, eoffs = cs.tile_offsets(bin_, n), cs.tile_offsets(bout, n)
    raw = np.zeros((int(ioffs[-1]) + 15) & ~15, np.uint8)
    raw[:int(ioffs[-1])] = np.tile(np.frombuffer(b"".join(base), np.uint8), t)[:int(ioffs[-1])]
    exp = np.tile(np.frombuffer(b"".join(want), np.uint8), t)[:int(eoffs[-1])]
    cap = int(rr.lib().rr_snappy_compress_bound(n, raw.size))
    buf = torch.full((ROOM + cap + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    engine.snappy_compress_device(torch.from_numpy(raw).cuda(), torch.from_numpy(ioffs).cuda(), buf[ROOM:ROOM + cap], oo)
    torch.cuda.synchronize()
    d_eoffs = torch.from_numpy(eoffs).cuda()
    if not torch.equal(oo, d_eoffs):
        k = int(torch.nonzero(oo != d_eoffs)[0])
        raise AssertionError(f"offsets differ from block {k} on: {int(oo[k])} vs {int(eoffs[k])}")
    got, d_exp = buf[ROOM:ROOM + exp.size], torch.from_numpy(exp).cuda()
    if not torch.equal(got, d_exp):
        at = int(torch.nonzero(got != d_exp)[0])
        raise AssertionError(f"bytes differ from {at} on, in block {int(np.searchsorted(eoffs, at, 'right')) - 1} of {n}")
    assert bool((buf[:ROOM] == SENTINEL).all()) and bool((buf[ROOM + exp.size:] == SENTINEL).all())


def test_arena_past_4_gib():
    """Blocks of 16381 bytes, half text and half random bytes, tiled on the device past 2^32 + 2^24
    bytes: block starts past 2^32 at every address mod 16, offsets and bytes against the base's oracle
    output tiled.  A fresh Engine, closed afterwards, so the session's context keeps its scratch."""
    bs, nbase = 16381, 61
    text = sref.read("alice29.txt") + sref.read("html")
    rng = np.random.default_rng(4)
    base = [text[4001 * k:4001 * k + bs] if k & 1 else rng.integers(0, 256, bs, dtype=np.uint8).tobytes()
            for k in range(nbase)]
    assert all(len(b) == bs for b in base) and (bs * nbase) % 16 != 0
    want = [cpu.snappy_compress(b) for b in base]
    assert sum(len(w) < bs * 3 // 4 for w in want) == nbase // 2        # (the text half compresses)
    raw, exp = np.frombuffer(b"".join(base), np.uint8), np.frombuffer(b"".join(want), np.uint8)
    t = -(-((1 << 32) + (1 << 24)) // raw.size)
    n = t * nbase
    starts = np.arange(n + 1, dtype=np.int64) * bs
    assert int(starts[-1]) > (1 << 32) + (1 << 24)
    assert {int(x) & 15 for x in starts[:-1][starts[:-1] >= 1 << 32]} == set(range(16))
    bout = np.zeros(nbase + 1, np.int64)
    bout[1:] = np.cumsum([len(w) for w in want])
    eoffs = np.append((np.arange(t, dtype=np.int64)[:, None] * exp.size + bout[None, :-1]).ravel(), t * exp.size)
    eng = rr.Engine(0)
    try:
        d_data = torch.zeros((t * raw.size + 15) & ~15, dtype=torch.uint8, device="cuda")      # (data_cap: a multiple of 16)
        d_data[:t * raw.size].view(t, raw.size).copy_(torch.from_numpy(raw.copy()).cuda().expand(t, raw.size))
        cap = int(rr.lib().rr_snappy_compress_bound(n, d_data.numel()))
        buf = torch.full((ROOM + cap + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda")
        oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        eng.snappy_compress_device(d_data, torch.from_numpy(starts).cuda(), buf[ROOM:ROOM + cap], oo)
        torch.cuda.synchronize()
        d_eoffs = torch.from_numpy(eoffs).cuda()
        if not torch.equal(oo, d_eoffs):
            k = int(torch.nonzero(oo != d_eoffs)[0])
            raise AssertionError(f"offsets differ from block {k} on (input byte {k * bs}): {int(oo[k])} vs {int(eoffs[k])}")
        del d_data
        total = t * exp.size
        d_exp = torch.from_numpy(exp.copy()).cuda()
        step = 256                                              # tiles compared at once
        for k in range(0, t, step):
            m = min(step, t - k)
            got = buf[ROOM + k * exp.size:ROOM + (k + m) * exp.size].view(m, exp.size)
            if not bool((got == d_exp).all()):
                row = int(torch.nonzero((got != d_exp).any(1))[0])
                at = int(torch.nonzero(got[row] != d_exp)[0])
                blk = int(np.searchsorted(bout, at, "right")) - 1
                raise AssertionError(f"tile {k + row}, base block {blk} (input byte {((k + row) * nbase + blk) * bs}): "
                                     f"compressed byte {at - int(bout[blk])} of the block differs")
        assert bool((buf[:ROOM] == SENTINEL).all()) and bool((buf[ROOM + total:] == SENTINEL).all())
    finally:
        eng.close()
