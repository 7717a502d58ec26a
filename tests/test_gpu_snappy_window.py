"""GPU snappy decompression on the LDS window's own paths and edges (dec_block_lds in
redrock_old_amd/csrc/rr_snappy.hip) against the CPU oracle: the bail-out to the global path,
the 64-tag batch and the 64-position speculation round at their boundaries, the back-reference
copies over offset x length x alignment, a fuzz that stays on the LDS path, the grid-stride
loops of both directions on their second iteration, and nothing written outside the output.
The streams come from tests/snappy_streams.py; tests/test_snappy_streams.py (CPU) pins each to
the oracle and to the path it is meant for."""
import os

import numpy as np
import pytest
import torch

import redrock_old_amd as rr
import snappy_streams as ss
from oracle import cpu
from snappy_corpus import corpus

pytestmark = pytest.mark.gpu


def check_at(engine, streams, alignments, what):
    """check_decompress of test_gpu_snappy.py with block i at address alignments[i] mod 4:
    statuses, and outputs where the status is OK, equal to cpu.snappy_uncompress's."""
    data, offs, real = ss.pack_at(streams, alignments)
    assert [int(offs[r]) & 3 for r in real] == list(alignments)
    want = [cpu.snappy_uncompress(s) for s in streams]
    total = sum(cpu.snappy_length(s)[1] for s in streams)
    out, ooffs, st = engine.snappy_decompress_host(data, offs, total)
    fill = np.ones(len(st), bool)
    fill[real] = False
    assert not st[fill].any(), f"{what}: a filler block's status"
    for i, (wst, wout) in enumerate(want):
        b = int(real[i])
        assert int(st[b]) == wst, f"{what}: stream {i} status {rr.SNAPPY_STATUS[int(st[b])]} vs {rr.SNAPPY_STATUS[wst]}"
        if wst == 0:
            assert out[int(ooffs[b]):int(ooffs[b + 1])].tobytes() == wout, f"{what}: stream {i} output differs"


def check_cases(engine, cases, what):
    check_at(engine, [c.stream for c in cases], [c.s0 for c in cases], what)


def test_bail_out(engine):
    """Blocks whose output catches up with their staged bytes (by a copy, by a literal) at every
    s0, ordinary blocks around them; blocks rejected after and before their bail point."""
    cases = ss.family_bail()
    assert sum(c.route.startswith("bail") for c in cases) >= 24
    check_cases(engine, cases, "bail-out")


def test_batch_boundaries(engine):
    check_cases(engine, ss.family_batch(), "batch boundaries")


def test_speculation_window(engine):
    check_cases(engine, ss.family_spec(), "speculation window")


@pytest.mark.parametrize("front", [False, True], ids=["lds", "global"])
def test_backreference_matrix(engine, front):
    check_cases(engine, ss.family_matrix(front), "back-reference matrix")


def test_fuzz_lds_valid_and_mutated(engine):
    """300 generated valid streams and a mutated round of them (and of compressed corpus
    prefixes), all entering the LDS path.  RR_FUZZ_ROUNDS=k runs k seeds (an extended run)."""
    for k in range(int(os.environ.get("RR_FUZZ_ROUNDS", "1"))):
        seed = 1 + 7919 * k
        check_cases(engine, ss.fuzz_valid(seed), f"fuzz valid, seed {seed}")
        mutated = ss.fuzz_mutated(seed)
        check_at(engine, [s for s, _ in mutated], [a for _, a in mutated], f"fuzz mutated, seed {seed}")


# ---- device entry points ----------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _decompress_device(engine, data, offs, out_cap, fill=0):
    n = len(offs) - 1
    d_out = torch.full((out_cap,), fill, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.snappy_decompress_device(_dev(data), _dev(offs), d_out, d_oo, d_st)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_oo.cpu().numpy().view(np.uint64), d_st.cpu().numpy()


def _compress_device(engine, data, offs, fill=0):
    n = len(offs) - 1
    cap = int(rr.lib().rr_snappy_compress_bound(n, data.size))
    d_out = torch.full((cap,), fill, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    engine.snappy_compress_device(_dev(data), _dev(offs), d_out, d_oo)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_oo.cpu().numpy().view(np.uint64)


def _pack_np(parts):
    """(data padded to 16 bytes, offsets) of numpy byte arrays, contiguous."""
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([p.size for p in parts])
    raw = np.concatenate(parts)
    data = np.zeros((raw.size + 15) & ~15, np.uint8)
    data[:raw.size] = raw
    return data, offs


GRID = 1 << 20     # grid_for's cap in rr_snappy.hip: a workgroup a block up to here
REAL = 64          # real blocks at either end


def _grid_stride_blocks():
    """(inputs, streams) of the 128 real blocks: 16 KiB pieces of text and random bytes, and the
    outputs / streams of two bailing blocks."""
    c = corpus()
    text = c["text_150k"]
    plain = [text[k:k + 16384] for k in range(0, len(text), 16384)] + [c["random_16k"]]
    bails = [ss.bail_copy_rle().finish(), ss.bail_copy_far().finish()]
    assert [ss.route(s)[0] for s, _ in bails] == ["bail-copy", "bail-copy"]
    inputs = plain + [out for _, out in bails]
    streams = [cpu.snappy_compress(x) for x in plain] + [s for s, _ in bails]
    pick = [k % len(inputs) for k in range(2 * REAL)]
    return [inputs[k] for k in pick], [streams[k] for k in pick]


def _with_tiny(real, tiny):
    n_tiny = GRID + REAL - 2 * REAL
    parts = [np.frombuffer(x, np.uint8) for x in real[:REAL]] + [np.tile(np.frombuffer(tiny, np.uint8), n_tiny)]
    parts += [np.frombuffer(x, np.uint8) for x in real[REAL:]]
    sizes = np.concatenate([[len(x) for x in real[:REAL]], np.full(n_tiny, len(tiny)), [len(x) for x in real[REAL:]]])
    offs = np.zeros(sizes.size + 1, np.uint64)
    offs[1:] = np.cumsum(sizes)
    raw = np.concatenate(parts)
    data = np.zeros((raw.size + 15) & ~15, np.uint8)
    data[:raw.size] = raw
    return data, offs


def _check_with_tiny(got, goffs, real, tiny, what):
    want_data, want_offs = _with_tiny(real, tiny)
    assert np.array_equal(goffs, want_offs), f"{what}: offsets"
    end = int(want_offs[-1])
    a, b = int(want_offs[REAL]), int(want_offs[GRID])
    assert np.array_equal(got[:a], want_data[:a]), f"{what}: first real blocks"
    assert np.array_equal(got[b:end], want_data[b:end]), f"{what}: last real blocks (the loops' second iteration)"
    mid = got[a:b].reshape(-1, len(tiny))
    assert (mid == np.frombuffer(tiny, np.uint8)).all(), f"{what}: tiny blocks"


def test_grid_stride_second_iteration(engine):
    """2^20 + 64 blocks: the kernels launch 2^20 workgroups, so the first 64 take a second block
    each, with the first one's bytes still in their LDS window / hash table.  Real blocks at
    both ends, a million one-byte blocks (3-byte streams) in between."""
    inputs, streams = _grid_stride_blocks()
    tiny_in, tiny_z = b"a", b"\x01\x00a"
    assert cpu.snappy_compress(tiny_in) == tiny_z and cpu.snappy_uncompress(tiny_z) == (0, tiny_in)
    for x, z in zip(inputs, streams):
        assert cpu.snappy_uncompress(z) == (0, x)
    # compress
    data, offs = _with_tiny(inputs, tiny_in)
    assert len(offs) - 1 == GRID + REAL
    got, goffs = _compress_device(engine, data, offs)
    _check_with_tiny(got, goffs, [cpu.snappy_compress(x) for x in inputs], tiny_z, "compress")
    # decompress
    data, offs = _with_tiny(streams, tiny_z)
    second = [ss.route(z, int(offs[GRID + k]) & 3)[0] for k, z in enumerate(streams[REAL:])]
    assert second.count("bail-copy") >= 8 and second.count("lds") >= 40    # both paths on the second iteration
    total =sum(len(x) for x in inputs) + GRID - REAL
    got, goffs, st = _decompress_device(engine, data, offs, (total + 64 + 15) & ~15)
    assert not st.any(), f"statuses {np.flatnonzero(st)[:8]}"
    _check_with_tiny(got, goffs, inputs, tiny_in, "decompress")


@pytest.mark.parametrize("family", ["bail", "matrix"])
def test_nothing_written_outside(engine, family):
    """Output buffers pre-filled with 0xA5: every byte past the last offset is still 0xA5 after
    decompressing the family's batch (capacity 64+ bytes past the output) and after compressing
    its outputs (capacity: the bound)."""
    cases = ss.family_bail() if family == "bail" else ss.family_matrix()
    data, offs, real = ss.pack_at([c.stream for c in cases], [c.s0 for c in cases])
    total = sum(cpu.snappy_length(c.stream)[1] for c in cases)
    out, ooffs, st = _decompress_device(engine, data, offs, (total + 64 + 15) & ~15, fill=0xA5)
    assert int(ooffs[-1]) == total
    assert (out[total:] == 0xA5).all() and out.size - total >= 64
    for i, c in enumerate(cases):
        b = int(real[i])
        assert int(st[b]) == c.status
        if c.status == 0:
            assert out[int(ooffs[b]):int(ooffs[b + 1])].tobytes() == cpu.snappy_uncompress(c.stream)[1]
    inputs = [c.expected for c in cases if c.status == 0]
    data, offs = _pack_np([np.frombuffer(x, np.uint8) for x in inputs])
    got, goffs = _compress_device(engine, data, offs, fill=0xA5)
    want = [cpu.snappy_compress(x) for x in inputs]
    assert [int(x) for x in np.diff(goffs.astype(np.int64))] == [len(w) for w in want]
    assert got[:int(goffs[-1])].tobytes() == b"".join(want)
    assert (got[int(goffs[-1]):] == 0xA5).all() and got.size > int(goffs[-1])
