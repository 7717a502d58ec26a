"""GPU LZ4 on the paths a wave-parallel kernel goes wrong on (lz4_dec_kernel / lz4_comp_kernel in
redrock_old_amd/csrc/rr_lz4.hip): the bail-out from the LDS window to the global path on its
boundary, the wave's copies over length x offset x alignment on both paths, a fuzz of generated
blocks and their mutants, output at every address mod 4 with nothing written outside a block's
range, the compressor's stores at every input and slot alignment, its length extensions around
15 + 255 * 64, periodic inputs across 64 KiB chunks, and both block codecs on a caller's stream
and under graph replay.  Expected bytes are the builders' own (tests/lz4_window_streams.py),
verdicts tests/lz4_reference.py's; tests/test_lz4_window_streams.py (CPU) pins every stream to the
path it is meant for and proves the coverage conditions."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import redrock_old_amd as rr
import lz4_reference as ref
import lz4_streams
import lz4_window_streams as ws
from test_gpu_lz4 import check_compressed, pack

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@contextlib.contextmanager
def window(w):
    """RR_LZ4_DEC_WINDOW for the calls inside (None: the compiled window), restored after."""
    old = os.environ.get("RR_LZ4_DEC_WINDOW")
    try:
        if w is None:
            os.environ.pop("RR_LZ4_DEC_WINDOW", None)
        else:
            os.environ["RR_LZ4_DEC_WINDOW"] = str(w)
        yield
    finally:
        if old is None:
            os.environ.pop("RR_LZ4_DEC_WINDOW", None)
        else:
            os.environ["RR_LZ4_DEC_WINDOW"] = old


def announced(stream):
    h = ref.read_varint32(stream)
    return h[0] if h else 0


def decompress_device(engine, data, offs, cap, fill=0, shift=0, room=64, alloc=None):
    """The device entry point with out->data at a 256-byte aligned buffer + shift (the buffer:
    alloc bytes, or data_cap, and room).  Returns (the whole buffer, offsets, status)."""
    n = len(offs) - 1
    d, o = torch.from_numpy(data).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    buf = torch.full((shift + max(cap, alloc or 0) + room,), fill, dtype=torch.uint8, device="cuda")
    oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    inb = rr.BlobBatch(d.data_ptr(), o.data_ptr(), n, d.numel())
    outb = rr.BlobBatch(buf.data_ptr() + shift, oo.data_ptr(), n, cap)
    rr._check(engine._L.rr_lz4_decompress_batch(engine._ctx, C.byref(inb), C.byref(outb), C.c_void_p(st.data_ptr()), None))
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert (st[n:] == 0xEE).all()
    return buf.cpu().numpy(), oo.cpu().numpy().view(np.uint64), st[:n]


def run_at(engine, streams, alignments, entry):
    """(per real stream: status, output bytes; the offsets of the real streams' outputs)."""
    data, offs, real = ws.pack_at(streams, alignments)
    assert [int(offs[r]) & 15 for r in real] == [a & 15 for a in alignments]
    total = sum(announced(s) for s in streams)
    if entry == "host":
        out, oo, st = engine.lz4_decompress_host(data, offs, total)
    else:
        out, oo, st = decompress_device(engine, data, offs, total, fill=SENTINEL)
        assert (out[total:] == SENTINEL).all()
    assert int(oo[-1]) == total
    fill = np.ones(len(st), bool)
    fill[real] = False
    parts = [data[int(offs[i]):int(offs[i + 1])].tobytes() for i in np.flatnonzero(fill)]
    assert [int(x) for x in st[fill]] == [ref.OK if p == ws.FILL_OK else ref.E_TRUNC for p in parts]
    return ([int(st[r]) for r in real], [out[int(oo[r]):int(oo[r + 1])].tobytes() for r in real],
            [int(oo[r]) for r in real])


def first_diff(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if a.size != b.size:
        return min(a.size, b.size)
    d = np.flatnonzero(a != b)
    return int(d[0]) if d.size else -1


def check_cases(engine, cases, entry, what):
    st, outs, oo = run_at(engine, [c.stream for c in cases], [c.s0 for c in cases], entry)
    bad = []
    for i, c in enumerate(cases):
        if st[i] != c.status:
            bad.append((c.name, ref.STATUS_NAMES.get(st[i], st[i]), ref.STATUS_NAMES[c.status]))
        elif c.status == ref.OK and outs[i] != c.expected:
            at = first_diff(outs[i], c.expected)
            k, e = ws.sequence_at(c, at)
            bad.append((c.name, f"byte {at} differs, in copy {k}: {e}", ws.regime(e) if e else None))
    assert not bad, f"{what} ({entry}): {len(bad)} of {len(cases)} differ, first {bad[:4]}"
    return st, outs, oo


def same_as(res, res0, cases, what):
    """Status, offsets and OK bytes of two runs of the same cases."""
    assert res[0] == res0[0] and res[2] == res0[2], what
    for i, c in enumerate(cases):
        if res[0][i] == ref.OK:
            assert res[1][i] == res0[1][i], (what, c.name)


def test_bail_out(engine):
    """Every bail family stream under the window it was built for, at its alignment: blocks on
    the boundary of LdsMem::match's test (they stay), one byte past it (the global path redoes
    them, 483 assembled bytes included), rejected after and before the bail point, and the entry
    test's edges.  Then under window 0: the same statuses, offsets and bytes."""
    for w in ws.WINDOWS:
        cases = [c for c in ws.family_bail() if c.w == w]
        assert sum(c.route == "bail-match" for c in cases) >= 20 and sum(c.kind == "eq" for c in cases) >= 8
        with window(w):
            res = check_cases(engine, cases, "host", f"bail-out, window {w}")
        with window(0):
            res0 = check_cases(engine, cases, "host", f"bail-out streams of window {w} under window 0")
        same_as(res, res0, cases, f"window {w} against 0")


@pytest.mark.parametrize("entry", ["host", "device"])
def test_copy_matrix(engine, entry):
    """The copy matrix under the default window (lds_copy's three regimes and the modulo rounds,
    every source and destination alignment) and under window 0 (GlobalMem::literals and
    GlobalMem::match: a wave reading back through the L2 what it has just stored)."""
    cases = ws.family_matrix()
    with window(None):
        res = check_cases(engine, cases, entry, "copy matrix, default window")
    with window(0):
        res0 = check_cases(engine, cases, entry, "copy matrix, window 0")
    same_as(res, res0, cases, "default window against 0")


def test_fuzz(engine):
    """Generated valid blocks and two mutants of each under the default window, 4096 and 0.
    RR_FUZZ_ROUNDS=k runs k seeds (an extended run)."""
    for k in range(int(os.environ.get("RR_FUZZ_ROUNDS", "1"))):
        seed = 1 + 7919 * k
        valid, mutated = ws.fuzz_valid(seed), ws.fuzz_mutated(seed)
        streams, at = [s for s, _ in mutated], [a for _, a in mutated]
        want = [ref.decode(s) for s in streams]
        got = {}
        for w in (None, 4096, 0):
            with window(w):
                check_cases(engine, valid, "host", f"fuzz valid, seed {seed}, window {w}")
                st, outs, oo = got[w] = run_at(engine, streams, at, "host")
            for i, (wst, wout, _) in enumerate(want):
                assert st[i] == wst, f"mutant {i}, seed {seed}, window {w}: {ref.STATUS_NAMES.get(st[i], st[i])} vs {ref.STATUS_NAMES[wst]}"
                if wst == ref.OK:
                    assert outs[i] == wout, f"mutant {i}, seed {seed}, window {w}: byte {first_diff(outs[i], wout)}"
        assert got[4096][2] == got[None][2] == got[0][2]


def _small_blocks():
    """[(stream, status, bytes)]: accepted blocks of 0..70 and 127..133 bytes in two forms (one
    literal run; a literal, a match at offset 1, a last run), with rejected ones between them:
    a bad preamble (no output range), and blocks the global path rejects after it has written."""
    rng = np.random.default_rng(41)
    b = lz4_streams.Block().seq(lz4_streams._lits(20, 9), 8, 20).seq(b"final")
    rejects = [(b"\x85", ref.E_HEADER), (b.stream()[:-1], ref.E_TRUNC), (b.stream(len(b.out) - 1), ref.E_OVERFLOW),
               (b"\xff\xff\xff\xff\x7f", ref.E_HEADER), (b.stream() + b"!", ref.E_OVERFLOW)]
    out = []
    for n in list(range(71)) + list(range(127, 134)):
        forms = [ws.Seqs(rng).rseq(n)] if n else []
        last = 5 + (n & 3)
        if n >= 13:      # (a run that ends within 12 bytes of N must be the last one)
            forms.append(ws.Seqs(rng).rseq(1, 1, n - 1 - last).rseq(last))
        for f in forms:
            out.append((f.stream(), ref.OK, bytes(f.out)))
        if n == 0:
            out.append((b"\x00\x00", ref.OK, b""))
        r = rejects[n % len(rejects)]
        out.append((r[0], r[1], None))
    for s, st, data in out:
        assert ref.decode(s)[:2] == (st, data)
    return out


@pytest.mark.parametrize("shift", range(4))
def test_output_alignment_and_nothing_outside(engine, shift):
    """out->data at an address = shift mod 4 (rr_lz4.h asks no alignment of out): the head / dword
    / tail split of the window's write-out, and the global path's byte stores.  Sentinel fill:
    accepted blocks exact, a bad preamble's range empty, nothing before out->data, past
    offsets[n], or from the first block cut by data_cap on.  Failed blocks write (inside their
    range) only on the global path: window 0 is the run that matters for them."""
    blocks = _small_blocks()
    streams = [s for s, _, _ in blocks]
    data, offs = pack(streams)
    total = sum(announced(s) for s in streams)
    ends = np.cumsum([announced(s) for s in streams])
    cut = int(ends[len(streams) * 3 // 4]) + 3          # inside a block of the last quarter
    assert sum(st == ref.OK for _, st, _ in blocks) >= 140 and {st for _, st, _ in blocks} >= {1, 2, 4}
    for w in (None, 0):
        for cap in (total, cut):
            with window(w):
                buf, oo, st = decompress_device(engine, data, offs, cap, fill=SENTINEL, shift=shift, room=256, alloc=total)
            what = f"shift {shift}, window {w}, data_cap {cap}"
            assert (buf[:shift] == SENTINEL).all(), what
            out = buf[shift:]
            first_cut, ncap = None, 0
            for i, (s, wst, wout) in enumerate(blocks):
                o0, o1 = int(oo[i]), int(oo[i + 1])
                assert o1 - o0 == announced(s), (what, i)
                if wst == ref.E_HEADER:
                    assert st[i] == ref.E_HEADER and o0 == o1, (what, i)
                elif o1 > cap:
                    assert st[i] == ref.E_CAPACITY, (what, i, int(st[i]))
                    first_cut = o0 if first_cut is None else first_cut
                    ncap += 1
                else:
                    assert st[i] == wst, (what, i, int(st[i]), wst)
                    if wst == ref.OK:
                        assert out[o0:o1].tobytes() == wout, (what, i, len(wout), first_diff(out[o0:o1].tobytes(), wout))
            assert int(oo[-1]) == total
            if cap == cut:
                assert ncap >= 10 and first_cut <= cap, what
                assert (out[first_cut:] == SENTINEL).all(), what    # a block past data_cap writes nothing, nor any after it
            else:
                assert ncap == 0 and (out[total:] == SENTINEL).all() and out.size - total >= 64, what


# ---- compression ---------------------------------------------------------------------------------
ALIGN_SIZES = (13, 64, 65, 68) + tuple(range(1023, 1033)) + (16384,)


def _align_fills(n, seed):
    rnd = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    planted = rnd.copy()
    if n >= 200:
        planted[n // 2 + 8:n // 2 + 72] = planted[8:72]
    elif n >= 40:
        planted[n // 2:n // 2 + 8] = planted[:8]
    return [bytes(n), rnd.tobytes(), (b"abcdefg" * (n // 7 + 1))[:n], planted.tobytes()]


def test_compress_alignment_matrix(engine):
    """One set of buffers behind a first block of 0..15 bytes: every c0 & 3 (Src's shifts) and
    every slot address mod 4 (Out::bytes' head / dword / tail split).  The same bytes at all 16
    positions, and valid ones."""
    bufs = [f for k, n in enumerate(ALIGN_SIZES) for f in _align_fills(n, 300 + k)]
    front = lz4_streams._lits(15, 4)
    blocks = None
    for j in range(16):
        data, offs = pack([front[:j]] + bufs)
        assert int(offs[1]) == j
        comp, co = engine.lz4_compress_host(data, offs)
        got = [comp[int(co[i + 1]):int(co[i + 2])].tobytes() for i in range(len(bufs))]
        if blocks is None:
            blocks = got
            check_compressed([front[:j]] + bufs, comp, co, "alignment matrix")
        for i, b in enumerate(bufs):
            assert got[i] == blocks[i], f"block {i} ({len(b)} bytes) behind {j} bytes: byte {first_diff(got[i], blocks[i])}"
    assert any(len(blocks[i]) < len(b) for i, b in enumerate(bufs))


EXT_T = (15, 270, 15 + 255 * 64, 15 + 255 * 65)   # a length's first, second, 65th and 66th extension byte
ROUND_POS = 64                                     # positions lz4_comp_kernel probes a round


def _distinct(n, base):
    """n bytes in which no four consecutive bytes occur twice: the 16-bit values (i + base) * 513,
    low byte first (from one value to the next the low byte moves by 1 and the high byte by 2, so
    a group of four at an even index differs from every one at an odd index, and two bytes 128
    apart differ); base + n / 2 < 65536."""
    v = ((np.arange((n + 1) // 2 + 1, dtype=np.uint32) + base) * 513).astype("<u2")
    return v.view(np.uint8)[:n].tobytes()


def _run_input(lit, K):
    """The issue's shape: lit bytes without a repeat, one byte K times, 12 more bytes."""
    return _distinct(lit, 100) + b"\xee" * K + _distinct(12, 60000)


def _planted_input(L):
    """A first sequence that ends at byte 240, then L bytes without a repeat, then 40 bytes that
    occurred 128 or more bytes (two rounds of the match finder) earlier, then 12 more bytes: a
    greedy finder that takes the first position whose four bytes it has seen emits a literal run
    of exactly L."""
    pre = _distinct(200, 100)
    pre += pre[72:112]
    y = _distinct(L, 20000)
    src = (pre + y)[240 + L - 128:240 + L - 88] if L >= 168 else pre[100:140]
    return pre + y + src + _distinct(12, 60000)


def test_length_extension_edges(engine):
    """Out::ext around one extension byte, two, 64 (one round of its loop) and 65 (a second round).
    Inputs of lit distinct bytes, a run of K equal bytes and 12 more, lit and K each through
    t - 2 .. t + 2 for every t of EXT_T.  The match finder looks a round of 64 positions up in the
    table before it inserts them, so it finds such a run at the next multiple of
    64 and never emits a literal run of t bytes for it; the guard below would not hold on those
    inputs alone.  So K also runs through t + 4 + (64 - lit) - 2 .. + 2, which gives matches of
    t - 2 .. t + 2 past the 4 implied bytes, and _planted_input() gives literal runs of exactly
    t - 2 .. t + 2.  The guard reads the GPU's own sequences: if the encoder's choices change so
    that the lengths around any t are no longer all met, it fails."""
    sweep = [t + d for t in EXT_T for d in range(-2, 3)]
    lit0, k0 = 20, 40
    bufs = [_run_input(lit, k0) for lit in sweep] + [_run_input(lit0, K) for K in sweep]
    bufs += [_run_input(lit0, K + 4 + ROUND_POS - lit0) for K in sweep] + [_planted_input(L) for L in sweep]
    data, offs = pack(bufs)
    comp, co = engine.lz4_compress_host(data, offs)
    check_compressed(bufs, comp, co, "length extensions")
    lits, matches = set(), set()
    for i in range(len(bufs)):
        s = comp[int(co[i]):int(co[i + 1])].tobytes()
        for q in ref.sequences(s[ref.read_varint32(s)[1]:]):
            lits.add(q[0])
            if q[1] is not None:
                matches.add(q[2] - 4)
    print(f"\nliteral lengths near t: {sorted(x for x in lits if any(abs(x - t) <= 2 for t in EXT_T))}")
    print(f"match lengths - 4 near t: {sorted(x for x in matches if any(abs(x - t) <= 2 for t in EXT_T))}")
    for t in EXT_T:
        for v in (t - 1, t, t + 1):
            assert v in lits, f"no literal run of {v} bytes (t = {t})"
            assert v in matches, f"no match of {v} + 4 bytes (t = {t})"


def test_periodic_inputs_across_chunks(engine):
    """200000 bytes of period P: matches inside a 64 KiB chunk, across chunk starts, and at
    distances of exactly 65535 (the farthest offset) and 65536 (none).  Every block is valid and
    round-trips on the GPU; for P <= 60000 the repeat lies inside one chunk and must be found.
    (It was not for P = 60000 while the finder kept only each hash's latest position: 200789
    bytes.  With the table of first positions, DESIGN.md §10: 60797.)"""
    periods = (4000, 60000, 65535, 65536, 70000)
    bufs = [(lz4_streams._lits(P, P) * (200000 // P + 1))[:200000] for P in periods]
    data, offs = pack(bufs)
    comp, co = engine.lz4_compress_host(data, offs)
    check_compressed(bufs, comp, co, "periodic")
    out, oo, st = engine.lz4_decompress_host(comp, co, int(offs[-1]))
    assert (st == 0).all() and np.array_equal(oo, offs) and out.tobytes() == b"".join(bufs)
    sizes = {P: int(co[i + 1] - co[i]) for i, P in enumerate(periods)}
    print(f"\nperiodic inputs of 200000 bytes, compressed sizes by period: {sizes}")
    for P in periods:
        if P <= 60000:
            assert sizes[P] < 200000, sizes


# ---- a caller's stream, graph replay ---------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snappy")
N_BLOCKS = 500


def _graph_batch(seed):
    """N_BLOCKS blocks of 0..16384 bytes: text, random bytes, zeros, a short period."""
    rng = np.random.default_rng(seed)
    text = open(os.path.join(GOLDEN, "alice29.txt" if seed & 1 else "html"), "rb").read()
    bufs = []
    for i in range(N_BLOCKS):
        n = int(rng.integers(0, 200)) if i % 7 == 0 else 16384 if i % 11 == 0 else int(rng.integers(200, 16385))
        kind = i % 4
        if kind == 0:
            at = int(rng.integers(0, len(text) - n))
            bufs.append(text[at:at + n])
        elif kind == 1:
            bufs.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif kind == 2:
            bufs.append(bytes(n))
        else:
            bufs.append((rng.integers(0, 256, 1 + i % 50, dtype=np.uint8).tobytes() * (n + 1))[:n])
    return bufs


def _rejects(codec):
    """Small rejected streams of the codec with the reference's status, every status among them."""
    if codec == "lz4":
        got = [(s, st) for _, s, st, _, _ in lz4_streams.hand_built() if st != ref.OK and len(s) < 100]
    else:
        import snappy_streams as ss
        got = [(c.stream, c.status) for c in ss.family_batch() if c.status != 0 and len(c.stream) < 400]
    assert {st for _, st in got} >= {2, 3, 4, 5}
    return got


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_side_stream_and_graph_replay(codec):
    """compress -> decompress on one non-default stream with nothing between them, then the same two
    calls captured in a graph (one stream, the launches in a line) and replayed over canaries, and
    over a second batch copied into the same buffers; and a graph of the decompression alone whose
    second batch carries rejected streams.  The first kernels of each call zero the scans'
    look-back words, so every replay must give what a first call gives: compressed bytes equal to
    the host entry point's (LZ4: its determinism promise; they decode under the reference) or to
    the CPU oracle's (snappy), blocks equal to the inputs, statuses equal to the reference's."""
    from oracle import cpu
    eng = rr.Engine(0)
    try:
        n = N_BLOCKS
        comp_dev = getattr(eng, f"{codec}_compress_device")
        dec_dev = getattr(eng, f"{codec}_decompress_device")
        comp_host = getattr(eng, f"{codec}_compress_host")
        batches = [_graph_batch(7), _graph_batch(8)]
        packed = [pack(b) for b in batches]
        zs = [comp_host(d, o) for d, o in packed]                  # (compressed bytes, offsets)
        for bufs, (z, zo) in zip(batches, zs):
            for i in range(0, n, 1 if codec == "snappy" else 5):   # (LZ4 under the Python reference: every 5th)
                s = z[int(zo[i]):int(zo[i + 1])].tobytes()
                if codec == "snappy":
                    assert s == cpu.snappy_compress(bufs[i]), i
                else:
                    assert ref.decode(s) == (ref.OK, bufs[i], None), i
        # the decompression's own second batch: every 5th stream replaced by a rejected one
        rej = _rejects(codec)
        streams2 = [zs[1][0][int(zs[1][1][i]):int(zs[1][1][i + 1])].tobytes() for i in range(n)]
        want2 = [(0, b) for b in batches[1]]
        for k, i in enumerate(range(3, n, 5)):
            streams2[i] = rej[k % len(rej)][0]
            want2[i] = (rej[k % len(rej)][1], None)
        length = (lambda s: announced(s)) if codec == "lz4" else (lambda s: cpu.snappy_length(s)[1])
        dz2 = pack(streams2)
        oo2 = np.zeros(n + 1, np.uint64)
        oo2[1:] = np.cumsum([length(s) for s in streams2])

        nb = max(d.size for d, _ in packed)
        bound = getattr(eng._L, f"rr_{codec}_compress_bound")
        zcap = int(bound(n, nb))
        room = 256
        back = nb + 65536                                          # (rejected streams announce lengths of their own)
        assert int(oo2[-1]) <= back
        dev = torch.device("cuda:0")
        d_data = torch.zeros(nb, dtype=torch.uint8, device=dev)
        d_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_z = torch.zeros(zcap + room, dtype=torch.uint8, device=dev)
        d_zo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_back = torch.zeros(back + room, dtype=torch.uint8, device=dev)
        d_bo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
        d_in2 = torch.zeros(max(zs[0][0].size, dz2[0].size) + 15 & ~15, dtype=torch.uint8, device=dev)   # decompression alone
        d_io2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)

        def load(k):
            d, o = packed[k]
            d_data.zero_()
            d_data[:d.size].copy_(torch.from_numpy(d))
            d_offs.copy_(torch.from_numpy(o.view(np.int64)))

        def load2(data, offs):
            d_in2.zero_()
            d_in2[:min(data.size, int(offs[-1]))].copy_(torch.from_numpy(data[:int(offs[-1])]))
            d_io2.copy_(torch.from_numpy(offs.view(np.int64)))

        def canaries():
            for t in (d_z, d_back, d_st):
                t.fill_(SENTINEL)
            d_zo.fill_(7)
            d_bo.fill_(7)

        def chain(stream):
            comp_dev(d_data, d_offs, d_z[:zcap], d_zo, stream=stream)
            dec_dev(d_z[:zcap], d_zo, d_back[:back], d_bo, d_st[:n], stream=stream)

        def alone(stream):
            dec_dev(d_in2, d_io2, d_back[:back], d_bo, d_st[:n], stream=stream)

        def verify_back(want, offs, what):
            st, bo, back = d_st.cpu().numpy(), d_bo.cpu().numpy().view(np.uint64), d_back.cpu().numpy()
            assert np.array_equal(bo, offs), what
            assert [int(x) for x in st[:n]] == [w[0] for w in want], what
            assert (st[n:] == SENTINEL).all(), what
            for i, (wst, wout) in enumerate(want):
                if wst == 0:
                    assert back[int(bo[i]):int(bo[i + 1])].tobytes() == wout, (what, i)
            assert (back[int(bo[-1]):] == SENTINEL).all(), what

        def verify_chain(k, what):
            z, zo = zs[k]
            got, gzo = d_z.cpu().numpy(), d_zo.cpu().numpy().view(np.uint64)
            assert np.array_equal(gzo, zo), what
            assert np.array_equal(got[:int(zo[-1])], z), f"{what}: first at byte {first_diff(got[:int(zo[-1])].tobytes(), z.tobytes())}"
            assert (got[int(zo[-1]):] == SENTINEL).all(), what
            verify_back([(0, b) for b in batches[k]], packed[k][1], what)

        load(0)
        load2(*zs[0])
        chain(None)                                              # the context's scratch grows here, not under capture
        alone(None)
        torch.cuda.synchronize()
        canaries()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain(s)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        verify_chain(0, "side stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            chain(torch.cuda.current_stream())
        for r in range(3):
            canaries()
            g.replay()
            torch.cuda.synchronize()
            verify_chain(0, f"replay {r}")
        load(1)
        for r in range(2):
            canaries()
            g.replay()
            torch.cuda.synchronize()
            verify_chain(1, f"second batch, replay {r}")
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2):
            alone(torch.cuda.current_stream())
        for r in range(3):
            canaries()
            g2.replay()
            torch.cuda.synchronize()
            verify_back([(0, b) for b in batches[0]], packed[0][1], f"decompression alone, replay {r}")
        load2(*dz2)
        for r in range(2):
            canaries()
            g2.replay()
            torch.cuda.synchronize()
            verify_back(want2, oo2, f"decompression alone, rejected streams, replay {r}")
    finally:
        eng.close()
