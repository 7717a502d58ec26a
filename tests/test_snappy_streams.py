"""The streams of tests/snappy_streams.py against the CPU oracle and against the path each is
meant to take in the GPU decompressor (route(): the kernel's entry and bail-out conditions
restated), before any GPU sees them.  tests/test_gpu_snappy_window.py runs the same streams."""
import collections
import os
import re

import numpy as np
import pytest

import snappy_streams as ss
from oracle import cpu
from snappy_corpus import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {
    "bail": ss.family_bail, "batch": ss.family_batch, "spec": ss.family_spec,
    "matrix": ss.family_matrix, "matrix_front": lambda: ss.family_matrix(True), "fuzz_valid": ss.fuzz_valid,
}


def routes(cases):
    return collections.Counter(ss.walk(c.stream, c.s0).route for c in cases)


def test_window_constant():
    """route() and every fixture assume the default window: a change of it must move them."""
    src = open(os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_snappy.hip")).read()
    assert int(re.search(r"^#define RR_SNZ_DEC_WIN (\d+)$", src, re.M).group(1)) == ss.W
    assert int(re.search(r"^#define RR_SNZ_SPEC (\d+)$", src, re.M).group(1)) * 64 == ss.ROUND
    assert re.search(r"dim3\(WAVE\), SNZ_DEC_WIN \+ 48, stream, .*\n.* status, SNZ_DEC_WIN\);", src)   # wcap = the window


def test_fillers_are_empty_streams():
    for f in ss.FILL.values():
        assert cpu.snappy_uncompress(f) == (0, b"")
    data, offs, real = ss.pack_at([b"\x01\x00a", b"\x01\x00b", b"\x01\x00c", b"\x00"], [3, 0, 0, 2])
    assert [int(offs[r]) & 3 for r in real] == [3, 0, 0, 2]
    assert [data[int(offs[r]):int(offs[r + 1])].tobytes() for r in real] == [b"\x01\x00a", b"\x01\x00b", b"\x01\x00c", b"\x00"]
    assert len(offs) == 4 + 4 + 1 and data.size % 16 == 0


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_matches_oracle_and_route(family):
    cases = FAMILIES[family]()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        st, out = cpu.snappy_uncompress(c.stream)
        assert st == c.status, (c.name, st)
        if st == 0:
            assert out == c.expected, c.name
        k = ss.walk(c.stream, c.s0)
        assert k.status == st, (c.name, k)          # the restatement decodes like the oracle
        assert k.route == c.route, (c.name, k)
        assert ss.route(c.stream, c.s0) == (k.route, k.ntags)
    print(f"\nroutes {family}: {dict(routes(cases))} of {len(cases)}")


def test_bail_family_shapes():
    cases = {c.name: c for c in ss.family_bail()}
    got = routes(cases.values())
    assert got["bail-copy"] >= 8 and got["bail-literal"] >= 4 and got["lds"] >= 8
    s, out = ss.bail_copy_rle().finish()
    assert (len(out), len(s)) == (18429, 2236)       # the issue's example
    assert len(ss.bail_copy_far().finish()[1]) == ss.W
    names = list(cases)
    for s0 in range(4):
        for shape in ("rle", "far", "longlit"):
            c = cases[f"{shape}_s{s0}"]
            assert c.s0 == s0 and c.status == 0
            i = names.index(c.name)                   # an ordinary block on either side
            assert names[i - 1].startswith("plain") and names[i + 1].startswith("plain")
        c = cases[f"longlit_s{s0}"]
        k = ss.walk(c.stream, s0)
        assert len(c.expected) == ss.W and k.event == k.ntags - 1
        assert 9 <= (-(s0 + len(c.stream))) % 16      # the padding behind the block
        # rejected after the bail point: the verdict is the global path's
        for name in ("bail_then_offset_same_batch", "bail_then_offset_later", "bail_then_length"):
            k = ss.walk(cases[f"{name}_s{s0}"].stream, s0)
            assert k.route == "bail-copy" and k.status != 0 and (k.bad > k.event or k.status == ss.LENGTH), (name, k)
        k = ss.walk(cases[f"bail_then_offset_same_batch_s{s0}"].stream, s0)
        assert k.bad // ss.BATCH == k.event // ss.BATCH
        # rejected before it: the LDS path's verdict (the same stream without the bad tag bails later)
        good = ss.walk(cases[f"rle_s{s0}"].stream, s0)
        for name in ("offset_then_bail_same_batch", "offset_then_bail_earlier"):
            k = ss.walk(cases[f"{name}_s{s0}"].stream, s0)
            assert k.route == "lds" and k.status == ss.OFFSET and k.bad < good.event, (name, k)
        k = ss.walk(cases[f"offset_then_bail_same_batch_s{s0}"].stream, s0)
        assert k.bad // ss.BATCH == good.event // ss.BATCH


def test_batch_family_shapes():
    cases = {c.name: c for c in ss.family_batch()}
    for n in ss.NTAGS:
        for mix in ("lit", "copy", "alt"):
            c = cases[f"{mix}{n}"]
            assert ss.route(c.stream, c.s0) == ("lds", n)
    for name, c in cases.items():
        k = ss.walk(c.stream, c.s0)
        m = re.fullmatch(r"(\w+?)_at(\d+)", name)
        if m and not name.startswith("length"):
            assert k.bad == int(m.group(2)), (name, k)     # the rejected tag sits where the name says
        elif m:
            assert k.ntags == int(m.group(2)) + 1 and k.status == ss.LENGTH
        m = re.fullmatch(r"two_(\w+)@(\d+)_(\w+)@(\d+)", name)
        if m:
            assert k.bad == int(m.group(2)) and k.status == ss.BAD_KINDS[m.group(1)]
            assert ss.BAD_KINDS[m.group(1)] != ss.BAD_KINDS[m.group(3)]
        if name.startswith("b2_"):
            assert k.ntags > ss.BATCH and k.status == 0
    assert {int(re.search(r"at(\d+)$", n).group(1)) for n in cases if n.startswith("offset0_at")} == set(ss.BAD_AT)


def test_spec_family_positions():
    """The tag the name speaks of starts at that offset from the round's first position (the
    first tag: the byte after the preamble)."""
    for c in ss.family_spec():
        m = re.search(r"_at(\d+)_", c.name) or re.search(r"_at(\d+)$", c.name[:-3])
        m2 = re.match(r"(one_literal|tags_to)_(\d+)_s", c.name)
        want = int(m.group(1)) if m else int(m2.group(2))
        s, p = c.stream, 0
        while s[p] & 0x80:
            p += 1
        p += 1
        first, starts = p, []
        while p < len(s) and p - first <= 70:      # tag starts (the tags in front are valid)
            starts.append(p - first)
            t = s[p]
            if t & 3 == 0:
                n = (t >> 2) + 1
                nb = n - 60 if n >= 61 else 0
                n = int.from_bytes(s[p + 1:p + 1 + nb], "little") + 1 if nb else n
                p += 1 + nb + n
            else:
                p += (0, 2, 3, 5)[t & 3]
        assert want in starts, (c.name, starts)


def test_matrix_covers_both_copy_kinds_and_alignments():
    indep = ordered = 0
    seen = set()
    for c in ss.family_matrix():
        k = ss.walk(c.stream, c.s0)
        indep += k.indep
        ordered += k.ordered
    assert indep >= 1000 and ordered >= 1000
    # every (offset, length, destination alignment) of the matrix occurs
    for c in ss.family_matrix():
        s, p, pos = c.stream, 0, 0
        while s[p] & 0x80:
            p += 1
        p += 1
        while p < len(s):
            t = s[p]
            if t & 3 == 0:
                n = (t >> 2) + 1
                nb = n - 60 if n >= 61 else 0
                n = int.from_bytes(s[p + 1:p + 1 + nb], "little") + 1 if nb else n
                p += 1 + nb + n
            else:
                nb = (0, 1, 2, 4)[t & 3]
                x = int.from_bytes(s[p + 1:p + 1 + nb], "little")
                n, off = (4 + ((t >> 2) & 7), ((t >> 5) << 8) | x) if t & 3 == 1 else ((t >> 2) + 1, x)
                seen.add((off, n, pos & 3))
                p += 1 + nb
            pos += n
    for off in ss.OFFSETS + (2047, 2048):
        for n in ss.LENGTHS:
            for a in range(4):
                assert (off, n, a) in seen or off >= 2047, (off, n, a)
            assert any((off, n, a) in seen for a in range(4))


def test_fuzz_conditions():
    """What the GPU fuzz relies on: the valid streams decode and reach both the plain LDS path and
    the bail-out; the mutated round stays LDS-eligible and meets every status often enough."""
    valid = ss.fuzz_valid(1)
    assert len(valid) == ss.FUZZ_N
    r = routes(valid)
    assert r["global"] == 0 and r["lds"] >= 100 and r["bail-literal"] + r["bail-copy"] >= 10, r
    assert max(ss.walk(c.stream, c.s0).ntags for c in valid) > 3 * ss.BATCH
    assert max(len(c.expected) for c in valid) > ss.W - 1000
    mutated = ss.fuzz_mutated(1)
    assert len(mutated) == ss.FUZZ_N + 40 * len(ss.MUT_INPUTS)
    elig = sum(ss.walk(s, s0).route != "global" for s, s0 in mutated)
    assert elig >= 0.9 * len(mutated), elig
    st = collections.Counter(cpu.snappy_uncompress(s)[0] for s, _ in mutated)
    for code in (ss.TRUNC, ss.OFFSET, ss.OVERFLOW, ss.LENGTH):
        assert st[code] >= 5, st
    assert st[ss.OK] >= 20, st
    for s, s0 in mutated:
        assert ss.walk(s, s0).status == cpu.snappy_uncompress(s)[0]
    print(f"\nroutes fuzz_mutated: {dict(collections.Counter(ss.walk(s, s0).route for s, s0 in mutated))}, statuses {dict(st)}")


def test_random_valid_stream_mixes_every_tag_form():
    rng = np.random.default_rng(5)
    kinds = collections.Counter()
    for _ in range(40):
        s = ss.random_valid_stream(rng, int(rng.integers(1, ss.W + 1)))
        stream, out = s.finish()
        assert cpu.snappy_uncompress(stream) == (0, out) and len(out) <= ss.W and len(stream) <= ss.W - 32
        for t in s.tags:
            kinds[("lit", (t[0] >> 2) - 59 if (t[0] >> 2) >= 60 else 0) if t[0] & 3 == 0 else ("copy", t[0] & 3)] += 1
    for k in [("lit", n) for n in range(5)] + [("copy", n) for n in (1, 2, 3)]:
        assert kinds[k] >= 20, kinds


def test_grid_stride_tiny_block():
    """The million identical blocks of the grid-stride test: one byte <-> its 3-byte stream."""
    assert cpu.snappy_compress(b"a") == b"\x01\x00a"
    assert cpu.snappy_uncompress(b"\x01\x00a") == (0, b"a")
    assert len(corpus()["random_16k"]) == 16384
