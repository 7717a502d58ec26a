"""The streams of tests/lz4_window_streams.py against the Python statement of the acceptance rule
(tests/lz4_reference.py) and against the path each is meant to take in the GPU decompressor
(route(): lz4_dec_kernel's entry and bail-out conditions restated), before any GPU sees them, with
the coverage conditions tests/test_gpu_lz4_window.py relies on: the bail family's cells, the copy
matrix's (regime, source & 3, destination & 3) triples, the fuzz's acceptance share and status
counts.

Beside LdsMem::literals: its `op > D + p` can not be true (lz4_window_streams' docstring gives the
induction: every match that stays leaves op + len <= D + next, and a run starts past next), so
route() has no 'bail-literal' stream and none is tested; the kernel's check stays as it is."""
import collections
import os
import re

import numpy as np
import pytest

import lz4_reference as ref
import lz4_streams
import lz4_window_streams as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"bail": ws.family_bail, "matrix": ws.family_matrix, "fuzz_valid": ws.fuzz_valid}


def test_window_constant():
    """route() and every fixture assume the default window: a change of it must move them."""
    src = open(os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_lz4.hip")).read()
    assert int(re.search(r"^#define RR_LZ4_DEC_WIN (\d+)$", src, re.M).group(1)) == ws.W
    assert ws.WINDOWS[-1] == ws.W and all(w % 16 == 0 and 1024 <= w <= ws.W for w in ws.WINDOWS)
    assert re.search(r"dim3\(WAVE\), LZ4_DEC_WIN \+ 48, stream, .*\n.* status, dec_window\(\)\);", src)   # wcap = the window
    assert (ws.OK, ws.HEADER, ws.TRUNC, ws.OFFSET, ws.OVERFLOW, ws.LENGTH, ws.CAPACITY) == (
        ref.OK, ref.E_HEADER, ref.E_TRUNC, ref.E_OFFSET, ref.E_OVERFLOW, ref.E_LENGTH, ref.E_CAPACITY)


def test_fillers_and_pack_at():
    assert ref.decode(ws.FILL_OK) == (ref.OK, b"", None) and ref.decode(ws.FILL_TRUNC)[0] == ref.E_TRUNC
    streams = [b"\x01\x10a", b"\x01\x10b", b"\x01\x10c", b"\x00\x00", b"\x01\x10d"]
    data, offs, real = ws.pack_at(streams, [3, 0, 15, 2, 4])
    assert [int(offs[r]) & 15 for r in real] == [3, 0, 15, 2, 4]
    assert [data[int(offs[r]):int(offs[r + 1])].tobytes() for r in real] == streams
    assert data.size % 16 == 0 and int(offs[-1]) <= data.size
    for i in set(range(len(offs) - 1)) - set(int(r) for r in real):
        assert data[int(offs[i]):int(offs[i + 1])].tobytes() in (ws.FILL_OK, ws.FILL_TRUNC)


def test_builder_expands_like_lz4_streams_block():
    """Seqs' periodic expansion against lz4_streams.Block's byte-at-a-time one."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, b = ws.Seqs(), lz4_streams.Block()
        for _ in range(int(rng.integers(1, 8))):
            lits = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            off = int(rng.integers(1, len(a.out) + len(lits) + 1))
            ml = int(rng.integers(4, 600))
            a.seq(lits, off, ml)
            b.seq(lits, off, ml)
        a.seq(b"the-last-run")
        b.seq(b"the-last-run")
        assert a.stream() == b.stream() and a.out == b.out
        assert ref.decode(a.stream()) == (ref.OK, bytes(a.out), None)


def test_hand_built_streams_walk_like_the_reference():
    """walk() restates lz4_walk: the verdicts of the suite's hand-built streams."""
    for name, s, status, out, dev in lz4_streams.hand_built():
        for s0 in range(4):
            assert ws.walk(s, s0).status == status, name


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_matches_reference_and_route(family):
    cases = FAMILIES[family]()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        st, out, _ = ref.decode(c.stream)
        assert st == c.status, (c.name, st)
        if st == ref.OK:
            assert out == c.expected, c.name
        k = ws.walk(c.stream, c.s0, c.w)
        assert k.status == st, (c.name, k.status)        # the restatement decodes like the reference
        assert k.route == c.route, (c.name, k.route)
        assert k.route != "bail-literal"
        assert ws.route(c.stream, c.s0, c.w) == k.route
        if st == ref.OK:
            assert k.ops == c.ops, c.name                # the builder's copies are the walk's
    print(f"\nroutes {family}: {dict(collections.Counter((c.w, c.route) for c in cases))} of {len(cases)}")


def test_bail_family_cells():
    cases = {c.name: c for c in ws.family_bail()}
    cells = collections.Counter()
    for c in cases.values():
        k = ws.walk(c.stream, c.s0, c.w)
        if c.kind == "eq":          # equality stays in the window
            assert k.route == "lds" and min(k.margins) == 0 and c.status == ref.OK, c.name
            cells[c.w, "lds-at-equality"] += 1
        if c.kind == "bail":        # one byte more leaves it
            assert k.route == "bail-match" and min(k.margins) == -1 and c.status == ref.OK, c.name
        if k.route == "bail-match":
            cells[c.w, "bail-match"] += 1
    for w in ws.WINDOWS:
        assert cells[w, "lds-at-equality"] >= 4 and cells[w, "bail-match"] >= 4, cells
        for s0 in range(4):
            tag = f"w{w}_s{s0}"
            for shape in ("first", "later"):
                eq, bail = cases[f"eq_{shape}_{tag}"], cases[f"bail_{shape}_{tag}"]
                assert eq.s0 & 3 == s0 and bail.s0 & 3 == s0
                assert len(bail.expected) == len(eq.expected) + 1 <= w      # the same plus one byte
                ke, kb = ws.walk(eq.stream, s0, w), ws.walk(bail.stream, s0, w)
                assert kb.event == (0 if shape == "first" else len(ws.PREFIX))
                assert ke.margins.index(0) == kb.event
            # (c): a few hundred bytes are in the window when the block leaves it
            kb = ws.walk(cases[f"bail_later_{tag}"].stream, s0, w)
            at = [e for e in kb.ops if e[0] == "match"][kb.event][1]
            assert 300 <= at <= 600
            # rejected after the bail point: the global path's verdict
            want = {"offset": ref.E_OFFSET, "overflow": ref.E_OVERFLOW, "trunc": ref.E_TRUNC}
            for name, status in want.items():
                k = ws.walk(cases[f"bail_then_{name}_{tag}"].stream, s0, w)
                assert k.route == "bail-match" and k.status == status and k.bad > k.event >= 0, (name, k[:5])
            # rejected before it: the LDS path's verdict (the same block with a good offset bails later)
            k = ws.walk(cases[f"offset_then_bail_{tag}"].stream, s0, w)
            assert k.route == "lds" and k.status == ref.E_OFFSET and 0 <= k.bad < kb.event
            assert len(cases[f"offset_then_bail_{tag}"].stream) == len(cases[f"bail_later_{tag}"].stream)
            # the entry test: N and the span at w - 16, w, w + 16
            for what in ("n", "span"):
                got = [cases[f"entry_{what}{dn:+d}_{tag}"] for dn in (-16, 0, 16)]
                assert [c.route for c in got] == ["lds", "lds", "global"]
                for c, dn in zip(got, (-16, 0, 16)):
                    n, span = ref.read_varint32(c.stream)[0], (s0 + len(c.stream) + 15) & ~15
                    assert (n if what == "n" else span) == w + dn
                    assert (span if what == "n" else n) <= w     # only the one side is past the window


@pytest.mark.parametrize("wrong", ["ge", "d+16", "d-16"])
def test_a_wrong_bail_condition_changes_a_route(wrong):
    """`>=` for `>` in the match test, or D off by 16 either way: at every (w, s0) at least one
    bail-family stream would take another path, so the GPU test runs a stream that shows it."""
    kw = {"ge": dict(ge=True), "d+16": dict(d_add=16), "d-16": dict(d_add=-16)}[wrong]
    moved = collections.Counter()
    for c in ws.family_bail():
        if ws.route(c.stream, c.s0, c.w, **kw) != ws.route(c.stream, c.s0, c.w):
            moved[c.w, c.s0 & 3] += 1
    for w in ws.WINDOWS:
        for s0 in range(4):
            assert moved[w, s0] >= 1, (wrong, w, s0, moved)


def test_matrix_is_complete():
    """Every (regime, source & 3, destination & 3) of lds_copy's three regimes and of the match's
    modulo rounds; every offset x length of the matrix at all four op & 3; every literal length at
    all sixteen alignment pairs as a middle and as a last run; offsets equal to the length, one
    around it, and equal to op."""
    cases = ws.family_matrix()
    assert len(cases) <= 3000 and max(len(c.expected) for c in cases) <= 12500
    triples = set()
    matches, lits = set(), set()
    for c in cases:
        triples |= ws.copy_triples(c)
        hl = len(ref.varint32(len(c.expected)))
        last = len(c.ops) - 1
        for i, e in enumerate(c.ops):
            if e[0] == "match":
                matches.add((e[2], e[3], e[1] & 3, e[2] == e[1]))
            else:
                lits.add((e[3], ((c.s0 & 3) + hl + e[1]) & 3, e[2] & 3, i == last))
    pairs = {(s, d) for s in range(4) for d in range(4)}
    for r in ws.REGIMES:
        assert {(s, d) for x, s, d in triples if x == r} == pairs, r
    for off in ws.MATCH_OFFS:
        for ln in ws.MATCH_LENS:
            for a in range(4):
                assert any((off, ln, a, z) in matches for z in (False, True)), (off, ln, a)
    for ln in ws.MATCH_LENS:
        for off in (ln - 1, ln, ln + 1):
            if off != 4101:
                assert any((off, ln, a, False) in matches for a in range(4)), (off, ln)
    assert sum(1 for m in matches if m[3]) >= 100            # off == op: from output byte 0
    for L in ws.LIT_LENS:
        for last in (False, True):
            want = pairs if L else set()                     # (an empty run copies nothing)
            assert {(s, d) for n, s, d, z in lits if n == L and z == last} >= want, (L, last)
            assert any(n == L and z == last for n, s, d, z in lits), (L, last)


def test_regime_boundaries():
    """regime() against lds_copy's own tests: len <= 64, and nd = (len - h) >> 2 > 256 for a
    second round of the dword loop."""
    assert ws.regime(("lit", 0, 0, 64)) == "byte" and ws.regime(("lit", 0, 0, 65)) == "dwords"
    for d in range(4):
        h = (4 - d) & 3
        for ln in range(1000, 1100):
            nd = (ln - h) >> 2
            assert ws.regime(("lit", 0, d, ln)) == ("rounds" if nd > 256 else "dwords")
    assert ws.regime(("match", 100, 70, 70)) == "dwords" and ws.regime(("match", 100, 69, 70)) == "modulo"
    assert ws.regime(("match", 100, 64, 64)) == "modulo" and ws.regime(("match", 2000, 1100, 1100)) == "rounds"


def test_fuzz_conditions():
    """Seed 1: 300 valid blocks, all accepted with the builder's bytes; 600 mutants of which the
    reference accepts 251 (41.8 %) and rejects 64 HEADER, 28 TRUNC, 172 OFFSET, 41 OVERFLOW, 44
    LENGTH; none announces more than 64 KiB.  Under window 4096, 199 of the valid blocks stay in the window and 101 go global."""
    valid = ws.fuzz_valid(1)
    assert len(valid) == ws.FUZZ_N
    mutated = ws.fuzz_mutated(1)
    assert len(mutated) == 2 * ws.FUZZ_N
    st = collections.Counter(ref.decode(s)[0] for s, _ in mutated)
    print(f"\nfuzz_mutated statuses {dict(st)}")
    assert 0.15 * len(mutated) <= st[ref.OK] <= 0.85 * len(mutated), st
    for code in (ref.OK, ref.E_HEADER, ref.E_TRUNC, ref.E_OFFSET, ref.E_OVERFLOW, ref.E_LENGTH):
        assert st[code] >= 5, st
    assert dict(st) == {ref.OK: 251, ref.E_HEADER: 64, ref.E_TRUNC: 28, ref.E_OFFSET: 172, ref.E_OVERFLOW: 41, ref.E_LENGTH: 44}
    for s, s0 in mutated:
        assert (ref.read_varint32(s) or (0,))[0] <= ws.MAX_ANNOUNCED
        for w in (ws.W, 4096):
            assert ws.walk(s, s0, w).status == ref.decode(s)[0]
    r = collections.Counter(ws.route(c.stream, c.s0, 4096) for c in valid)
    assert r["lds"] >= 100 and r["global"] >= 50, r
    assert max(len(c.expected) for c in valid) > ws.W - 1000


def test_random_valid_block_mixes_every_token_form():
    rng = np.random.default_rng(5)
    forms = collections.Counter()
    for _ in range(60):
        b = ws.random_valid_block(rng, int(rng.integers(13, ws.W + 1)))
        assert ref.decode(b.stream()) == (ref.OK, bytes(b.out), None)
        for e in b.ops:
            if e[0] == "lit":
                forms["L", (e[3] > 0) + (e[3] >= 15) + (e[3] > 15)] += 1      # 0, below, at, above 15
            else:
                m = e[3] - 4
                forms["M", (m >= 15) + (m > 15)] += 1
                forms["off", "short" if e[2] <= 8 else "start" if e[2] == e[1] else "far"] += 1
    for k in [("L", n) for n in range(4)] + [("M", n) for n in range(3)] + [("off", n) for n in ("short", "start", "far")]:
        assert forms[k] >= 20, forms
