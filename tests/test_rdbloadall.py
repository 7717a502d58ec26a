"""CPU tests of include/rr_rdbloadall.h: the selection rule of tests/rdbloadall_reference.py against hand-written
status and size triples for every row of the header's table, expected() against the per-stage references over the
load, convert and zset corpora, the workspace layout and the three bounds, the argument checks that return before
any HIP call, and the ABI.  The GPU side is tests/test_gpu_rdbloadall.py."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np

import redrock_old_amd as rr

import rdbconvert_reference as cv
import rdbload_mutants as mut
import rdbload_reference as ld
import rdbloadall_reference as la
import rdbzset_reference as zr
import test_rdbconvert as tc
import test_rdbload as tl
import test_rdbzset as tz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, CONV, SLICE = la.E_CAPACITY, la.E_CONVERT, la.E_SLICE
SKIP2, SKIP3 = cv.SKIP, zr.SKIP


def forged(rows):
    """rows: (s1, s2, s3, size1, size2, size3) -> three stage batches whose value i has these statuses and
    sizes, every stage's bytes its own (stage k's value i is bytes of (16 k + i) & 0xFF)."""
    n = len(rows)
    stages = []
    for k in range(3):
        sizes = [r[3 + k] for r in rows]
        offs = np.zeros(n + 1, np.uint64)
        np.cumsum(sizes, out=offs[1:])
        data = b"".join(bytes([(16 * (k + 1) + i) & 0xFF]) * s for i, s in enumerate(sizes))
        stages.append((np.frombuffer(data, np.uint8), offs, np.array([r[k] for r in rows], np.uint8), len(data)))
    return stages


# (s1, s2, s3, size1, size2, size3) -> (merged status, holding stage or 0, size); the bytes are written for status 0
RULE = [((0, SKIP2, SKIP3, 7, 0, 0), (0, 1, 7)),
        ((CAP, SKIP2, SKIP3, 9, 0, 0), (CAP, 1, 9)),
        ((CONV, 0, SKIP3, 0, 24, 0), (0, 2, 24)),
        ((CONV, CAP, SKIP3, 0, 30, 0), (CAP, 2, 30)),
        ((CONV, CONV, 0, 0, 0, 31), (0, 3, 31)),
        ((CONV, CONV, CAP, 0, 0, 33), (CAP, 3, 33)),
        ((CONV, CONV, CONV, 0, 0, 0), (CONV, 0, 0)),
        ((CONV, CONV, SKIP3, 0, 0, 0), (CONV, 0, 0)),
        ((CONV, SKIP2, 0, 0, 0, 5), (CONV, 0, 0)),             # anything else behind it: stage 3 is not looked at
        ((CONV, 99, 0, 0, 6, 5), (CONV, 0, 0)),
        ((ld.E_TRUNC, SKIP2, SKIP3, 0, 0, 0), (ld.E_TRUNC, 0, 0)),
        ((ld.E_TYPE, 0, 0, 0, 8, 8), (ld.E_TYPE, 0, 0)),       # any other s1 wins whatever is behind it
        ((200, CONV, 0, 3, 3, 3), (200, 0, 0)),
        # the inconsistent ones: only the statuses decide, the first holder wins
        ((0, 0, 0, 6, 8, 10), (0, 1, 6)),
        ((0, CONV, 0, 6, 0, 10), (0, 1, 6)),
        ((CAP, 0, 0, 6, 8, 10), (CAP, 1, 6)),
        ((CONV, 0, 0, 6, 8, 10), (0, 2, 8)),
        ((CONV, CAP, 0, 6, 8, 10), (CAP, 2, 8)),
        ((0, SKIP2, SKIP3, 0, 4, 4), (0, 1, 0))]               # a holder of size 0 holds nothing, and is no error


def test_rule_table():
    rows = [r for r, _ in RULE]
    stages = forged(rows)
    types = np.arange(len(rows), dtype=np.uint8) + 100
    conv_types = np.arange(len(rows), dtype=np.uint8) + 150
    data, offs, out_types, status, totals, blobs = la.merge(*stages, types, conv_types)
    at = 0
    for i, (row, (st, k, size)) in enumerate(RULE):
        assert la.select(*row[:3]) == (k, st), (i, row)
        assert (int(status[i]), int(offs[i]), int(offs[i + 1])) == (st, at, at + size), (i, row)
        want = bytes([(16 * k + i) & 0xFF]) * size if k and st == 0 else None
        assert blobs[i] == want, (i, row)
        assert int(out_types[i]) == ((100 + i, 150 + i, 12)[k - 1] if k else 0xFF), (i, row)
        assert data[at:at + size].tobytes() == (want or bytes(size))
        at += size
    written = [(k, size) for _, (st, k, size) in RULE if k and st == 0]
    assert totals == {"bytes": at, "n_bad": sum(st != 0 for _, (st, _, _) in RULE),
                      "payload": sum(s for _, s in written), "n_elems": sum(k >= 2 for k, _ in written)}
    assert len(written) == 7 and {st for _, (st, _, _) in RULE} >= {0, CAP, CONV, ld.E_TRUNC, ld.E_TYPE}


def test_slices_and_capacity():
    rows = [(0, SKIP2, SKIP3, 20, 0, 0), (CONV, 0, SKIP3, 0, 30, 0), (CONV, CONV, 0, 0, 0, 40), (0, SKIP2, SKIP3, 10, 0, 0)]
    s = forged(rows)
    types = conv = np.zeros(4, np.uint8)
    full = la.merge(*s, types, conv)
    assert full[3].tolist() == [0, 0, 0, 0] and full[1].tolist() == [0, 20, 50, 90, 100]
    # a reversed slice, and one past that batch's data_cap: RR_RDBMERGE_E_SLICE, size 0, the neighbours as they were
    o2 = s[1][1].copy()
    o2[1], o2[2] = 30, 0
    rev = la.merge(s[0], (s[1][0], o2, s[1][2], s[1][3]), s[2], types, conv)
    assert rev[3].tolist() == [0, SLICE, 0, 0] and rev[1].tolist() == [0, 20, 20, 60, 70] and rev[5][1] is None
    assert rev[5][0] == full[5][0] and rev[5][2] == full[5][2] and int(rev[2][1]) == 0xFF
    past = la.merge(s[0], s[1], (s[2][0], s[2][1], s[2][2], 39), types, conv)
    assert past[3].tolist() == [0, 0, SLICE, 0] and past[1].tolist() == [0, 20, 50, 50, 60]
    # a stage's RR_E_CAPACITY slice lies past its data_cap by construction: the size is kept
    capped = la.merge(s[0], (s[1][0][:0], s[1][1], np.array([SKIP2, CAP, CONV, SKIP2], np.uint8), 0), s[2], types, conv)
    assert capped[3].tolist() == [0, CAP, 0, 0] and capped[1].tolist() == full[1].tolist() and capped[4]["payload"] == 70
    # the merged capacity: a value that ends past data_cap, its size kept, nothing of it written
    for cap, want in ((100, [0, 0, 0, 0]), (99, [0, 0, 0, CAP]), (50, [0, 0, CAP, CAP]), (0, [CAP] * 4)):
        got = la.merge(*s, types, conv, cap)
        assert got[3].tolist() == want and got[1].tolist() == full[1].tolist() and len(got[0]) == min(cap, 100)
        assert got[4]["payload"] == sum(b is not None and len(b) for b in got[5]) and got[4]["n_bad"] == sum(w != 0 for w in want)


def corpora():
    """(types, payloads, options) groups: the load tests' corpus, the three CPU files' literals, the zset file's random values."""
    types, pays, _ = mut.corpus()
    groups = {}
    for t, p in zip(types, pays):
        groups.setdefault(tuple(sorted(mut.OPTS.items())), []).append((int(t), p))
    for cases in (tl.literal_cases(), tc.literal_cases()):
        for t, p, o, _, _ in cases:
            groups.setdefault(tuple(sorted((o or ld.DEFAULTS).items())), []).append((t, p))
    for p, o, _, _ in tz.literal_cases():
        groups.setdefault(tuple(sorted((o or ld.DEFAULTS).items())), []).append((rr.T_ZSET_SKIPLIST, p))
    for p in tz.random_zsets():                                 # the zset test's random values, fractional scores mostly
        groups[tuple(sorted(ld.DEFAULTS.items()))].append((rr.T_ZSET_SKIPLIST, p))
    return [([c[0] for c in v], [c[1] for c in v], dict(k)) for k, v in groups.items()]


def test_expected_against_the_stage_references():
    """Every value of the corpora: expected() holds the blob of the first stage whose own reference gives one."""
    seen = collections.Counter()
    for types, pays, opts in corpora():
        data, offs, out_types, status, totals, blobs, stage_bytes = la.expected(pays, types, opts)
        at = 0
        for i, (t, p) in enumerate(zip(types, pays)):
            s1, b1, _, _ = ld.load_blob(t, p, opts)
            want, wt, k = (b1, t, 1) if s1 == 0 else (None, 0xFF, 0)
            st = s1
            if s1 == ld.E_CONVERT:
                s2, t2, b2, _, _ = cv.convert_blob(t, p, opts)
                if s2 == 0:
                    want, wt, st, k = b2, t2, 0, 2
                elif t == rr.T_ZSET_SKIPLIST:
                    s3, b3, _, _ = zr.zset_blob(p, opts)
                    if s3 == 0:
                        want, wt, st, k = b3, rr.T_ZSET_ZIPLIST, 0, 3
            assert (int(status[i]), blobs[i], int(out_types[i])) == (st, want, wt), (i, t, p)
            size = len(want) if want is not None else 0
            assert int(offs[i]) == at and data[at:at + size].tobytes() == (want or b"")
            assert want is None or want[0] == wt
            at += size
            seen[k] += 1
        assert int(offs[-1]) == at == totals["bytes"] == totals["payload"] and sum(stage_bytes) == at
        assert totals["n_bad"] == int((status != 0).sum())
    assert seen[1] > 100 and seen[2] >= 50 and seen[3] >= 50 and seen[0] > 100, seen   # every stage holds, and nothing does


def test_expected_with_short_stages():
    """A stage that ran short: its RR_E_CAPACITY values keep their sizes in the merge, and the sizing run
    (every capacity 0) has the full run's offsets."""
    types, pays, opts = max(corpora(), key=lambda g: len(g[0]))
    full = la.expected(pays, types, opts)
    sizing = la.expected(pays, types, opts, stage_cap=(0, 0, 0), data_cap=0)
    assert np.array_equal(sizing[1], full[1]) and sizing[6] == full[6] and len(sizing[0]) == 0
    assert set(sizing[3][full[3] == 0].tolist()) == {CAP} and np.array_equal(sizing[3][full[3] != 0], full[3][full[3] != 0])
    assert np.array_equal(sizing[2], full[2])                                   # the types of values that are held
    short = la.expected(pays, types, opts, stage_cap=(full[6][0], full[6][1] - 1, full[6][2]))
    last2 = max(i for i, t in enumerate(types) if full[3][i] == 0 and ld.load_blob(t, pays[i], opts)[0] == ld.E_CONVERT
                and cv.convert_blob(t, pays[i], opts)[0] == 0)
    assert short[3][last2] == CAP and np.array_equal(np.delete(short[3], last2), np.delete(full[3], last2))
    assert np.array_equal(short[1], full[1])


def test_workspace_layout_and_caps():
    for n, pb in ((0, 0), (1, 1), (3, 100), (1000, 12345), (1 << 20, 1 << 29)):
        caps = rr.rdbloadall_caps(n, pb)
        assert caps == (rr.rdbload_bound(n, pb), rr.rdbconvert_bound(n, pb), rr.rdbzset_bound(n, pb))
        for sc in (caps, (0, 0, 0), (1, 17, 33), (16, 0, 15)):
            assert rr.rdbloadall_ws_bytes(n, sc) == la.ws_bytes(n, sc), (n, sc)
            assert rr.rdbloadall_ws_bytes(n, sc) % 16 == 0
    assert rr.rdbloadall_ws_bytes(5, (0, 0, 0)) == 144 + 96 + 32               # 3 x 6 offsets, 3 totals, 4 x 5 bytes
    assert rr.rdbloadall_ws_bytes(5, (1, 16, 17)) == 144 + 96 + 32 + 16 + 16 + 32


def test_argument_checks():
    """Bad options give RR_API_EINVAL before anything else is looked at, as for rr_rdbload_batch; then the NULL
    arguments.  All of it returns before any HIP call.  (The workspace checks need a context: the GPU file.)"""
    lib = rr.lib()
    offs = np.zeros(1, np.uint64)
    t = rr.Totals()
    ib, ob = rr.BlobBatch(), rr.BlobBatch()
    caps = (C.c_uint64 * 3)()

    def host(o):
        rc = lib.rr_rdbloadall_batch_host(None, None, rr._ptr(offs), None, 0, o, None, 0, rr._ptr(offs), None, None, None, C.byref(t))
        return rc, lib.rr_last_error().decode()

    def dev(o):
        rc = lib.rr_rdbloadall_batch(None, C.byref(ib), None, None, 0, caps, C.byref(ob), None, None, None, None, o, None)
        return rc, lib.rr_last_error().decode()

    for call in (host, dev):
        rc, msg = call(C.byref(rr.RdbLoadOpts(flags=1)))
        assert rc == rr.API_EINVAL and "flags" in msg
        rc, msg = call(C.byref(rr.RdbLoadOpts(zset_max_ziplist_entries=32768)))
        assert rc == rr.API_EINVAL and "32767" in msg
        rc, msg = call(None)
        assert rc == rr.API_EINVAL and "NULL" in msg                           # the options pass; the missing context is next
    b = [rr.BlobBatch() for _ in range(4)]
    for drop in range(4):                                                       # the primitive: a NULL batch, a NULL context
        a = [C.byref(x) if k != drop else None for k, x in enumerate(b)]
        rc = lib.rr_rdbmerge_batch(None, a[0], None, a[1], None, None, a[2], None, None, a[3], None, None, None, None)
        assert rc == rr.API_EINVAL and "NULL" in lib.rr_last_error().decode()


def test_library_exports_every_rdbloadall_symbol():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_rdbloadall.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert len(syms) == 5
    lib = rr.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_rdbloadall.h but not exported"
        assert getattr(lib, s).argtypes, f"{s} not bound"
    assert sorted(rr.RDBLOADALL_EXPORTS) == syms
    for name, py in (("RR_RDBMERGE_E_SLICE", rr.RDBMERGE_E_SLICE), ("RR_RDBMERGE_SPAN", rr.RDBMERGE_SPAN),
                     ("RR_RDBMERGE_MAX_WAVES", rr.RDBMERGE_MAX_WAVES)):
        assert int(re.search(rf"#define {name}\s+(\d+)", txt).group(1)) == py
    assert rr.RDBMERGE_E_SLICE == la.E_SLICE == 57 and rr.RDBMERGE_SPAN % 1024 == 0


def test_rdbloadall_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_rdbloadall.h"\n'
                   'int main(void){ uint64_t cap[3] = {0, 0, 0};\n'
                   '  return (RR_RDBMERGE_E_SLICE == 57 && RR_RDBMERGE_E_SLICE > RR_RDBZSET_SKIP && RR_RDBMERGE_SPAN % 1024 == 0\n'
                   '          && RR_RDBMERGE_MAX_WAVES % 4 == 0 && cap[2] == 0) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
