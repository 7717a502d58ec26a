"""CPU tests of include/rr_aof.h: the restatement (tests/aof_reference.py) against a hand-written
fixture and against an independent replay, the host score-text function against float(), the bound,
the SELECT line, and the stand-alone C check built with the address and undefined-behaviour
sanitizers.  No GPU is touched."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import redrock_old_amd as rr
from oracle import cpu

import aof_reference as ar
from aof_shapes import HALFWAY, REFUSED                   # the two lists, shared with the device's shapes
import rdb_reference as ref
import rdbzset_reference as zr
from helpers import batch_from_blobs, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "aof")


def flat_of(blobs):
    data, offs = batch_from_blobs(blobs)
    return cpu.decode(data, offs)[:3]


def test_abi_exports():
    lib = rr.lib()
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_aof.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert syms == sorted(rr.AOF_EXPORTS)
    for s in syms:
        assert hasattr(lib, s), s


def test_restatement_against_fixture():
    """One value per type and encoding, two of them with an expiry: the .resp files are typed by hand."""
    fx = json.load(open(os.path.join(FIX, "values.json")))
    assert {f["name"] for f in fx} == {"string_raw", "string_int", "string_embstr", "list_quicklist", "set_intset", "set_ht",
                                       "hash_ht", "zset_skiplist", "hash_ziplist", "zset_ziplist"}
    values, elems, arena = flat_of([bytes.fromhex(f["blob"]) for f in fx])
    assert (values["status"] == 0).all()
    kd, ko = ar.keys_of([f["key"].encode() for f in fx])
    exp = np.array([f["expire"] for f in fx], np.int64)
    data, offs, status, totals, slices = ar.aof_batch(values, elems, arena, kd, ko, exp)
    assert (status == 0).all() and totals["n_bad"] == 0
    for f, s in zip(fx, slices):
        want = open(os.path.join(FIX, f["name"] + ".resp"), "rb").read()
        assert s == want, f["name"]
    assert bytes(data) == b"".join(slices) and int(offs[-1]) == len(data)
    assert len(data) <= rr.aof_bound(len(values), len(elems), int(elems["len"].sum()), len(kd))


def test_replay_equals_the_oracles_objects():
    """A minimal RESP parser applies the restatement's commands to a Python model; the model equals the
    oracle's decode of the same blobs, for every golden blob."""
    g = golden()
    blobs = [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]
    values, elems, arena = flat_of(blobs)
    names = [b"key:%d" % i for i in range(len(blobs))]
    kd, ko = ar.keys_of(names)
    exp = np.array([-1 if i % 3 else 1600000000000 + i for i in range(len(blobs))], np.int64)
    data, offs, status, totals, slices = ar.aof_batch(values, elems, arena, kd, ko, exp)
    assert set(status.tolist()) <= {ar.OK, ar.E_ENCODE} and (status == 0).sum() >= 40
    assert ((status == ar.E_ENCODE) == (values["status"] != 0)).all()
    db, expd = ar.replay(data)
    ab = arena.tobytes()
    seen = 0
    for i, (val, descs) in enumerate(ref.flat_values(values, elems, arena)):
        if status[i]:
            assert names[i] not in db and names[i] not in expd
            continue
        assert db.get(names[i]) == ar.model(val, descs, ab), i
        assert expd.get(names[i], -1) == int(exp[i])
        seen += 1
    assert seen == int((status == 0).sum()) and len(db) <= seen


def g17(t):
    return ("%.17g" % float(t)).encode()


def test_score_text_prints_every_d2string_text():
    """The floor: every text rr_d2string can produce is taken and prints itself; and rioWriteBulkDouble's
    %.17g is d2string's text for every non-NaN double, the integer shortcut included."""
    n = 0
    for bits in zr.edge_scores().tolist():
        t = zr.d2string(bits)
        if t == b"nan":
            assert rr.aof_score_text(t) is None
            continue
        assert t == g17(zr.to_double(bits)) == zr.libc_g17(zr.to_double(bits)), t
        assert rr.aof_score_text(t) == t and ar.score_text(t) == t, t
        n += 1
    assert n > 8000
    for v in (2.0**52 - 1, -(2.0**52 - 1), 2.0**52 - 2, 1.0, -1.0, 4503599627370494.0, 123456789012345.0):   # the shortcut's range
        assert zr.d2string(zr.to_bits(v)) == g17(v)


def test_score_text_random_mantissas():
    rng = random.Random(20240)
    for _ in range(100000):
        nd = rng.randint(1, 17)
        m = rng.randint(10 ** (nd - 1), 10 ** nd - 1)
        e = rng.randint(-345, 310)
        form = rng.randint(0, 3)
        if form == 0:
            t = "%de%d" % (m, e)
        elif form == 1:
            s = str(m)
            t = "%s.%sE%+d" % (s[0], s[1:], e)
        elif form == 2:
            t = "-.%de%d" % (m, e)
        else:
            t = "%d.e%d" % (m, e)
        assert rr.aof_score_text(t.encode()) == g17(t), t


@pytest.mark.parametrize("t", HALFWAY)
def test_score_text_halfway_and_forms(t):
    assert rr.aof_score_text(t.encode()) == g17(t) == ar.score_text(t.encode())


@pytest.mark.parametrize("t", REFUSED)
def test_score_text_refused(t):
    assert rr.aof_score_text(t.encode()) is None and ar.score_text(t.encode()) is None


def test_integer_entries_round_to_even():
    """What the restatement prints for a ziplist's integer score entries (the GPU test holds the kernel to
    it): (double) v rounds to nearest, ties to even."""
    for v, want in ((2**53 + 1, b"9007199254740992"), (2**63 - 1, b"9.2233720368547758e+18"), (-2**63, b"-9.2233720368547758e+18"),
                    (2**53 + 3, b"9007199254740996")):
        assert g17(v) == want == zr.libc_g17(float(v))
    assert rr.aof_score_text(b"9007199254740993") == b"9007199254740992"


def test_select_line():
    for dbi in (0, 9, 10, 15, 2**31 - 1):
        assert rr.aof_select(dbi) == b"*2\r\n$6\r\nSELECT\r\n" + ar.bulk_longlong(dbi)
    buf = np.zeros(8, np.uint8)
    assert rr.lib().rr_aof_select(buf.ctypes.data, 8, 0) == 0 and not buf.any()


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/aof_host_check.c: its own main over the same parser, built with ASan and UBSan, run alone."""
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = tmp_path / "aof_host_check"
    subprocess.run([cc, "-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "redrock_old_amd", "csrc"),
                    os.path.join(ROOT, "tools", "aof_host_check.c"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout
