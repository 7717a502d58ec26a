"""CPU tests of the RDB value payload rule (include/rr_rdbsave.h) as tests/rdb_reference.py states
it: literals derived by hand from the reference's source lines, the save / load round trip over the
golden fixtures and a generated batch, and the new header's exports.  The GPU tests hold
rr_rdbsave_batch to this same statement (tests/test_gpu_rdbsave.py)."""
import os
import re
import struct
import subprocess

import numpy as np

import redrock_old_amd as rr

import rdb_reference as ref
from helpers import batch_from_blobs, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_save_len_literals():
    assert ref.save_len(0) == b"\x00"                        # rdb.c:151: len < 64, one byte
    assert ref.save_len(63) == b"\x3F"
    assert ref.save_len(64) == b"\x40\x40"                   # :156: 01|len>>8, len&0xFF
    assert ref.save_len(16383) == b"\x7F\xFF"
    assert ref.save_len(16384) == b"\x80\x00\x00\x40\x00"    # :162: 0x80 then htonl(len)


def test_raw_string_integer_rule_literals():
    s = ref.save_raw_string
    assert s(b"0") == b"\xC0\x00"                            # rdb.c:242: INT8
    assert s(b"-0") == b"\x02-0"                             # ll2string(0) is "0": lengths differ, :318
    assert s(b"127") == b"\xC0\x7F"
    assert s(b"128") == b"\xC1\x80\x00"                      # :246: INT16, little-endian
    assert s(b"-128") == b"\xC0\x80"
    assert s(b"-129") == b"\xC1\x7F\xFF"
    assert s(b"32767") == b"\xC1\xFF\x7F"
    assert s(b"32768") == b"\xC2\x00\x80\x00\x00"            # :251: INT32
    assert s(b"2147483647") == b"\xC2\xFF\xFF\xFF\x7F"
    assert s(b"2147483648") == b"\x0A2147483648"             # outside int32: rdbEncodeInteger returns 0, :259
    assert s(b"-2147483648") == b"\xC2\x00\x00\x00\x80"      # 11 characters: the last length tried, :416
    assert s(b"-2147483649") == b"\x0B-2147483649"
    assert s(b"01") == b"\x0201"                             # ll2string(1) is "1", :318
    assert s(b"+1") == b"\x02+1"
    assert s(b" 1") == b"\x02 1"                             # strtoll skips the space, ll2string does not print it
    assert s(b"1 ") == b"\x021 "                             # endptr[0] != 0, :313
    assert s(b"") == b"\x00"                                 # strlen("0") != 0, :318
    assert s(b"12\x00") == b"\x0312\x00"                     # strtoll stops at the NUL; strlen("12") != 3
    assert s(b"123456789012") == b"\x0C123456789012"         # 12 characters: not tried, :416


def test_int_string_literals():
    f = ref.save_longlong
    assert f(2147483647) == b"\xC2\xFF\xFF\xFF\x7F"          # rdb.c:447-449
    assert f(-2147483648) == b"\xC2\x00\x00\x00\x80"
    assert f(2147483648) == b"\x0A2147483648"                # :452-456: rdbSaveLen(digits) + text
    assert f(-2147483649) == b"\x0B-2147483649"
    assert f(2**63 - 1) == b"\x139223372036854775807"
    assert f(-2**63) == b"\x14-9223372036854775808"


def test_score_literals():
    arena = b"a"
    val = {"type": rr.T_ZSET_SKIPLIST, "enc": 0}
    for x, bits in ((-0.0, b"\x00\x00\x00\x00\x00\x00\x00\x80"), (float("inf"), b"\x00\x00\x00\x00\x00\x00\xF0\x7F")):
        d = struct.unpack("<Q", struct.pack("<d", x))[0]
        # rdbSaveLen(1) | rdbSaveRawString("a") | the double's 8 bytes little-endian (rdb.c:605-608)
        assert ref.save(val, [(rr.K_STR, 0, 1), (rr.K_SCORE, d, 0)], arena) == b"\x01\x01a" + bits


def test_two_entry_list_node_byte_by_byte():
    arena = b"hello"
    val = {"type": rr.T_LIST_QUICKLIST, "enc": 0}
    got = ref.save(val, [(rr.K_STR, 0, 5), (rr.K_INT, 1024, 0)], arena)
    zl = (b"\x16\x00\x00\x00"      # zlbytes 22 = 10 header + 7 + 4 + 1 end
          b"\x11\x00\x00\x00"      # zltail 17: the second entry's offset
          b"\x02\x00"              # zllen 2
          b"\x00\x05hello"         # prevlen 0 | ZIP_STR_06B 5 | bytes   (ziplist.c:338-340)
          b"\x07\xC0\x00\x04"      # prevlen 7 | ZIP_INT_16B | 1024 LE   (ziplist.c:491, :513-516)
          b"\xFF")
    # rdbSaveLen(1 node) | rdbSaveRawString(node): 22 < 64, one length byte (rdb.c:774, :784)
    assert got == b"\x01" + b"\x16" + zl
    assert ref.load(rr.T_LIST_QUICKLIST, got) == ("list", [b"hello", b"1024"])


def test_node_split_at_the_limit():
    """fill -2: an entry joins while node->sz + sz + overhead <= 8192 (quicklist.c:441-442)."""
    # a node of one 200-byte entry is 11 + 1 + 2 + 200 = 214 bytes; a pushed string of sz in [254, 16384)
    # is estimated at sz + 5 + 2 (:427-438), so sz 7971 gives new_sz 8192 and joins, 7972 gives 8193
    counts = lambda strings, fill: [struct.unpack("<H", z[8:10])[0] for z in ref.list_nodes(strings, fill)]
    assert counts([b"x" * 200, b"y" * 7971], -2) == [2]
    assert counts([b"x" * 200, b"y" * 7972], -2) == [1, 1]
    # the estimate is not the real size: after an 8000-byte entry (node 8014) sz 173 is estimated at
    # 173 + 1 + 2 -> 8190 and joins, but its prevlen takes 5 bytes (ziplist.c:410): the node is 8194
    # and even an empty string (8194 + 0 + 1 + 1) no longer fits
    strings = [b"x" * 8000, b"y" * 173, b"", b""]
    assert counts(strings, -2) == [2, 2]
    assert len(ref.list_nodes(strings, -2)[0]) == 8194
    assert counts(strings, 0) == [1, 1, 1, 1]              # count < 0 never holds, :446
    assert counts(strings, 3) == [2, 2]                    # the 8192 safety limit still splits, :444
    assert counts([b"a"] * 7, 3) == [3, 3, 1]
    assert counts([b"a"] * 7, -9) == counts([b"a"] * 7, -5) == [7]   # quicklistSetFill's clamp, :120


def _flat_of(blobs, flags=0):
    data, offs = batch_from_blobs(blobs)
    return rr.host_decode_ex(data, offs, flags)[:3]


def _roundtrip(values, elems, arena, fill=-2):
    ab = arena.tobytes()
    seen = set()
    for (val, descs), r in zip(ref.flat_values(values, elems, arena), values):
        if not ref.accepted_value(val, descs, len(arena)):
            continue
        used = descs[:1] if val["type"] in (rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST) else descs
        pay = ref.save(val, used, ab, fill)
        assert ref.load(val["type"], pay) == ref.model(val, used, ab)
        seen.add(val["type"])
    return seen


def test_roundtrip_golden_fixtures():
    g = golden()
    blobs = [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]
    seen = _roundtrip(*_flat_of(blobs))
    assert len(seen) == 8
    _roundtrip(*_flat_of(blobs, rr.CTX_ZL_RAW))
    for fill in (-1, 0, 1, 3):
        _roundtrip(*_flat_of(blobs), fill=fill)


def test_roundtrip_generated_batch():
    data, offs = rr.gen_batch(4, 2000)
    values, elems, arena, _ = rr.host_decode(data, offs)
    assert len(_roundtrip(values, elems, arena)) >= 6


def test_bound_holds_for_reference_output():
    data, offs = rr.gen_batch(4, 2000)
    values, elems, arena, _ = rr.host_decode(data, offs)
    for fill in (-2, 0):
        total = int(ref.save_batch(values, elems, arena, fill)[2][-1])
        assert total <= rr.rdbsave_bound(values, elems)


def test_tiled_expectation_equals_reference_on_tiled_records():
    """The shortcut of tests/test_gpu_rdbsave_scale.py (flat_forge.tile_expect: the reference once on
    a 61-value base, its payloads repeated) against save_batch on the repeated records themselves:
    three whole tiles, a cut last tile, and a data_cap in the middle of a value of the third tile."""
    import flat_forge as ff
    values, elems, arena = ff.tiling_base()
    base_ref, pays = ff.tiling_reference(values, elems, arena)
    assert len(values) == ff.TILE_BASE and len(set(values["type"].tolist())) == 8
    assert int(base_ref[2][-1]) <= 40 * ff.TILE_BASE          # short payloads: the big batches stay cheap
    st = base_ref[3]
    assert values["status"][3] != 0 and st[3] == rr.E_ENCODE and (np.delete(st, 3) == 0).all()
    nodes = lambda i: base_ref[5][i][0]                       # rdbSaveLen(node count), one byte here
    assert nodes(0) == 2 and base_ref[5][2] == b"\x01\x0d" + ref.list_nodes([b"5"], ff.TILE_FILL)[0]
    assert len(ref.list_nodes([b"5"], ff.TILE_FILL)[0]) == 13 and base_ref[5][1] == b"\xC1\x39\x30"
    sizes = np.diff(base_ref[2].astype(np.int64))
    for n, cut_at in ((3 * ff.TILE_BASE, None), (2 * ff.TILE_BASE + 22, None), (3 * ff.TILE_BASE, 2 * ff.TILE_BASE + 5)):
        tv = ff.tile_records(values, n)
        cap = None
        if cut_at is not None:
            assert sizes[cut_at % ff.TILE_BASE] > 1
            full = ff.tile_expect(values, base_ref, pays, n)[2]
            cap = (int(full[cut_at]) + int(full[cut_at + 1])) // 2
        want = ref.save_batch(tv, elems, arena, ff.TILE_FILL, cap)
        types, data, offsets, status, totals = ff.tile_expect(values, base_ref, pays, n, cap)
        assert np.array_equal(types, want[0]) and np.array_equal(offsets, want[2])
        assert np.array_equal(status, want[3]) and totals == want[4]
        if cap is None:
            assert np.array_equal(data, want[1])
        else:
            j = int(np.nonzero(status == rr.E_CAPACITY)[0][0])
            assert j == cut_at and (status[j:] != 0).all() and (status[:j] == np.tile(st, 3)[:j]).all()
            # save_batch leaves unwritten bytes zero; nothing is written from offsets[j] on
            assert np.array_equal(data[:int(offsets[j])], want[1][:int(offsets[j])])
            assert not want[1][int(offsets[j]):].any()


def test_library_exports_every_rdbsave_symbol():
    """include/rr_rdbsave.h: every declared function is named rr_rdbsave_*, exported and listed."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_rdbsave.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert len(syms) == 5 and all(s.startswith("rr_rdbsave_") for s in syms)
    lib = rr.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_rdbsave.h but not exported"
    assert sorted(rr.RDBSAVE_EXPORTS) == syms
    assert lib.rr_rdbsave_bound(3, 5, 100) == (17 * 3 + 26 * 5 + 100 + 15) & ~15


def test_rdbsave_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_rdbsave.h"\n#include "rr_rdb.h"\n'
                   'int main(void){ rr_rdbsave_opts o = {RR_RDBSAVE_DEFAULT_FILL, 0};\n'
                   '  return (RR_RDB_SAVE_TAG != RR_RDB_FLAT_TAG && RR_RDB_SAVE_TAG < 0 && o.list_fill == -2) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
