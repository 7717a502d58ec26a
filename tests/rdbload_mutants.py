"""A deterministic corpus of corrupt RDB value payloads for rr_rdbload_batch: a handful of small
valid seeds that between them reach every branch of the load rule (include/rr_rdbload.h), and every
single-byte substitution, strict prefix, appended byte and type swap of each.  Plain Python: no GPU
and no call into the library.  tests/test_rdbload_mutants.py checks the corpus itself;
tests/test_gpu_rdbload_edges.py sends it through the kernels.

  seeds()    [(type, payload)]
  corpus()   (types, payloads, origin): origin[i] = (seed index, kind, position)
  OPTS       thresholds under which some seeds load and some give RR_RDBLOAD_E_CONVERT
"""
import struct

import redrock_old_amd as rr

import lzf_reference as lzf
import rdb_reference as ref
import rdbload_reference as ld

S, L, SET, HASH, ZSET = rr.T_STRING, rr.T_LIST_QUICKLIST, rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST
ISET, HZL, ZZL = rr.T_SET_INTSET, rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST

OPTS = ld.options(set_max_intset_entries=2, hash_max_ziplist_entries=1, hash_max_ziplist_value=64,
                  zset_max_ziplist_entries=1, zset_max_ziplist_value=64)

# the values every byte position is replaced by: the borders of the length forms (rdb.c:196-219), of
# the string encodings (:500-512), of the LZF control byte (lzf_d.c:72, :119) and of the ziplist
# entry classes (ziplist.c:332-364, :507-534)
SUBST = (0x00, 0x01, 0x0A, 0x0B, 0x3F, 0x40, 0x7F, 0x80, 0x81, 0x82, 0xBF, 0xC0, 0xC1, 0xC2, 0xC3, 0xC4, 0xE0,
         0xF0, 0xF1, 0xFD, 0xFE, 0xFF)
NOT_TYPES = (1, 3, 9, 10, 15, 255)       # the legacy types, a module, no type at all: RR_RDBLOAD_E_TYPE


def zl_of(n_entries):
    """A ziplist of n one-byte string entries 'a' (3 bytes each: prevlen, 0x01, 'a')."""
    body = b"".join(bytes([0 if k == 0 else 3, 1]) + b"a" for k in range(n_entries))
    tail = 10 + 3 * (n_entries - 1) if n_entries else 10
    return struct.pack("<IIH", 11 + len(body), tail, n_entries) + body + b"\xFF"


def intset_of(enc, vals):
    return struct.pack("<II", enc, len(vals)) + b"".join(int(v).to_bytes(enc, "little", signed=True) for v in vals)


def node_of(entries):
    """A ziplist from raw (encoding + body) entries, the prevlen chain computed."""
    body, prev, tail = b"", 0, 10
    for e in entries:
        tail = 10 + len(body)
        ent = (bytes([prev]) if prev < 254 else b"\xFE" + struct.pack("<I", prev)) + e
        body += ent
        prev = len(ent)
    return struct.pack("<IIH", 11 + len(body), tail, len(entries)) + body + b"\xFF"


def raw(b):
    return ref.save_len(len(b)) + b


def lzf_str(stream, ulen):
    return b"\xC3" + ref.save_len(len(stream)) + ref.save_len(ulen) + stream


def lz(b):
    """b as an LZF string by the CPU compressor (it must compress)."""
    comp = lzf.compress(b, len(b) - 4)
    assert comp is not None and lzf.decompress(comp, len(b)) == b
    return lzf_str(comp, len(b))


def class_node():
    """A List node with every ziplist entry class: the three string length forms, the thirteen
    immediate integers' ends, the five integer widths, and an entry of 256 bytes so that the one
    behind it carries a 5-byte prevlen."""
    return node_of([bytes([5]) + b"hello",                                   # ZIP_STR_06B
                    bytes([0x40, 2]) + b"hi",                                # ZIP_STR_14B
                    b"\x80" + struct.pack(">I", 3) + b"abc",                 # ZIP_STR_32B
                    b"\xF1", b"\xFD",                                        # 0 and 12
                    b"\xFE\x85",                                             # int8 -123
                    b"\xC0\x00\x80",                                         # int16 -32768
                    b"\xF0\xFF\xFF\x7F",                                     # int24 2^23 - 1
                    b"\xD0\x00\x00\x00\x80",                                 # int32 -2^31
                    b"\xE0" + struct.pack("<q", -2**63),                     # int64
                    bytes([0x41, 0x00]) + b"wxyz" * 64,                      # 256 bytes
                    bytes([3]) + b"end"])                                    # behind it: prevlen 0xFE + u32


def seeds():
    """[(type, payload)]: valid under OPTS or RR_RDBLOAD_E_CONVERT under it, nothing else."""
    sc = struct.pack("<d", 1.5) + struct.pack("<d", -2.25)
    text = b"the quick brown fox jumps over the lazy dog, the quick brown fox jumps over"
    node = class_node()
    out = [
        (S, raw(b"hello world!")),                                           # raw text
        (S, raw(b"-922337203685477580")),                                    # raw decimal, 19 bytes: enc INT
        (S, b"\xC0\x85"),                                                    # the integer forms
        (S, b"\xC1\x00\x80"),
        (S, b"\xC2\x00\x00\x00\x80"),                                        # "-2147483648": 11 bytes of text
        (S, lz(text)),                                                       # an LZF string
        (S, lz(b"12" * 9)),                                                  # LZF digits, 18 bytes: enc INT
        (S, b"\xC3\x05\x0A\x00a\xE0\x00\x00"),                               # 'a', then a match of 9 at distance 1
        (SET, b"\x03" + raw(b"member") + b"\xC1\x39\x30" + lz(b"xy" * 20)),  # raw, integer form, LZF
        (SET, b"\x02" + raw(b"17") + b"\xC0\x07"),                           # integers only: CONVERT at n <= 2
        (HASH, b"\x40\x01" + raw(b"field") + lz(b"value-" * 12)),            # the 14-bit count form; 72 > 64 stays
        (ZSET, b"\x02" + lz(b"ab" * 18) + sc[:8] + raw(b"m") + sc[8:]),      # n 2 > 1 stays
        (ISET, raw(intset_of(4, [-5, 70000]))),                              # n 2 <= 2 stays
        (ISET, lz(intset_of(2, [7] * 40))),                                  # n 40: CONVERT
        (HZL, raw(zl_of(4))),                                                # zllen / 2 == 2 > 1: CONVERT
        (ZZL, raw(zl_of(2))),                                                # 1 <= 1 stays
        (ZZL, lz(zl_of(20))),                                                # CONVERT
        (L, b"\x02" + raw(zl_of(2)) + raw(node)),                            # two nodes, every entry class
        (L, b"\x02" + lz(node) + raw(zl_of(0))),                             # the same node as LZF, then an empty one
    ]
    return out


def mutants(typ, p):
    """[(type, payload, kind, position)] of one seed, in a fixed order."""
    out = []
    for i, b in enumerate(p):
        vals = list(SUBST) + [b ^ 1, (b + 1) & 0xFF, (b - 1) & 0xFF, b ^ 0x80]
        for v in dict.fromkeys(vals):                    # each value once, first-seen order
            if v != b:
                out.append((typ, p[:i] + bytes([v]) + p[i + 1:], "byte", i))
    for k in range(len(p)):
        out.append((typ, p[:k], "prefix", k))
    out.append((typ, p + b"\x00", "append", 0x00))
    out.append((typ, p + b"\xFF", "append", 0xFF))
    for t in ld.TYPES:
        if t != typ:
            out.append((t, p, "type", t))
    for t in NOT_TYPES:
        out.append((t, p, "type", t))
    return out


def corpus():
    """(types, payloads, origin) over every seed: the seed itself first, then its mutants."""
    types, pays, origin = [], [], []
    for si, (typ, p) in enumerate(seeds()):
        types.append(typ); pays.append(p); origin.append((si, "seed", 0))
        for t, q, kind, pos in mutants(typ, p):
            types.append(t); pays.append(q); origin.append((si, kind, pos))
    return types, pays, origin
