"""What rr_aof_batch must produce, restated in plain Python from the reference's source text
(include/rr_aof.h states the same rule).

  commands(val, descs, arena, key, expire)   (status, bytes, payload): what rewriteAppendOnlyFileRio
                                             (aof.c:1342-1370) and the rewrite*Object functions
                                             (aof.c:921-1135) write for the key holding the object
                                             desObject builds from the flat value
  score_text(text)                           %.17g of zzlGetScore's strtod, or None for a text the
                                             engine leaves to the CPU path
  aof_batch(...)                             the whole call: data, offsets, status, totals, slices
  replay(data)                               a minimal RESP parser that applies the commands to a plain
                                             Python model, and model(val, descs, arena): the same model
                                             straight from the flat value

Scores come from rdbzset_reference.d2string (a SCORE descriptor) and float(text) (a ziplist entry):
Python's float() is correctly rounded, and '%.17g' is held to the C library's in tests/test_d2string.py.
Which values are saveable is rr_encode_batch's rule, tests/encode_expect.py, plus the rule for a
ziplist's entry descriptors that include/rr_aof.h adds.
"""
import re
import struct

import numpy as np

import redrock_old_amd as rr
import rdbzset_reference as zr
from encode_expect import accepted_value

OK, E_CAPACITY, E_ENCODE, E_KEY, E_CPU = 0, 11, 12, 41, 56
ITEMS_PER_CMD = 64                                   # AOF_REWRITE_ITEMS_PER_CMD
MAX_SLICE = 0x7FFFFFF0
SCORE_TEXT_MAX, SCORE_DIGITS = 40, 17
_ZL = (rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST)
_NUM = re.compile(rb"-?(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE][+-]?[0-9]+)?", re.S)


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


# ---- rio.c:406-445 --------------------------------------------------------------------------------
def bulk_count(prefix, n):
    return prefix + str(n).encode() + b"\r\n"


def bulk_string(s):
    return bulk_count(b"$", len(s)) + bytes(s) + b"\r\n"


def bulk_longlong(v):
    return bulk_string(str(v).encode())


# ---- scores ---------------------------------------------------------------------------------------
def score_text(text):
    """The grammar of include/rr_aof.h; None: RR_AOF_E_CPU."""
    text = bytes(text)
    if text in (b"inf", b"-inf"):
        return text
    if len(text) > SCORE_TEXT_MAX:
        return None
    m = _NUM.fullmatch(text)
    if not m:
        return None
    digits = ((m.group(1) or b"") + (m.group(2) or b"") + (m.group(3) or b"")).lstrip(b"0").rstrip(b"0")
    if len(digits) > SCORE_DIGITS:
        return None
    return ("%.17g" % float(text)).encode()


def score_of_bits(bits):
    """rioWriteBulkDouble of a SCORE descriptor; None for a NaN (RR_AOF_E_CPU)."""
    v = zr.to_double(bits)
    return None if v != v else zr.d2string(bits)


# ---- one value ------------------------------------------------------------------------------------
class Cpu(Exception):
    pass


def _item_str(d, arena):
    """A STR or INT descriptor as the bytes of its bulk string."""
    return str(_signed(d[1])).encode() if d[0] == rr.K_INT else arena[d[1]:d[1] + d[2]]


def zl_entries_ok(descs, arena_cap):
    ents = descs[1:]
    return len(ents) % 2 == 0 and all(d[0] == rr.K_INT or (d[0] == rr.K_STR and d[1] + d[2] <= arena_cap) for d in ents)


def items_of(val, descs, arena):
    """(verb, [item, ...]) with an item the list of its bulk strings' bytes, in the order written.
    Raises Cpu for what is left to the CPU path."""
    t = val["type"]
    if t == rr.T_STRING:
        return b"SET", [[_item_str(descs[0], arena)]]
    if t == rr.T_LIST_QUICKLIST:                     # aof.c:935-965
        return b"RPUSH", [[_item_str(d, arena)] for d in descs]
    if t in (rr.T_SET_INTSET, rr.T_SET_HT):          # :969-1012
        return b"SADD", [[_item_str(d, arena)] for d in descs]
    if t == rr.T_HASH_HT:                            # :1111-1135
        return b"HMSET", [[_item_str(descs[k], arena), _item_str(descs[k + 1], arena)] for k in range(0, len(descs), 2)]
    if t == rr.T_ZSET_SKIPLIST:                      # :1054-1076: score, then member
        out = []
        for k in range(0, len(descs), 2):
            sc = score_of_bits(descs[k + 1][1])
            if sc is None:
                raise Cpu
            out.append([sc, _item_str(descs[k], arena)])
        return b"ZADD", out
    ents = descs[1:]
    if not ents and descs[0][2] != 11:               # the ZLRAW alone, and not the empty ziplist
        raise Cpu
    if t == rr.T_HASH_ZIPLIST:
        return b"HMSET", [[_item_str(ents[k], arena), _item_str(ents[k + 1], arena)] for k in range(0, len(ents), 2)]
    out = []                                         # ZSET_ZIPLIST, :1019-1053
    for k in range(0, len(ents), 2):
        s = ents[k + 1]
        sc = ("%.17g" % float(_signed(s[1]))).encode() if s[0] == rr.K_INT else score_text(arena[s[1]:s[1] + s[2]])
        if sc is None:
            raise Cpu
        out.append([sc, _item_str(ents[k], arena)])
    return b"ZADD", out


def commands(val, descs, arena, key, expire=-1):
    """(status, bytes, payload bytes) of a value whose status on entry is 0 and whose descriptors lie
    inside elem_cap (descs None otherwise); key None: a bad key slice."""
    if not accepted_value(val, descs, len(arena)) or (val["type"] in _ZL and not zl_entries_ok(descs, len(arena))):
        return E_ENCODE, b"", 0
    if key is None:
        return E_KEY, b"", 0
    try:
        verb, items = items_of(val, descs, arena)
    except Cpu:
        return E_CPU, b"", 0
    per = len(items[0]) if items else 1
    out = b""
    for c0 in range(0, len(items), ITEMS_PER_CMD):
        chunk = items[c0:c0 + ITEMS_PER_CMD]
        out += bulk_count(b"*", 2 + per * len(chunk)) + bulk_string(verb) + bulk_string(key)
        for it in chunk:
            out += b"".join(bulk_string(x) for x in it)
    if expire != -1:                                 # aof.c:1365-1370
        out += b"*3\r\n$9\r\nPEXPIREAT\r\n" + bulk_string(key) + bulk_longlong(expire)
    used = descs[1:] if val["type"] in _ZL else descs
    if val["type"] == rr.T_ZSET_ZIPLIST:
        used = used[0::2]                            # a score entry's text is parsed, not copied
    pay = sum(d[2] for d in used if d[0] == rr.K_STR)
    return OK, out, pay


# ---- the batch ------------------------------------------------------------------------------------
def key_slices(key_data, key_offsets, key_cap=None):
    kb = bytes(key_data)
    cap = len(kb) if key_cap is None else key_cap
    out = []
    for i in range(len(key_offsets) - 1):
        o0, o1 = int(key_offsets[i]), int(key_offsets[i + 1])
        out.append(kb[o0:o1] if o0 <= o1 <= cap and o1 - o0 < MAX_SLICE else None)
    return out


def aof_batch(values, elems, arena, key_data, key_offsets, expires=None, data_cap=None, key_cap=None):
    """(data, offsets, status, totals, slices): data has min(data_cap, offsets[n]) bytes, unwritten ones
    zero; slices[i] is b"" for a value with a non-zero status."""
    import rdb_reference as ref
    ab = arena.tobytes()
    n = len(values)
    keys = key_slices(key_data, key_offsets, key_cap)
    res, n_elems = [], 0
    for i, ((val, descs), r) in enumerate(zip(ref.flat_values(values, elems, arena), values)):
        n_elems += int(r["n_elems"])
        res.append(commands(val, descs, ab, keys[i], -1 if expires is None else int(expires[i])))
    offsets = np.zeros(n + 1, np.uint64)
    at = 0
    for i, x in enumerate(res):
        offsets[i] = at
        at += len(x[1])
    offsets[n] = at
    if data_cap is None:
        data_cap = at
    out = bytearray(min(data_cap, at))
    status = np.zeros(n, np.uint8)
    n_bad = pay = 0
    slices = []
    for i, (st, b, p) in enumerate(res):
        o = int(offsets[i])
        if st == OK and o + len(b) > data_cap:
            st = E_CAPACITY
        status[i] = st
        if st != OK:
            n_bad += 1
            slices.append(b"")
            continue
        out[o:o + len(b)] = b
        pay += p
        slices.append(b)
    totals = {"n_elems": n_elems, "bytes": at, "n_bad": n_bad, "payload": pay}
    return np.frombuffer(bytes(out), np.uint8), offsets, status, totals, slices


def keys_of(names):
    """(key_data, key_offsets) of a list of key bytes."""
    offs = np.zeros(len(names) + 1, np.uint64)
    offs[1:] = np.cumsum([len(k) for k in names], dtype=np.uint64) if names else offs[1:]
    raw = b"".join(names)
    return np.frombuffer(raw or b"\0", np.uint8).copy(), offs


# ---- the independent replay -----------------------------------------------------------------------
def parse_resp(data):
    """The commands of a RESP stream of multi-bulk requests: a list of argument lists."""
    data = bytes(data)
    p, cmds = 0, []

    def line():
        nonlocal p
        e = data.index(b"\r\n", p)
        s = data[p:e]
        p = e + 2
        return s

    while p < len(data):
        h = line()
        assert h[:1] == b"*", h
        args = []
        for _ in range(int(h[1:])):
            ln = line()
            assert ln[:1] == b"$", ln
            k = int(ln[1:])
            args.append(data[p:p + k])
            assert data[p + k:p + k + 2] == b"\r\n"
            p += k + 2
        cmds.append(args)
    return cmds


def replay(data):
    """Applies SET / RPUSH / SADD / ZADD / HMSET / PEXPIREAT to {key: object}, {key: expiry}, as the
    server would: a field or member written twice keeps its last value (a ziplist blob may hold one twice)."""
    db, exp = {}, {}
    for a in parse_resp(data):
        verb, key, rest = a[0], a[1], a[2:]
        if verb == b"SET":
            assert len(rest) == 1
            db[key] = ("string", rest[0])
        elif verb == b"RPUSH":
            assert 1 <= len(rest) <= ITEMS_PER_CMD
            db.setdefault(key, ("list", []))[1].extend(rest)
        elif verb == b"SADD":
            assert 1 <= len(rest) <= ITEMS_PER_CMD
            s = db.setdefault(key, ("set", set()))[1]
            s.update(rest)
        elif verb == b"HMSET":
            assert len(rest) % 2 == 0 and 2 <= len(rest) <= 2 * ITEMS_PER_CMD
            h = db.setdefault(key, ("hash", {}))[1]
            for k in range(0, len(rest), 2):
                h[rest[k]] = rest[k + 1]
        elif verb == b"ZADD":
            assert len(rest) % 2 == 0 and 2 <= len(rest) <= 2 * ITEMS_PER_CMD
            z = db.setdefault(key, ("zset", {}))[1]
            for k in range(0, len(rest), 2):
                z[rest[k + 1]] = struct.pack("<d", float(rest[k]))
        elif verb == b"PEXPIREAT":
            assert len(rest) == 1
            exp[key] = int(rest[0])
        else:
            raise AssertionError(verb)
    return db, exp


def model(val, descs, arena):
    """The object desObject builds from a saveable flat value, as replay() models it; None for an
    aggregate with no items (no command creates it)."""
    t = val["type"]
    s = lambda d: _item_str(d, arena)
    ents = descs[1:] if t in _ZL else descs
    if t == rr.T_STRING:
        return ("string", s(descs[0]))
    if not ents:
        return None
    if t == rr.T_LIST_QUICKLIST:
        return ("list", [s(d) for d in ents])
    if t in (rr.T_SET_INTSET, rr.T_SET_HT):
        return ("set", {s(d) for d in ents})
    if t in (rr.T_HASH_HT, rr.T_HASH_ZIPLIST):
        return ("hash", {s(ents[k]): s(ents[k + 1]) for k in range(0, len(ents), 2)})
    if t == rr.T_ZSET_SKIPLIST:
        return ("zset", {s(ents[k]): struct.pack("<Q", ents[k + 1][1]) for k in range(0, len(ents), 2)})
    z = {}
    for k in range(0, len(ents), 2):                 # zzlGetScore
        d = ents[k + 1]
        z[s(ents[k])] = struct.pack("<d", float(_signed(d[1])) if d[0] == rr.K_INT else float(arena[d[1]:d[1] + d[2]]))
    return ("zset", z)
