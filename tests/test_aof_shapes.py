"""CPU tests of tests/aof_shapes.py: every builder reaches the edge it is named for, decided by
tests/aof_reference.py and the host build of the score parser (rr.aof_score_text) alone.  A builder
changed so that it misses its edge fails here, without a GPU; tests/test_gpu_aof_edges.py then holds the
kernels to the reference on the same batches."""
import numpy as np

import redrock_old_amd as rr

import aof_reference as ar
import aof_shapes as sh


reference = sh.reference


def g17(t):
    return ("%.17g" % float(t)).encode()


def score_args(cmds):
    """The score arguments of a slice's ZADD commands."""
    return [x for a in ar.parse_resp(cmds) if a[0] == b"ZADD" for x in a[2::2]]


# ---- A ----------------------------------------------------------------------------------------------------
def test_score_texts_are_taken_and_long():
    """Guards A: every text is inside the grammar for the host parser, float() and the restatement alike
    (no refused case), 1,000 of them divide more than 300 times and 1,000 multiply; the seams, the 39- and
    40-byte texts, the split digits and the text at the arena's end are there."""
    s = sh.score_text_batch()
    texts = s.meta["texts"]
    assert len(texts) == sh.N_TEXTS == len(s.values) * sh.WAVE
    refused = [t for t in texts if not (rr.aof_score_text(t) == g17(t) == ar.score_text(t))]
    assert refused == []
    firsts = [sh.first_exponent(t) for t in texts]
    assert sum(1 for x in firsts if x is not None and x < -300) >= 1000
    assert sum(1 for x in firsts if x is not None and -326 <= x < -300) >= 1000   # and not the shortcut to zero
    assert sum(1 for x in firsts if x is not None and x > 0) >= 1000
    assert sum(1 for x in firsts if x is not None and 0 < x < 310) >= 1000
    assert {t.encode() for t in sh.HALFWAY} <= set(texts)
    exps = {(sh.decimal_parts(t)[2], sh.decimal_parts(t)[1]) for t in texts if t not in (b"inf", b"-inf")}
    for e in sh.SEAM_EXPONENTS:
        assert (e, 1) in exps and (e, 17) in exps, e
    assert sum(1 for t in texts if len(t) == 39) >= 4 and sum(1 for t in texts if len(t) == 40) >= 4
    assert max(len(t) for t in texts) == 40
    split = [t for t in texts if b"." in t and sh.decimal_parts(t)[1] == 17 and b"000." in t and b".000" in t]
    assert len(split) >= 3
    assert max(sh.parse_words(t) for t in texts) == 29 and min(sh.parse_words(t) for t in texts) == 0
    # a different text in every lane of every value, and the last one ends the arena
    assert all(len(set(texts[v:v + sh.WAVE])) >= 60 for v in range(0, sh.N_TEXTS, sh.WAVE))
    assert bytes(s.arena[-len(sh.LAST_TEXT):]) == sh.LAST_TEXT == texts[-1]
    last = s.elems[-1]
    assert int(last["data"]) + int(last["len"]) == len(s.arena) and last["kind"] == rr.K_STR
    data, offs, status, totals, slices = reference(s)
    assert (status == 0).all()
    assert [x for c in slices for x in score_args(c)] == [g17(t) for t in texts]


def test_score_ints_round():
    """Guards A's integer entries: the values where (double) v rounds, both signs, all printed."""
    s = sh.score_int_batch()
    ints = s.meta["ints"]
    assert len(ints) == sh.N_INTS and -2**63 in ints and 2**63 - 1 in ints and -(2**63 - 1) in ints
    for k in range(9):
        assert 2**53 + k in ints and -(2**53 + k) in ints
    for k in range(53, 63):
        assert {2**k, 2**k + 1, 2**k - 1} <= set(ints)
    assert sum(1 for v in ints if int(float(v)) != v) >= 300           # most do not fit 53 bits
    _, _, status, _, slices = reference(s)
    assert (status == 0).all()
    assert [x for c in slices for x in score_args(c)] == [g17(v) for v in ints]


def test_refused_batch():
    """Guards A's refused texts: all of REFUSED, each at a lane of its own, each alone in its value."""
    s = sh.refused_batch()
    assert len(sh.REFUSED) == 23 and len(s.values) == 46
    assert all(rr.aof_score_text(t.encode()) is None and ar.score_text(t.encode()) is None for t in sh.REFUSED)
    assert len({p % sh.WAVE for p in s.meta["at"]}) == 23 and {p // sh.WAVE for p in s.meta["at"]} == {0, 1, 2}
    _, _, status, totals, slices = reference(s)
    assert (status[0::2] == rr.AOF_E_CPU).all() and (status[1::2] == 0).all() and totals["n_bad"] == 23
    for j, t in enumerate(sh.REFUSED):                                   # without the text the value is written
        b = int(s.values["elem_base"][2 * j]) + 2 + 2 * s.meta["at"][j]
        assert bytes(s.arena[int(s.elems["data"][b]):][:int(s.elems["len"][b])]) == t.encode()
        e = s.elems.copy()
        e["kind"][b], e["data"][b] = rr.K_INT, 3
        assert ar.aof_batch(s.values[2 * j:2 * j + 1], e, s.arena, *ar.keys_of([b"k"]))[2][0] == 0


# ---- B ----------------------------------------------------------------------------------------------------
def test_stale_schedules():
    """Guards B: the schedules put a one-word number behind a 29-word one and the other way round, in every
    lane, and the fifth one runs on a few lanes."""
    words = [[0 if isinstance(x, int) else sh.parse_words(x) for x in sc] for sc in sh.SCHEDULES]
    assert words[0][:2] == [29, 1] and words[1][:2] == [1, 29] and words[1][2] >= 20 and words[2][0] >= 20
    assert words[2][1] >= 24 and words[3][1] >= 24 and words[4][0] == 29
    s = sh.stale_rounds_batch()
    assert int(s.values["n_elems"][0]) == 1 + 2 * 3 * sh.WAVE
    _, _, status, _, slices = reference(s)
    assert (status == 0).all()
    got = score_args(slices[0])
    for lane in range(sh.WAVE):
        want = sh.schedule_of(lane)
        assert [got[lane], got[sh.WAVE + lane], got[2 * sh.WAVE + lane]] == [g17(x) for x in want]
    assert {sh.SCHEDULES.index(sh.schedule_of(lane)) for lane in range(sh.WAVE)} == {0, 1, 2, 3, 4}


def test_stale_values_share_a_wave():
    """Guards B across values: of each pair (v, v + RR_AOF_MAX_WAVES) one prints a text below 1e-300 in
    every lane's reach and the other single digits only; both orders, all four orders of the encodings."""
    s = sh.stale_values_batch()
    n = rr.AOF_MAX_WAVES + sh.STALE_PAIRS
    assert len(s.values) == n
    pick = list(range(sh.STALE_PAIRS)) + list(range(rr.AOF_MAX_WAVES, n))
    sub = sh.Shape(s.values[pick], s.elems, s.arena, [s.names[i] for i in pick], None, {})
    _, _, status, _, slices = reference(sub)
    assert (status == 0).all()
    orders = set()
    for p in range(sh.STALE_PAIRS):
        a, b = score_args(slices[p]), score_args(slices[sh.STALE_PAIRS + p])
        assert len(a) == len(b) == 70
        long, short = (a, b) if p % 2 == 0 else (b, a)
        assert any(sh.first_exponent(t) is not None and sh.first_exponent(t) < -300 for t in long)
        assert all(len(t) == 1 and t.isdigit() for t in short)
        orders.add((int(s.values["type"][p]), int(s.values["type"][rr.AOF_MAX_WAVES + p]), p % 2))
    assert len(orders) == 8
    mid = s.values[sh.STALE_PAIRS:rr.AOF_MAX_WAVES]
    assert (mid["type"] == rr.T_STRING).all() and (mid["n_elems"] == 1).all()


# ---- C ----------------------------------------------------------------------------------------------------
def test_seam24_crosses_every_piece():
    """Guards C: a bulk that begins 2^24 bytes into its command, a single bulk of 2^24 bytes and one byte
    either side, one lane's cost and payload above 2^24, a wave whose low 24 bits sum past 2^24, and a
    payload total above 2^24."""
    s = sh.seam24_batch()
    _, offs, status, totals, slices = reference(s)
    assert (status == 0).all() and totals["payload"] > sh.SEAM
    assert [len(c) - len(b"*3\r\n$3\r\nSET\r\n$2\r\nk0\r\n") - 2 - len(b"$16777216\r\n") for c in slices[:3:2]] == [sh.SEAM - 1, sh.SEAM + 1]
    assert b"$16777215\r\n" in slices[0][:40] and b"$16777216\r\n" in slices[1][:40] and b"$16777217\r\n" in slices[2][:40]
    li, hi, si = s.meta["list"], s.meta["hash"], s.meta["set"]
    tail = b"$3\r\n" + s.meta["tail"] + b"\r\n"
    cmd = slices[li][:slices[li].index(b"*3\r\n$9\r\nPEXPIREAT")]
    assert cmd.endswith(tail) and len(cmd) - len(tail) >= sh.SEAM
    d = s.elems[int(s.values["elem_base"][hi]):][:2]
    assert int(d["len"][0]) < sh.SEAM < int(d["len"].sum())             # lane 0 of the pair: cost and payload
    m = s.elems[int(s.values["elem_base"][si]):][:sh.WAVE]
    assert (m["len"] < sh.SEAM).all() and int(m["len"].sum()) > sh.SEAM and len(m) == sh.WAVE
    assert int(offs[-1]) > 6 * sh.SEAM


# ---- D ----------------------------------------------------------------------------------------------------
def test_past_4gib_offsets():
    """Guards D: the tail of the repeated batch lies past 2^32, every aggregate encoding with three commands
    and an expiry in it."""
    s = sh.past_4gib_batch()
    _, offs1, status, totals1, slices = reference(s)
    big = sh.Shape(s.values[:1], s.elems, s.arena, s.names[:1], s.expires[:1], {})
    totals_big = reference(big)[3]
    assert (status == 0).all() and int(offs1[1]) == len(b"*3\r\n$3\r\nSET\r\n$1\r\nk\r\n$65536\r\n") + sh.BIG_LEN + 2
    offsets, totals = sh.past_4gib_expect(offs1, totals1, totals_big, len(s.values) - 1)
    assert int(offsets[sh.NBIG]) > 1 << 32 and int(offsets[1]) == int(offs1[1]) and len(offsets) == sh.NBIG + len(s.values)
    assert int(offsets[1]) % 16 != 0 and totals["bytes"] == int(offsets[-1])
    assert sorted(int(t) for t in s.values["type"][1:]) == sorted(sh.AGGREGATES)
    assert all(c.count(b"PEXPIREAT") == 1 and c.count(b"\r\n$1\r\n" + k + b"\r\n") >= 4 for c, k in zip(slices[1:], s.names[1:]))
    assert all(len(k) == 1 for k in s.names)


# ---- E ----------------------------------------------------------------------------------------------------
def test_body_alignment_matrix():
    """Guards E for bodies: every (source mod 16, destination mod 16) pair for the lengths around SHORT_BODY
    and 64 pairs for the loop's second trip, in a List and as a Hash value."""
    s = sh.body_alignment()
    _, offs, status, _, slices = reference(s)
    assert (status == 0).all()
    seen = {}
    for i, (a, body) in zip(s.meta["at"], s.meta["info"]):
        assert len(body) > sh.SHORT_BODY
        assert int(offs[i]) % 16 == 0 and int(s.elems["data"][int(s.values["elem_base"][i]) + 1]) % 16 == a
        dst = int(offs[i]) + slices[i].index(body)
        seen.setdefault((int(s.values["type"][i]), len(body)), set()).add((a, dst % 16))
    for typ in (sh.L, sh.HH):
        for ln in sh.BODY_SMALL:
            assert len(seen[(typ, ln)]) == 256
        for ln in sh.BODY_LONG:
            assert len(seen[(typ, ln)]) == 64
    assert len(seen) == 12


def test_key_alignment_matrix():
    """Guards E for keys: every (source mod 16, destination mod 16) pair for every key length."""
    s = sh.key_alignment_batch()
    kd, ko = ar.keys_of(s.names)
    _, offs, status, _, slices = reference(s)
    assert (status == 0).all()
    seen = {}
    for i, (a, d, key) in zip(s.meta["at"], s.meta["info"]):
        assert s.names[i] == key and int(ko[i]) % 16 == a
        dst = int(offs[i]) + slices[i].index(b"\r\n" + key + b"\r\n") + 2
        assert dst % 16 == d
        seen.setdefault(len(key), set()).add((int(ko[i]) % 16, dst % 16))
    assert sorted(seen) == sorted(sh.KEY_LENGTHS) and all(len(v) == 256 for v in seen.values())


# ---- F ----------------------------------------------------------------------------------------------------
def test_digit_seams():
    """Guards F: every "$len" seam of a member, "*9" / "*10", "*8" / "*10", "*98" / "*100", the keys of 999
    and 1,000 bytes, the expiries and the integers at their widest."""
    s = sh.digit_seam_batch()
    _, _, status, _, slices = reference(s)
    assert (status == 0).all()
    for ln in sh.MEMBER_SEAMS:
        assert (b"\r\n$%d\r\n" % ln) in slices[0]
    for x in (-2**63, 2**63 - 1, 10**18, 10**18 - 1, 9, 10):
        assert (b"\r\n$%d\r\n%d\r\n" % (len(str(x)), x)) in slices[0]
    heads = {}
    for i, c in enumerate(slices):
        for a in ar.parse_resp(c):
            heads.setdefault((int(s.values["type"][i]), a[0]), set()).add(len(a))
    for typ, verb in ((sh.L, b"RPUSH"), (sh.SI, b"SADD"), (sh.SH, b"SADD")):
        assert {9, 10, 66} <= heads[(typ, verb)]
    for typ, verb in ((sh.HH, b"HMSET"), (sh.ZS, b"ZADD"), (sh.HZ, b"HMSET"), (sh.ZZ, b"ZADD")):
        assert {8, 10, 98, 100, 130} <= heads[(typ, verb)]
    joined = b"".join(slices)
    assert joined.count(b"\r\n$999\r\n") >= 5 and joined.count(b"\r\n$1000\r\n") >= 5
    for i, c in enumerate(slices):                                      # every expiry in a PEXPIREAT of its key, last
        last = ar.parse_resp(c)[-1]
        assert last == [b"PEXPIREAT", s.names[i], b"%d" % s.expires[i]]
    assert (b"PEXPIREAT\r\n$2\r\nk0\r\n$20\r\n-9223372036854775808\r\n") in slices[0]
    assert set(s.expires) == set(sh.EXPIRY_SEAMS)


# ---- G ----------------------------------------------------------------------------------------------------
def test_intset_limits():
    """Guards G: the limits of width 2 and 4 at lane 0, lane 63 and in the second round are written, one
    past each is RR_E_ENCODE between two written values, the other widths are refused, width 8 takes both
    ends of int64."""
    s = sh.intset_batch()
    _, _, status, _, slices = reference(s)
    bad = s.meta["bad"]
    assert len(bad) == 12 + 4 and sorted(np.nonzero(status)[0].tolist()) == sorted(bad)
    assert (status[bad] == rr.E_ENCODE).all()
    for i in bad[:12]:
        assert status[i - 1] == 0 and status[i + 1] == 0 and int(s.values["enc"][i]) in (2, 4)
        w = int(s.values["enc"][i])
        lim = 1 << (8 * w - 1)
        el = s.elems["data"][int(s.values["elem_base"][i]):][:100].view(np.int64)
        out = [(k, int(x)) for k, x in enumerate(el) if not -lim <= x < lim]
        assert len(out) == 1 and out[0][0] in sh.INTSET_PLACES and out[0][1] in (-lim - 1, lim)
        good = s.elems["data"][int(s.values["elem_base"][i - 1]):][:100].view(np.int64)
        assert int(good[out[0][0]]) in (-lim, lim - 1)
    assert sorted(int(s.values["enc"][i]) for i in bad[12:]) == [0, 1, 3, 16]
    joined = b"".join(slices)
    for x in (-2**15, 2**15 - 1, -2**31, 2**31 - 1, -2**63, 2**63 - 1):
        assert joined.count(b"\r\n%d\r\n" % x) == 3
    for x in (-2**15 - 1, 2**15, -2**31 - 1, 2**31):
        assert (b"\r\n%d\r\n" % x) not in joined


# ---- H ----------------------------------------------------------------------------------------------------
def test_precedence_batch():
    """Guards H: the bad descriptor sits in a later round than the refused text (RR_E_ENCODE all the same),
    and without it the value is RR_AOF_E_CPU."""
    s = sh.precedence_batch()
    _, _, status, _, _ = reference(s)
    assert len(s.meta["encode"]) == 5 and len(s.meta["cpu"]) == 3
    assert (status[s.meta["encode"]] == rr.E_ENCODE).all() and (status[s.meta["cpu"]] == rr.AOF_E_CPU).all()
    acap = len(s.arena)

    def fits(t, k, d):
        """Descriptor k of a value's items, as include/rr_aof.h wants it."""
        if t == sh.ZS and k % 2:
            return d["kind"] == rr.K_SCORE
        return (d["kind"] == rr.K_STR and int(d["data"]) + int(d["len"]) <= acap) or (d["kind"] == rr.K_INT and t == sh.ZZ)

    def refused(d):
        if d["kind"] == rr.K_SCORE:
            return int(d["data"]) & 0x7FFFFFFFFFFFFFFF > 0x7FF0000000000000
        return d["kind"] == rr.K_STR and bytes(s.arena[int(d["data"]):][:int(d["len"])]) == b"nan"

    rounds = set()
    for i in s.meta["encode"] + s.meta["cpu"]:
        b, c, t = int(s.values["elem_base"][i]), int(s.values["n_elems"][i]), int(s.values["type"][i])
        ents = s.elems[b + (t == sh.ZZ):b + c]
        wrong = [k for k in range(len(ents)) if not fits(t, k, ents[k])]
        nans = [k // 2 for k in range(1, len(ents), 2) if refused(ents[k])]
        assert len(nans) == 1
        if i in s.meta["cpu"]:
            assert wrong == [] and (nans[0] // sh.WAVE == 3 or t == sh.ZS)   # nothing to refuse but the text
            continue
        assert len(wrong) == 1 and nans[0] < sh.WAVE <= wrong[0] // 2      # one bad descriptor, in a later round
        rounds.add((t, wrong[0] // 2 // sh.WAVE, wrong[0] // 2 % sh.WAVE))
        if ents["kind"][wrong[0]] == rr.K_STR and t == sh.ZZ:
            assert int(ents["data"][wrong[0]]) + int(ents["len"][wrong[0]]) == acap + 1
    assert {(t, r) for t, r, _ in rounds} == {(sh.ZZ, 1), (sh.ZZ, 2), (sh.ZZ, 3), (sh.ZS, 1)}
    assert (sh.ZZ, 3, 63) in rounds and (sh.ZZ, 3, 7) in rounds


# ---- I ----------------------------------------------------------------------------------------------------
def test_capacity_batch_and_refused_blobs():
    s = sh.capacity_batch()
    _, offs, status, _, _ = reference(s)
    assert (status == 0).all() and int(offs[1]) == 0 and len(s.values) == 2 + len(sh.AGGREGATES)
    from helpers import batch_from_blobs
    data, o = batch_from_blobs(sh.refused_blobs())
    v, e, a, _ = rr.host_decode(data, o)
    assert (v["status"] == 0).all()
    st = ar.aof_batch(v, e, a, *ar.keys_of([b"a", b"b", b"c", b"d"]))[2]
    assert st.tolist() == [rr.AOF_E_CPU] * 3 + [0]
