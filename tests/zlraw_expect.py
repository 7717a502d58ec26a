"""The expected output of a raw-ziplist decode (RR_CTX_ZL_RAW), derived from the STRICT oracle.

The oracle (oracle/) has no raw mode.  For a batch, expect_raw() takes the oracle's strict output
and rewrites only the values the mode changes:

  a type-12/13 value of L >= 13 bytes whose u64 at byte 5 equals L - 13 (and fits 32 bits), with
  strict status RR_OK or RR_E_ZL_CORRUPT, becomes {status 0, enc 0, lru & 0xFFFFFF, n_elems 1},
  reserves ONE slot, and that slot is ZLRAW{blob offset + 13, L - 13, zenc 0}.  For a strict-OK
  value the oracle's own first descriptor must already be that ZLRAW (asserted).

Every other value keeps the oracle's record, descriptors and reservation (the oracle's elem_base
differences).  elem_base, the compacted descriptor array and the totals are then recomputed, and
the capacity rule (a valid value whose slots pass elem_cap: RR_E_CAPACITY, nothing written)
applied on top.  No engine code is used here.
"""
import numpy as np

import redrock_old_amd as rr
from oracle import cpu

ST_OK, ST_ZL_LEN, ST_ZL_CORRUPT, ST_CAPACITY = 0, 9, 10, 11
ZL_TYPES = (12, 13)


def _le(data, at, nbytes):
    """little-endian unsigned integers of nbytes bytes at the byte positions `at`"""
    idx = at[:, None].astype(np.int64) + np.arange(nbytes, dtype=np.int64)[None, :]
    b = data[idx].astype(np.uint64)
    return (b << (np.arange(nbytes, dtype=np.uint64) * np.uint64(8))[None, :]).sum(axis=1, dtype=np.uint64)


def expect_raw(data, offs, elem_cap=None, nthreads=8):
    """(values, elems, totals, info) a raw-mode decode of the batch must give.  info: 'accepted'
    (mask of the values the mode rewrote), 'corrupt_accepted' / 'len_rejected' (the counts the
    anti-vacuity condition needs), 'strict' (the oracle's own strict output)."""
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    n = len(offs) - 1
    ov, oe, oa, ot = cpu.decode(data, offs, nthreads=nthreads)   # (full capacity: the descriptor bound)
    assert (ov["status"] != ST_CAPACITY).all()
    o0 = offs[:-1].astype(np.int64)
    lens = np.diff(offs.astype(np.int64))
    typ = np.zeros(n, np.int64)
    typ[lens > 0] = data[o0[lens > 0]]
    cand = (lens >= 13) & np.isin(typ, ZL_TYPES)
    lz = np.zeros(n, np.uint64)
    lru = np.zeros(n, np.uint64)
    if cand.any():
        lz[cand] = _le(data, o0[cand] + 5, 8)
        lru[cand] = _le(data, o0[cand] + 1, 4) & np.uint64(0xFFFFFF)
    st = ov["status"].astype(np.int64)
    acc = cand & (lz == (lens - 13).astype(np.uint64)) & (lz < np.uint64(1 << 32)) & np.isin(st, (ST_OK, ST_ZL_CORRUPT))

    # the oracle's reservations: its elem_base differences
    base_or = ov["elem_base"].astype(np.int64)
    r_or = np.diff(np.concatenate([base_or, [int(ot["n_elems"])]]))
    assert (r_or >= 0).all() and len(oe) == int(ot["n_elems"])
    # its payload per value: a ziplist counts its ZLRAW, the others their STR descriptors
    owner = np.repeat(np.arange(n), r_or)
    zl_owner = np.isin(typ, ZL_TYPES)[owner]
    counted = np.where(zl_owner, oe["kind"] == rr.K_ZLRAW, oe["kind"] == rr.K_STR)
    pay_or = np.bincount(owner, weights=oe["len"].astype(np.float64) * counted, minlength=n).astype(np.int64)
    pay_or[st != ST_OK] = 0
    assert int(pay_or.sum()) == int(ot["payload"]), "helper's per-value payload disagrees with the oracle's total"

    raw_desc = np.zeros(n, rr.ELEM_DT)
    raw_desc["data"] = (o0 + 13).astype(np.uint64)
    raw_desc["len"] = lz.astype(np.uint32)
    raw_desc["kind"] = rr.K_ZLRAW
    ok_acc = acc & (st == ST_OK)
    assert np.array_equal(oe[base_or[ok_acc]], raw_desc[ok_acc]), "a strict-OK ziplist's first descriptor is not its ZLRAW"

    r_new = np.where(acc, 1, r_or)
    base_new = np.concatenate([[0], np.cumsum(r_new)])[:-1]
    total = int(r_new.sum())
    elems = np.zeros(total, rr.ELEM_DT)
    keep = ~acc
    rk = r_or[keep]
    if rk.sum():
        within = np.arange(int(rk.sum())) - np.repeat(np.cumsum(rk) - rk, rk)
        elems[np.repeat(base_new[keep], rk) + within] = oe[np.repeat(base_or[keep], rk) + within]
    elems[base_new[acc]] = raw_desc[acc]

    values = ov.copy()
    values["enc"][acc] = 0
    values["status"][acc] = ST_OK
    values["lru"][acc] = lru[acc].astype(np.uint32)
    values["n_elems"][acc] = 1
    values["elem_base"] = base_new.astype(np.uint32)
    pay = np.where(acc, lz.astype(np.int64), pay_or)

    if elem_cap is not None:   # a valid value whose slots pass the capacity: RR_E_CAPACITY, nothing written
        fits = base_new + r_new <= elem_cap
        cut = ~fits & (values["status"] == ST_OK)
        values["status"][cut] = ST_CAPACITY
        pay[cut] = 0
        nofit = np.repeat(~fits, r_new)
        elems[nofit] = np.zeros(1, rr.ELEM_DT)[0]
        elems = elems[:min(total, elem_cap)]
    totals = {"n_elems": total, "bytes": int(offs[-1]), "n_bad": int((values["status"] != ST_OK).sum()),
              "payload": int(pay[values["status"] == ST_OK].sum())}
    info = {"accepted": acc, "corrupt_accepted": int((acc & (st == ST_ZL_CORRUPT)).sum()),
            "len_rejected": int((values["status"] == ST_ZL_LEN).sum()), "strict": (ov, oe, oa, ot)}
    return values, elems, totals, info


def assert_anti_vacuity(info):
    """Every batch-level test: the batch holds a value strict mode rejects as RR_E_ZL_CORRUPT that
    raw mode accepts, and an RR_E_ZL_LEN that stays rejected (both read off the oracle alone)."""
    assert info["corrupt_accepted"] >= 1, "no strict-CORRUPT value that raw mode accepts in this batch"
    assert info["len_rejected"] >= 1, "no RR_E_ZL_LEN value in this batch"


# ---- batch builders shared by the CPU and GPU tests -----------------------------------------
def zl_blob(tag, body, lru=0x123456, lz=None):
    """type tag | lru | u64 count (default: the body's length) | body"""
    return bytes([tag]) + int(lru).to_bytes(4, "little") + int(len(body) if lz is None else lz).to_bytes(8, "little") + body


def good_ziplist(entries):
    """A valid ziplist of short byte-string entries (6-bit string encoding, 1-byte prevlen)."""
    body, prev, tail = b"", 0, 10
    for e in entries:
        assert len(e) < 64 and prev < 254
        tail = 10 + len(body)
        ent = bytes([prev, len(e)]) + e
        body += ent
        prev = len(ent)
    zlbytes = 10 + len(body) + 1
    return zlbytes.to_bytes(4, "little") + tail.to_bytes(4, "little") + len(entries).to_bytes(2, "little") + body + b"\xff"


def corrupt_in_place(blobs, rng, frac, tags=ZL_TYPES):
    """Overwrite one ziplist body byte (length kept) in about `frac` of the ziplist blobs whose
    count field is right; returns the new list."""
    out = []
    for b in blobs:
        if len(b) > 24 and b[0] in tags and int.from_bytes(b[5:13], "little") == len(b) - 13 and rng.random() < frac:
            m = bytearray(b)
            at = int(rng.integers(13, len(m)))
            m[at] ^= 1 << int(rng.integers(0, 8))
            b = bytes(m)
        out.append(b)
    return out


def with_len_defects(blobs, rng, k=3):
    """Append k copies of ziplist blobs whose count field is off by one (RR_E_ZL_LEN in any mode)."""
    zl = [b for b in blobs if len(b) >= 24 and b[0] in ZL_TYPES]
    out = list(blobs)
    for i in range(k):
        b = zl[int(rng.integers(len(zl)))]
        lz = int.from_bytes(b[5:13], "little") + (1 if i & 1 else -1)
        out.append(b[:5] + lz.to_bytes(8, "little") + b[13:])
    return out


def split_blobs(data, offs):
    return [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
