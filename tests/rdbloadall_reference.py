"""What rr_rdbmerge_batch and rr_rdbloadall_batch must produce, restated in plain Python
(include/rr_rdbloadall.h states the same rule).

  select(s1, s2, s3)                  (holding stage 1..3 or 0, merged status before the slice and capacity checks)
  merge(stage1, stage2, stage3, types, conv_types, data_cap)
                                      stageK = (data, offsets, status, data_cap): (out data, offsets, out_types,
                                      status, totals, blobs)
  expected(payloads, types, opts, stage_cap, data_cap), expected_batch(types, data, offsets, ...)
                                      the same from payloads, through rdbload_reference, rdbconvert_reference and
                                      rdbzset_reference: no stage kernel is involved; also returns the stages' bytes
  ws_bytes(n, stage_cap)              the one call's workspace layout"""
import numpy as np

import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbzset_reference as zr

OK, E_CAPACITY, E_CONVERT, E_SLICE = 0, 11, ld.E_CONVERT, 57
ZSET_ZIPLIST = 12
NO_TYPE = 0xFF


def select(s1, s2, s3):
    holds = (OK, E_CAPACITY)
    if s1 in holds:
        return 1, s1
    if s1 != E_CONVERT:
        return 0, s1
    if s2 in holds:
        return 2, s2
    if s2 == E_CONVERT and s3 in holds:
        return 3, s3
    return 0, E_CONVERT


def merge(stage1, stage2, stage3, types, conv_types, data_cap=None):
    """out data has min(data_cap, offsets[n]) bytes, unwritten ones zero; blobs[i] is what value i writes, or None."""
    stages = (stage1, stage2, stage3)
    n = len(stage1[1]) - 1
    sizes, status, out_types, blobs = [0] * n, np.zeros(n, np.uint8), np.full(n, NO_TYPE, np.uint8), [None] * n
    held = [0] * n
    for i in range(n):
        k, st = select(int(stage1[2][i]), int(stage2[2][i]), int(stage3[2][i]))
        if k:
            data, offs, _, cap = stages[k - 1]
            o0, o1 = int(offs[i]), int(offs[i + 1])
            if o0 > o1 or (st == OK and o1 > cap):
                st = E_SLICE
            else:
                sizes[i] = o1 - o0
                out_types[i] = (int(types[i]), int(conv_types[i]), ZSET_ZIPLIST)[k - 1]
                if st == OK:
                    blobs[i] = bytes(data[o0:o1])
                    held[i] = k
        status[i] = st
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(sizes, out=offsets[1:])
    total = int(offsets[n])
    if data_cap is None:
        data_cap = total
    out = bytearray(min(data_cap, total))
    pay = nel = 0
    for i in range(n):
        if status[i] == OK and int(offsets[i + 1]) > data_cap:
            status[i], blobs[i] = E_CAPACITY, None
        if blobs[i] is not None:
            out[int(offsets[i]):int(offsets[i + 1])] = blobs[i]
            pay += len(blobs[i])
            nel += held[i] >= 2
    totals = {"n_elems": nel, "bytes": total, "n_bad": int((status != 0).sum()), "payload": pay}
    return np.frombuffer(bytes(out), np.uint8), offsets, out_types, status, totals, blobs


def expected_batch(types, data, offsets, opts=None, stage_cap=None, data_cap=None):
    """(out data, offsets, out_types, status, totals, blobs, stage_bytes) of rr_rdbloadall_batch over an input
    batch; stage_cap None: every stage has room."""
    caps = list(stage_cap) if stage_cap is not None else [None] * 3
    d1, o1, s1, _, _ = ld.load_batch(types, data, offsets, opts, caps[0])
    d2, o2, t2, s2, _, _ = cv.convert_batch(types, data, offsets, s1, opts, caps[1])
    d3, o3, s3, _, _ = zr.zset_batch(types, data, offsets, s2, opts, caps[2])
    full = [int(o[-1]) for o in (o1, o2, o3)]
    caps = [full[k] if caps[k] is None else caps[k] for k in range(3)]
    return merge((d1, o1, s1, caps[0]), (d2, o2, s2, caps[1]), (d3, o3, s3, caps[2]), types, t2, data_cap) + (full,)


def expected(payloads, types, opts=None, stage_cap=None, data_cap=None):
    return expected_batch(types, *ld.pack(payloads), opts, stage_cap, data_cap)


def a16(x):
    return (x + 15) & ~15


def ws_bytes(n, stage_cap):
    """offsets | totals | s1, s2, s3, conv_types | the three data areas, each part rounded up to 16."""
    return a16(3 * 8 * (n + 1)) + 3 * 32 + a16(4 * n) + sum(a16(int(c)) for c in stage_cap)
