"""rr_rdbmerge_batch on the batches of tests/rdbmerge_shapes.py, through test_gpu_rdbloadall.merge_device and
loadall: every byte of the output room, the offsets, status, out_types and totals against
tests/rdbloadall_reference.py, canaries behind every buffer.  What the shapes are for: wave_find past its second
level and the lanes' own search over runs of empty values longer than a step; the emit prologue's second stride
and the scan across look-back groups, with both forms of its wave sums; out_cap inside a piece, a row and a span;
empty blobs at and past the cap; pieces of sixteen one-byte values; holes (a stage's RR_E_CAPACITY values) from
one byte to more than a span; load_seg on a holding batch of under 16 bytes and on one with room behind its last
byte; and the one call over payloads whose second stage ran short.  tests/test_rdbmerge_shapes.py holds the
shapes to account on the CPU."""
import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import rdbloadall_reference as la
import rdbmerge_shapes as sh
from test_gpu_rdbloadall import CANARY, Out, _dev, _offs, loadall, merge_device

pytestmark = pytest.mark.gpu

MID = sh.mid_caps()


def run(engine, shape, cap=None, fast=False):
    """The shape's stage batches through the primitive; the expectation merge()'s, or fast_merge's image."""
    stages = shape.stages()
    want = shape.fast(cap, stages=stages) if fast else None
    return merge_device(engine, stages, *sh.type_bytes(shape.n), cap, want=want)


# ---- A ----------------------------------------------------------------------------------------------------
def test_deep_search_and_second_stride(engine):
    shape = sh.deep_search()
    want = run(engine, shape, fast=True)
    assert shape.n > rr.RDBMERGE_MAX_WAVES * 64 and want[4]["bytes"] > 5_000_000 and want[4]["n_bad"] > 30000


# ---- B ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", range(len(MID.caps)))
def test_mid_caps(engine, at):
    cap = MID.caps[at]
    want = run(engine, MID, cap)
    first = int(np.nonzero(want[3])[0][0])
    assert int(want[1][first]) <= cap < int(want[1][first + 1]) and (want[3][first:] == sh.CAP).all()


# ---- C ----------------------------------------------------------------------------------------------------
def test_empty_at_cap(engine):
    shape = sh.empty_at_cap()
    want = run(engine, shape, shape.caps[0])
    assert want[3][shape.facts["at_cap"]].tolist() == [0, sh.BAD[0], 0, 0]
    assert want[3][shape.facts["past"]].tolist() == [sh.CAP, sh.BAD[1], sh.CAP, sh.CAP]


# ---- D ----------------------------------------------------------------------------------------------------
def test_packed(engine):
    want = run(engine, sh.packed())
    assert want[4]["n_bad"] > 500 and want[4]["payload"] == want[4]["bytes"]


# ---- E ----------------------------------------------------------------------------------------------------
def test_holes(engine):
    shape = sh.holes()
    want = run(engine, shape)
    assert want[4]["n_bad"] == int((shape.items[:, 0] < 0).sum()) == 66
    assert want[4]["bytes"] - want[4]["payload"] == int(shape.items[shape.items[:, 0] < 0, 1].sum()) > sh.S + sh.ROW


# ---- F, J -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [3, 1])
@pytest.mark.parametrize("total", sorted(sh.SMALL_PARTS))
def test_small_stage(engine, total, small):
    want = run(engine, sh.small_stage(total, small))
    assert not want[3].any()


@pytest.mark.parametrize("tail", [0, 1, 15, 16, 17])
def test_last_bytes(engine, tail):
    want = run(engine, sh.last_bytes(tail))
    assert not want[3].any()
    if tail:
        run(engine, sh.small_stage(5, 3, tail))                                  # under 16 bytes used, data_cap on both sides of 16
        run(engine, sh.small_stage(17, 1, tail))


# ---- G ----------------------------------------------------------------------------------------------------
def sizing(engine, shape):
    """Offsets only: every stage's data and the output NULL, 64 canary bytes of room."""
    n = shape.n
    stages = shape.stages()
    want = shape.fast(0, 64, stages)
    o = Out(n, 0, 64)
    types, conv = sh.type_bytes(n)
    dev = [(_dev(d), _offs(of), _dev(s)) for d, of, s, _ in stages]
    engine.rdbmerge(*dev, _dev(conv), _dev(types), *o.args(), o.tot[:4])
    torch.cuda.synchronize()
    o.compare(want)
    total = int(shape.items[:, 1].sum())
    assert (want[3] == sh.CAP).all() and want[4] == {"n_elems": 0, "bytes": total, "n_bad": n, "payload": 0}
    assert bool((o.data == CANARY).all())
    return total


def test_sizing_past_4gib_across_groups(engine):
    assert sizing(engine, sh.sizing_past_4gib()) > 1 << 44


def test_size_kernel_second_stride(engine):
    """More values than merge_size_kernel's grid has threads (16384 x 256)."""
    n = 16384 * 256 + 300
    assert sizing(engine, sh.sizing_past_4gib(n)) > 1 << 47


# ---- H ----------------------------------------------------------------------------------------------------
def test_one_call_packed_with_a_short_stage(engine):
    types, data, offs = sh.one_call_packed()
    full = la.expected_batch(types, data, offs, sh.OPTS)
    caps = (full[6][0], full[6][1] // 2, full[6][2])
    want = la.expected_batch(types, data, offs, sh.OPTS, stage_cap=caps)
    total = int(want[1][-1])
    assert ((want[3] == sh.CAP) & (full[3] == 0)).sum() > 300
    loadall(engine, types, data, offs, sh.OPTS, caps, total + 24, want)
    loadall(engine, types, data, offs, sh.OPTS, full[6], total, full)
