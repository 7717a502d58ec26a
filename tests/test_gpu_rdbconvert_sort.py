"""rr_rdbconvert_batch on the shapes of tests/rdbconvert_shapes.py, against tests/rdbconvert_reference.py
through test_gpu_rdbconvert's check / compare: every status, type, offset, blob byte and total, and the
canaries.  What the shapes are for: the order among negative scores (score_key), signed Set order and
the width from the extremes, duplicates across the dedup loop's 64-lane steps, integer-form member
text past byte 8 (Txt::hi), a wave's LDS slab taken over by its next value in both directions, a Hash
of 65534 entries, and a 5-byte prevlen on a ZSet's score entries.  tests/test_rdbconvert_shapes.py
holds the shapes and the reference to account on the CPU."""
import numpy as np
import pytest
import torch

import rdbconvert_reference as cv
import rdbconvert_shapes as sh
import rdbload_reference as ld
from test_gpu_rdbconvert import check, compare, loader_status, mixed, run_device

pytestmark = pytest.mark.gpu


def run_mixed(engine, vals, stays=(), host=False, claim=False):
    """The values between SKIP filler; their statuses are 0, but for `stays` (indices into vals).
    claim: the values are claimed RR_RDBLOAD_E_CONVERT, whatever the loader would say."""
    opts = vals[0][2]
    types, pays = mixed([(t, p) for t, p, _ in vals])
    load_status = None
    if claim:
        load_status = np.full(len(types), cv.E_CONVERT, np.uint8)
        load_status[0::2] = loader_status(types[0::2], pays[0::2], opts)
    st, tot = check(engine, types, pays, opts, host=host, load_status=load_status)
    assert (st[0::2] == cv.SKIP).all()
    assert st[1::2].tolist() == [cv.E_CONVERT if k in stays else 0 for k in range(len(vals))]
    assert tot["n_bad"] == len(stays)


def test_neg_score_zsets(engine):
    vals = sh.neg_score_zsets()
    run_mixed(engine, vals, stays=range(len(vals) - sh.NEG_STAYS, len(vals)))


def test_extreme_sets(engine):
    run_mixed(engine, sh.extreme_sets(), host=True)


def test_seam_duplicate_sets(engine):
    run_mixed(engine, sh.seam_duplicate_sets())


def test_long_int_members(engine):
    run_mixed(engine, sh.long_int_members(), host=True)


@pytest.mark.parametrize("swap", [False, True], ids=["big_then_small", "small_then_big"])
def test_lds_reuse_batch(engine, swap):
    vals = sh.lds_reuse_batch(swap)
    n = len(vals)
    types, opts = [t for t, _, _ in vals], vals[0][2]
    data, offsets = ld.pack([p for _, p, _ in vals])
    claim = np.full(n, cv.E_CONVERT, np.uint8)
    want = cv.convert_batch(types, data, offsets, claim, opts)
    room = int(want[1][-1]) + 64
    bufs = run_device(engine, types, data, offsets, claim, opts, room - 24, room)
    torch.cuda.synchronize()
    compare(bufs, n, want, room)
    stay = sh.REUSE_STAYS if swap else cv.MAX_WAVES + sh.REUSE_STAYS
    assert n > cv.MAX_WAVES and want[3].tolist() == [cv.E_CONVERT if k == stay else 0 for k in range(n)]


def test_hash_at_entry_cap(engine):
    run_mixed(engine, sh.hash_at_entry_cap(), stays=(2,), claim=True)


def test_zset_wide_prevlen(engine):
    run_mixed(engine, sh.zset_wide_prevlen())
