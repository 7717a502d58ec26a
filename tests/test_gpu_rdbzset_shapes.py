"""rr_d2string_batch and rr_rdbzset_batch on the shapes of tests/rdbzset_shapes.py, byte-exact against
tests/rdbzset_reference.py through test_gpu_rdbzset's expect_texts / run_device / compare / check, canaries
behind every written buffer.  What the shapes are for: the device compile of the printer on every
exponent with full mantissas, on the range where the notation and ll2string's window switch and on
random bits; d2string_kernel's second round (the grid is capped, so a wave comes back for more scores:
its states and slots used again, and the slot limit of a partial round); a lane's sequence of prints
inside one ZSet; printed scores at every ziplist integer encoding's edge and in a wave's last text
slot; and a wave of rdbzset_size_kernel and rdbzset_emit_kernel taking a second value, big then small
and small then big, with the totals it adds up over both.  tests/test_rdbzset_shapes.py holds the
shapes and the yardstick to account on the CPU."""
import numpy as np
import pytest
import torch

import redrock_old_amd as rr

import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbzset_reference as zr
import rdbzset_shapes as sh
from test_gpu_rdbzset import CANARY, check, compare, expect_texts, run_device
from test_rdbzset import ZSET

pytestmark = pytest.mark.gpu


# ---- rr_d2string_batch ------------------------------------------------------------------------------------
def first_bad(bits, text, ln, want, wlen):
    """None, or the first pattern whose length or slot differs: (index, bits in hex, got, want)."""
    bad = np.nonzero((ln != wlen) | (text != want).any(axis=1))[0]
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return i, hex(int(bits[i])), text[i].tobytes(), want[i].tobytes()


def host_entry(engine, bits):
    want, wlen = expect_texts(bits)
    text, ln = engine.d2string_host(bits, fill=CANARY)
    assert text.shape == want.shape and first_bad(bits, text, ln, want, wlen) is None, first_bad(bits, text, ln, want, wlen)


def test_d2string_stratified(engine):
    host_entry(engine, sh.stratified_bits())


def test_d2string_window(engine):
    host_entry(engine, sh.window_bits())


def test_d2string_random(engine):
    host_entry(engine, sh.random_bits())


def test_d2string_round_two(engine):
    """N2 scores through the device entry: wave 0 of workgroup 0 prints a second round of 64, wave 1 a
    second round of one.  The expected slots are one fancy index of the table's."""
    table = sh.round_two_table()
    n = sh.N2
    idx = np.arange(n) % sh.T
    tab_text, tab_len = expect_texts(table)
    d_bits = torch.from_numpy(table[idx].view(np.int64)).cuda()
    d_text = torch.full((32 * n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_len = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    engine.d2string(d_bits, d_text[:32 * n], d_len[:n])
    torch.cuda.synchronize()
    text, ln = d_text.cpu().numpy(), d_len.cpu().numpy()
    assert (ln[n:] == CANARY).all() and (text[32 * n:] == CANARY).all()
    text, ln = text[:32 * n].reshape(n, 32), ln[:n]
    want, wlen = tab_text[idx], tab_len[idx]
    if not (np.array_equal(ln, wlen) and np.array_equal(text, want)):
        i, b, got, exp = first_bad(table[idx], text, ln, want, wlen)
        raise AssertionError(f"score {i} (round {i // sh.D2S_ROUND}, lane {i % 64}) {b}: got {got} len {ln[i]}, want {exp}")


# ---- rr_rdbzset_batch -------------------------------------------------------------------------------------
def within_bound(offsets, n, data_len):
    assert int(offsets[n]) <= rr.rdbzset_bound(n, data_len)


def run_attempted(engine, vals):
    """A list whose every value the second stage leaves: check() with the statuses of a real rr_rdbload_batch
    and rr_rdbconvert_batch chain, device and host entry; every value converts."""
    pays, opts = [p for p, _ in vals], vals[0][1]
    conv, st, tot = check(engine, [ZSET] * len(pays), pays, opts, host=True)
    assert (conv == zr.E_CONVERT).all() and (st == 0).all() and tot["n_bad"] == 0
    assert tot["n_elems"] == sum(zr.zset_blob(p, opts)[3] for p in pays)
    assert tot["bytes"] <= rr.rdbzset_bound(len(pays), sum(len(p) for p in pays))


def test_lane_sequence_zsets(engine):
    run_attempted(engine, sh.lane_sequence_zsets())


def test_int_text_zsets(engine):
    run_attempted(engine, sh.int_text_zsets())


@pytest.mark.parametrize("swap", [False, True], ids=["big_then_small", "small_then_big"])
def test_wave_reuse_batch(engine, swap):
    """MAX_WAVES + 7 values: every wave of the first seven's converts a second value.  The totals are sums a
    wave keeps over its values before its atomics."""
    vals = sh.wave_reuse_batch(swap)
    n = len(vals)
    opts = vals[0][1]
    types = [ZSET] * n
    data, offsets = ld.pack([p for p, _ in vals])
    claim = np.full(n, zr.E_CONVERT, np.uint8)
    want = zr.zset_batch(types, data, offsets, claim, opts)
    room = int(want[1][-1]) + 64
    bufs = run_device(engine, types, data, offsets, claim, opts, room - 24, room)
    torch.cuda.synchronize()
    compare(bufs, n, want, room)                                              # offsets, statuses, totals, bytes, canaries
    stay = n - 7 + sh.REUSE_STAYS if swap else sh.REUSE_STAYS
    assert n > cv.MAX_WAVES and want[2].tolist() == [zr.E_CONVERT if k == stay else 0 for k in range(n)]
    assert want[3]["n_bad"] == 1 and want[3]["payload"] == int(want[1][-1]) - 13 * (n - 1)
    assert want[3]["n_elems"] == sum(zr.zset_blob(p, opts)[3] for p, _ in vals[:7] + vals[-7:]) + sum(p[0] for p, _ in vals[7:-7])
    within_bound(want[1], n, len(data))
