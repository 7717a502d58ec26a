"""The GPU encoders on flat batches no decoder produced (tests/flat_forge.py), bit-exact against the
encode contract stated in plain Python (tests/encode_expect.py; tests/test_encode_contract.py
ties that statement to the C oracle and the host codec on the same batches): offsets, totals and
the bytes in [0, min(data_cap, offsets[n])).

Every forged value is legal input: rr_serdes.h promises that an unencodable value has size 0 and
that nothing outside the caller's descriptor array and arena is read.  The batches are the
smallest that reach the kernels' boundaries: 256-value E1 blocks, 16 KiB output windows, the
4,096-task map limit, the one-launch kernel's wave / lane routes and its 16 KiB input staging.
data_cap is always explicit (encode_bound sums raw len fields; a forged len is 2^32 - 1)."""
import ctypes as C

import numpy as np
import pytest

import redrock_old_amd as rr

import flat_forge as ff
from encode_expect import accepted_mask, expect_encode

pytestmark = pytest.mark.gpu

MUTATION_SEEDS = (101, 202, 303, 404)
SMALL_WAVE_N = 256          # at most this many values: the one-launch kernel puts a wave on each
SMALL_STAGE = 16 * 1024     # inputs up to this size are staged in LDS first


def small_fits(n, cap):
    f = rr.lib().rr_small_encode_fits
    f.argtypes = [C.c_uint64, C.c_uint64]
    return bool(f(n, cap))


def staged(v, e, a):
    return (len(v) + len(e) + (len(a) + 15) // 16) * 16 <= SMALL_STAGE


def check(eng, v, e, a, cap, what=""):
    xb, xo, xt = expect_encode(v, e, a, cap)
    ob, oo, ot = eng.encode_host(v, e, a, data_cap=cap)
    assert np.array_equal(oo, xo), f"{what} cap {cap}: offsets differ at {np.nonzero(oo != xo)[0][:5]}"
    assert ot == xt, f"{what} cap {cap}: totals {ot} != {xt}"
    k = min(cap, int(xo[-1]))
    assert len(ob) >= k
    if not np.array_equal(ob[:k], xb[:k]):
        at = int(np.nonzero(ob[:k] != xb[:k])[0][0])
        raise AssertionError(f"{what} cap {cap}: bytes differ first at {at} (value {int(np.searchsorted(xo, at, 'right')) - 1})")
    return ob, oo, ot


def caps_of(v, e, a):
    acc = accepted_mask(v, e, a)
    _, xo, xt = expect_encode(v, e, a, 1 << 62)
    return ff.cap_settings(xo, acc, xt["bytes"])


def both_routes(engine, engine_small, v, e, a, caps, what):
    """The one-launch kernel and the pipeline on the same batch: each equal to the contract (so to
    each other), at every cap the one-launch kernel takes."""
    for cap in caps:
        assert small_fits(len(v), cap), (what, len(v), cap)
        s = check(engine_small, v, e, a, cap, what + " small")
        p = check(engine, v, e, a, cap, what + " pipeline")
        assert np.array_equal(s[1], p[1]) and s[2] == p[2] and np.array_equal(s[0], p[0])


def _mutants(seed, n):
    v, e, a = ff.well_formed(seed, n)
    return ff.forge_mutations(v, e, a, seed)[:3]


# ---- the pipeline (E1 - E4) ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", MUTATION_SEEDS)
def test_pipeline_mutants(engine, seed):
    """6,000 values, ~40 % of them mutants the rule rejects, scattered: E1's lane and task-round
    costs, E3's window index over size-0 values, E4's walk; at the full cap, a cap at a rejected
    value, a cap at an accepted value's end and one byte before."""
    v, e, a = _mutants(seed, 6000)
    for cap in caps_of(v, e, a):
        assert cap <= 400 * 1024
        check(engine, v, e, a, cap, f"mutants {seed}")


@pytest.mark.parametrize("which", ["block", "first", "last"])
def test_pipeline_rejected_runs(engine, which):
    """A run of 320 rejected values across two E1 block edges; the first / the last value rejected."""
    v, e, a = ff.block_edge_run()[0] if which == "block" else ff.edges_rejected(which)
    for cap in caps_of(v, e, a):
        check(engine, v, e, a, cap, which)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_pipeline_window_edge_after_a_rejected_run(engine, delta):
    """300 size-0 values, then a value starting 1 byte before / at / 1 byte after the 16 KiB window
    edge: fv[1] must name it (or the value before the run, which holds byte 16383), never one of
    the run, and the window's walk must pass the whole run."""
    (v, e, a), (r0, r1), at = ff.window_edge_run(delta)
    for cap in caps_of(v, e, a) + [at, at + 1]:
        check(engine, v, e, a, cap, f"window edge {delta:+d}")


def test_pipeline_block_past_the_task_map(engine):
    """An E1 block of more than 4,096 tasks (the task search): the values past task 4,096 that hold
    one bad descriptor are rejected, their neighbours sized and written."""
    (v, e, a), bad = ff.big_task_block()
    caps = caps_of(v, e, a)
    ob, oo, ot = check(engine, v, e, a, caps[0], "big block")
    sizes = np.diff(oo.astype(np.int64))
    assert (sizes[bad] == 0).all() and ot["n_bad"] == len(bad)
    for cap in caps[1:]:
        check(engine, v, e, a, cap, "big block")


def test_pipeline_every_value_rejected(engine):
    v, e, a = ff.edges_rejected("all")
    for cap in (0, 16, 4096):
        ob, oo, ot = check(engine, v, e, a, cap, "all rejected")
        assert ot["bytes"] == 0 and ot["n_bad"] == len(v) and not oo.any()


@pytest.mark.parametrize("dense", [True, False], ids=["more_than_21_a_wave", "at_most_21_a_wave"])
def test_pipeline_decimal_lengths(engine, engine_small, dense):
    """List integers at every digit-count and bit-count edge (udigits' one table read) through
    E4's two decimal paths and the one-launch kernel: str(x) with a u32 length prefix."""
    (v, e, a), lists = ff.decimal_lists(dense)
    _, xo, xt = expect_encode(v, e, a, 1 << 62)
    assert xt["n_bad"] == 0
    both_routes(engine, engine_small, v, e, a, [xt["bytes"] + 16], "decimals")


@pytest.mark.parametrize("route", ["pipeline", "small"])
def test_device_entry_point(engine, engine_small, route):
    """rr_encode_batch with device-resident inputs whose elem_cap and arena_cap are the arrays'
    true lengths (no slack behind them for a missing guard to land in)."""
    import torch
    dev = torch.device("cuda:0")
    eng = engine if route == "pipeline" else engine_small
    v, e, a = _mutants(505, 1200)
    _, xo0, xt0 = expect_encode(v, e, a, 1 << 62)
    cap = (xt0["bytes"] // 2) & ~15          # (cuts the batch too)
    assert small_fits(len(v), cap)
    xb, xo, xt = expect_encode(v, e, a, cap)
    d_v = torch.from_numpy(v.view(np.uint8).copy()).to(dev)
    d_e = torch.from_numpy(e.view(np.uint8).copy()).to(dev)
    d_a = torch.from_numpy(a.copy()).to(dev)
    assert d_e.numel() == 16 * len(e) and d_a.numel() == len(a)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_oo = torch.zeros(len(v) + 1, dtype=torch.int64, device=dev)
    d_t = torch.full((4,), -1, dtype=torch.int64, device=dev)
    eng.encode_device(d_v, d_e, d_a, d_out, d_oo, d_t)
    torch.cuda.synchronize()
    assert np.array_equal(d_oo.cpu().numpy().view(np.uint64), xo)
    t = d_t.cpu().numpy().view(np.uint64)
    assert {"n_elems": int(t[0]), "bytes": int(t[1]), "n_bad": int(t[2]), "payload": int(t[3])} == xt
    k = min(cap, xt["bytes"])
    assert np.array_equal(d_out.cpu().numpy()[:k], xb[:k])


# ---- the one-launch kernel (encode_small_kernel) ---------------------------------------------
@pytest.mark.parametrize("n,stage", [(1, "staged"), (32, "staged"), (33, "staged"), (1, "unstaged"), (32, "unstaged"),
                                     (33, "unstaged"), (SMALL_WAVE_N, "unstaged"), (SMALL_WAVE_N + 1, "unstaged")])
def test_small_route_boundaries(engine, engine_small, n, stage):
    """A wave per value up to 256 values, a lane per value past that; inputs staged in LDS when
    they fit 16 KiB or read in place.  The batches are n consecutive values of a mutated batch
    with its descriptor array and arena whole (a 64-value batch fits the staging, a 1,500-value
    one does not); for n = 1 every one of the first values takes its turn alone."""
    v, e, a = _mutants(600, 64) if stage == "staged" else _mutants(606, 1500)
    starts = range(0, 40) if n == 1 else (0, len(v) - n, (len(v) - n) // 2)
    seen = set()
    for s in starts:
        w = v[s:s + n]
        assert staged(w, e, a) == (stage == "staged")
        both_routes(engine, engine_small, w, e, a, caps_of(w, e, a), f"n={n} {stage} from {s}")
        seen |= set(accepted_mask(w, e, a))
    assert seen == {True, False}


def test_small_4096_tiny_values(engine, engine_small):
    v, e, a = _mutants(707, rr.SMALL_N)
    caps = caps_of(v, e, a)
    assert caps[0] <= rr.SMALL_BYTES
    both_routes(engine, engine_small, v, e, a, caps, "4096 tiny")


@pytest.mark.parametrize("seed", MUTATION_SEEDS)
def test_small_mutants(engine, engine_small, seed):
    v, e, a = _mutants(seed, 1500)
    both_routes(engine, engine_small, v, e, a, caps_of(v, e, a), f"small mutants {seed}")


@pytest.mark.parametrize("which", ["block", "window-1", "window+0", "window+1", "first", "last", "all"])
def test_small_placements(engine, engine_small, which):
    """The rejected runs and edges of the pipeline tests through the one-launch kernel (its scan
    and capacity cut see the same size-0 values), and the two routes equal."""
    if which == "block":
        v, e, a = ff.block_edge_run()[0]
    elif which.startswith("window"):
        v, e, a = ff.window_edge_run(int(which[6:]))[0]
    else:
        v, e, a = ff.edges_rejected(which)
    both_routes(engine, engine_small, v, e, a, caps_of(v, e, a), which)
