"""Diagnostics: time rr_rdbzset_batch (include/rr_rdbzset.h) and rr_d2string_batch (include/rr_d2string.h);
device-resident, HIP events.  Each figure is the call time (every launch of the call) over `steps` calls
after a warm-up call, three trials, fastest and slowest shown.
  zsets    ZSets of 32 members (8-letter members) with fractional scores through rr_rdbzset_batch, beside
           rr_rdbconvert_batch on the same ZSets with the scores truncated to integers: the ratio is the
           cost of printing over not printing
  scores   rr_d2string_batch on scores of one class at a time: small fractions, values near DBL_MAX (the
           longest division loops), subnormals (the longest multiplication loops), and integers in
           ll2string's window (no multi-word arithmetic at all)
Usage: python tools/time_rdbzset.py [zsets|scores|all] [n zsets] [n scores] [steps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
n_zsets = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
n_scores = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
eng = rr.Engine(0)
eng.set_options(rr.CTX_NO_SMALL)
s = torch.cuda.current_stream()
rng = np.random.default_rng(7)
E_CONVERT = rr.RDBLOAD_E_CONVERT


def timed(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(steps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return min(out), max(out)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def dev_offs(o):
    return torch.from_numpy(np.ascontiguousarray(o, np.uint64).view(np.int64).copy()).cuda()


def zset_batch(n, scores, m=32):
    """n ZSET_2 payloads of m members: count | (8 | 8 letters | 8 score bytes) x m."""
    rec = np.empty((n, m, 17), np.uint8)
    rec[:, :, 0] = 8
    rec[:, :, 1:9] = rng.integers(97, 123, (n, m, 8), dtype=np.uint8)
    rec[:, :, 9:] = scores.astype(np.float64).view(np.uint8).reshape(n, m, 8)
    data = np.concatenate([np.full((n, 1), m, np.uint8), rec.reshape(n, -1)], axis=1)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(data.shape[1])
    return np.ascontiguousarray(data).reshape(-1), offs


def zsets():
    n = n_zsets
    frac = rng.integers(0, 1_000_000, (n, 32)) / 1000.0 + 0.0005          # rankings, timestamps with a fraction
    d_types = torch.full((n,), rr.T_ZSET_SKIPLIST, dtype=torch.uint8, device="cuda")
    claim = torch.full((n,), E_CONVERT, dtype=torch.uint8, device="cuda")
    o_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    o_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    o_ty = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    res = {}
    for name, sc in (("fractional", frac), ("truncated", np.floor(frac))):
        data, offs = zset_batch(n, sc)
        nb = int(offs[-1])
        d_data, d_offs = dev(data), dev_offs(offs)
        out = torch.zeros(rr.rdbzset_bound(n, nb) + 16, dtype=torch.uint8, device="cuda")
        if name == "fractional":
            eng.rdbconvert(d_data, d_offs, d_types, claim, out, o_off, o_ty, o_st, d_tot, stream=s)
            torch.cuda.synchronize()
            assert int((o_st == E_CONVERT).sum().item()) == n, "the second stage leaves every fractional ZSet"
            conv = o_st.clone()
            t = timed(lambda: eng.rdbzset(d_data, d_offs, d_types, conv, out, o_off, o_st, d_tot, stream=s))
            call = "rr_rdbzset_batch   "
        else:
            t = timed(lambda: eng.rdbconvert(d_data, d_offs, d_types, claim, out, o_off, o_ty, o_st, d_tot, stream=s))
            call = "rr_rdbconvert_batch"
        assert int(d_tot[2].item()) == 0 and int((o_st == 0).sum().item()) == n, "every value converts"
        res[name] = t
        print(f"ZSets of 32, {name} scores: n={n} payload bytes={nb} blob bytes={int(o_off[-1].item())}")
        print(f"  {call}  {t[0]:.3f}-{t[1]:.3f} ms  {n / t[0] / 1e3:.2f} M values/s  {32 * n / t[0] / 1e3:.1f} M scores/s")
    print(f"  printing / not printing x{res['fractional'][0] / res['truncated'][0]:.2f}")


def scores():
    n = n_scores
    classes = (("small fractions", rng.integers(0, 1_000_000, n) / 1000.0 + 0.0005),
               ("near DBL_MAX", 1.7976931348623157e308 * (1.0 - rng.random(n) / 2)),
               ("subnormals", (rng.integers(1, 1 << 52, n, dtype=np.uint64)).view(np.float64)),
               ("integers below 2^52", rng.integers(0, 1 << 40, n).astype(np.float64)))
    text = torch.zeros(rr.D2STRING_SLOT * n, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for name, v in classes:
        bits = torch.from_numpy(np.ascontiguousarray(v, np.float64).view(np.int64).copy()).cuda()
        t = timed(lambda: eng.d2string(bits, text, ln, stream=s))
        got = bytes(text[:32].cpu().numpy()[:int(ln[0].item())])
        assert got == rr.d2string(float(v[0])), (got, rr.d2string(float(v[0])))
        print(f"rr_d2string_batch, {name}: n={n}  {t[0]:.3f}-{t[1]:.3f} ms  {n / t[0] / 1e3:.1f} M scores/s"
              f"  mean text {float(ln.float().mean().item()):.1f} bytes  e.g. {got.decode()}")


if what in ("zsets", "all"):
    zsets()
if what in ("scores", "all"):
    scores()
