"""Diagnostics: time rr_rdbsave_batch (include/rr_rdbsave.h) beside rr_encode_batch on the same flat
batch, device-resident, HIP events: config batches decoded on the device, and a List-only batch.
Each figure is the call time (every launch of the call) over `steps` calls after a warm-up call,
three trials, fastest and slowest shown.  --lzf: the call again with RR_RDBSAVE_LZF, and its output
bytes as a fraction of the output without it.
Usage: python tools/time_rdbsave.py [--lzf] [configs, e.g. 2,3,4] [n] [steps] [n_lists] [entries per list]"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

LZF = "--lzf" in sys.argv
sys.argv = [a for a in sys.argv if a != "--lzf"]
cfgs = [int(c) for c in (sys.argv[1] if len(sys.argv) > 1 else "2,3,4").split(",")]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
n_lists = int(sys.argv[4]) if len(sys.argv) > 4 else 20_000
per_list = int(sys.argv[5]) if len(sys.argv) > 5 else 100
eng = rr.Engine(0)
eng.set_options(rr.CTX_NO_SMALL)
s = torch.cuda.current_stream()


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


def list_batch(count, per):
    """count List blobs of `per` entries: 8-24 byte words, every fourth a decimal integer."""
    rng = np.random.default_rng(0x115)
    blobs = []
    for _ in range(count):
        b = bytearray(bytes([rr.T_LIST_QUICKLIST]) + struct.pack("<I", 0))
        lens = rng.integers(8, 25, per)
        for k in range(per):
            e = str(int(rng.integers(-10**9, 10**9))).encode() if k % 4 == 0 else bytes(rng.integers(97, 123, int(lens[k]), dtype=np.uint8))
            b += struct.pack("<I", len(e)) + e
        blobs.append(bytes(b))
    offs = np.zeros(count + 1, np.uint64)
    offs[1:] = np.cumsum([len(b) for b in blobs])
    raw = b"".join(blobs)
    data = np.zeros((len(raw) + 15) & ~15, np.uint8)
    data[:len(raw)] = np.frombuffer(raw, np.uint8)
    return data, offs


def run(name, data, offs):
    nv, nb = len(offs) - 1, int(offs[-1])
    cap = rr.elem_bound(nv, nb)
    d_data = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_vals = torch.zeros(nv * 16, dtype=torch.uint8, device="cuda")
    d_elems = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
    d_arena = torch.zeros(d_data.numel(), dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=s)
    torch.cuda.synchronize()
    ne = int(d_tot[0].item())
    room = int(rr.lib().rr_rdbsave_bound(nv, ne, nb))
    out = torch.zeros(max(room, d_data.numel()) + 16, dtype=torch.uint8, device="cuda")
    o_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    o_ty = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    o_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    els = d_elems[:max(ne, 1) * 16]
    te = timed(lambda: eng.encode_device(d_vals, els, d_arena, out, o_off, d_tot, stream=s))
    eb = int(o_off[-1].item())
    tr = timed(lambda: eng.rdbsave_device(d_vals, els, d_arena, out, o_off, o_ty, o_st, d_tot, stream=s))
    rb, bad = int(o_off[-1].item()), int(d_tot[2].item())
    print(f"{name} n={nv} descriptors={ne} blob bytes={nb}")
    print(f"  rr_encode_batch   {te[0]:.3f}-{te[1]:.3f} ms  {nv / te[0] / 1e3:.2f} M values/s  {eb / te[0] / 1e6:.1f} GB/s out")
    print(f"  rr_rdbsave_batch  {tr[0]:.3f}-{tr[1]:.3f} ms  {nv / tr[0] / 1e3:.2f} M values/s  {rb / tr[0] / 1e6:.1f} GB/s out"
          f"  payload bytes={rb} bad={bad}  time vs encode x{tr[0] / te[0]:.2f}")
    if LZF:
        tz = timed(lambda: eng.rdbsave_device(d_vals, els, d_arena, out, o_off, o_ty, o_st, d_tot, stream=s, lzf=True))
        zb, zbad = int(o_off[-1].item()), int(d_tot[2].item())
        print(f"  ... with LZF      {tz[0]:.3f}-{tz[1]:.3f} ms  {nv / tz[0] / 1e3:.2f} M values/s  {zb / tz[0] / 1e6:.1f} GB/s out"
              f"  payload bytes={zb} bad={zbad}  output x{zb / rb:.3f} of flag off  time x{tz[0] / tr[0]:.2f} of flag off")


for cfg in cfgs:
    run(f"cfg={cfg}", *rr.gen_batch(cfg, n))
run(f"lists ({per_list} entries each)", *list_batch(n_lists, per_list))
