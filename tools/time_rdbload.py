"""Diagnostics: time rr_rdbload_batch (include/rr_rdbload.h) on the payloads rr_rdbsave_batch writes
for a config batch, flag off and with RR_RDBSAVE_LZF, beside rr_rdbsave_batch on the same batch;
device-resident, HIP events.  Each figure is the call time (every launch of the call) over `steps`
calls after a warm-up call, three trials, fastest and slowest shown.  The thresholds are the
defaults, so the status counts show how many values the defaults leave to the CPU path (CONVERT).
Usage: python tools/time_rdbload.py [configs, e.g. 2,3,4] [n] [steps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

cfgs = [int(c) for c in (sys.argv[1] if len(sys.argv) > 1 else "2,3,4").split(",")]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
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


def run(cfg):
    data, offs = rr.gen_batch(cfg, n)
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
    els = d_elems[:max(ne, 1) * 16]
    pay = torch.zeros(int(rr.lib().rr_rdbsave_bound(nv, ne, nb)) + 16, dtype=torch.uint8, device="cuda")
    p_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    p_ty = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    p_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    out = torch.zeros(nb + 64 * nv + 16, dtype=torch.uint8, device="cuda")   # blobs: never longer than the source blobs
    o_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    o_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    print(f"cfg={cfg} n={nv} descriptors={ne} blob bytes={nb}")
    for lzf in (False, True):
        save = lambda: eng.rdbsave_device(d_vals, els, d_arena, pay, p_off, p_ty, p_st, d_tot, stream=s, lzf=lzf)
        ts = timed(save)
        pb = int(p_off[-1].item())
        load = lambda: eng.rdbload(pay[:pb], p_off, p_ty, out, o_off, o_st, d_tot, stream=s)
        tl = timed(load)
        ob, bad = int(o_off[-1].item()), int(d_tot[2].item())
        st = np.bincount(o_st.cpu().numpy(), minlength=39)
        kinds = " ".join(f"{k}:{int(c)}" for k, c in enumerate(st) if c)
        print(f"  {'RR_RDBSAVE_LZF' if lzf else 'flag off      '} payload bytes={pb}")
        print(f"    rr_rdbsave_batch  {ts[0]:.3f}-{ts[1]:.3f} ms  {nv / ts[0] / 1e3:.2f} M values/s  {pb / ts[0] / 1e6:.1f} GB/s out")
        print(f"    rr_rdbload_batch  {tl[0]:.3f}-{tl[1]:.3f} ms  {nv / tl[0] / 1e3:.2f} M values/s  {pb / tl[0] / 1e6:.1f} GB/s in"
              f"  {ob / tl[0] / 1e6:.1f} GB/s out  blob bytes={ob} bad={bad} status {kinds}  time vs save x{tl[0] / ts[0]:.2f}")


for c in cfgs:
    run(c)
