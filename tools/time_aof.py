"""Diagnostics: time rr_aof_batch (include/rr_aof.h) on a mixed batch; device-resident, HIP events.  Each
figure is the call time (every launch of the call) over `steps` calls after a warm-up call, three trials,
fastest and slowest shown.  Beside it: rr_rdbsave_batch on the same flat batch (the BGSAVE half of the
same row), and the CPU restatement tests/aof_reference.py on the first `sample` values (Python: a floor
for what a per-key CPU path costs, not the reference's C).  Reported numbers, not pass criteria.
Usage: python tools/time_aof.py [n values] [steps] [sample] [output file]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402
import aof_reference as ar  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sample = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000
dest = sys.argv[4] if len(sys.argv) > 4 else None
eng = rr.Engine(0)
eng.set_options(rr.CTX_NO_SMALL)
s = torch.cuda.current_stream()
lines = []


def say(x):
    print(x)
    lines.append(x)


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


data, offs = rr.gen_batch(rr.CONFIG_MIXED, n)
values, elems, arena, tot = rr.host_decode(data, offs)
assert tot["n_bad"] == 0
names = [b"key:%d" % i for i in range(n)]
kd, ko = ar.keys_of(names)
exp = np.where(np.arange(n) % 4 == 0, 1700000000000 + np.arange(n), -1).astype(np.int64)
d_v, d_e, d_a, d_kd = dev(values), dev(elems), dev(arena), dev(kd)
d_ko = torch.from_numpy(ko.view(np.int64).copy()).cuda()
d_exp = torch.from_numpy(exp).cuda()
o_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
o_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
o_ty = torch.zeros(n, dtype=torch.uint8, device="cuda")
d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
eng.aof(d_v, d_e, d_a, d_kd, d_ko, empty, o_off, o_st, d_tot, expires=d_exp, stream=s)   # sizes first
torch.cuda.synchronize()
total = int(o_off[-1].item())
out = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
t_aof = timed(lambda: eng.aof(d_v, d_e, d_a, d_kd, d_ko, out, o_off, o_st, d_tot, expires=d_exp, stream=s))
assert int(d_tot[2].item()) == 0 and int(d_tot[1].item()) == total
rout = torch.zeros(rr.rdbsave_bound(values, elems), dtype=torch.uint8, device="cuda")
t_rdb = timed(lambda: eng.rdbsave_device(d_v, d_e, d_a, rout, o_off, o_ty, o_st, d_tot, stream=s))
rbytes = int(d_tot[1].item())

m = min(sample, n)
t0 = time.perf_counter()
want = ar.aof_batch(values[:m], elems, arena, *ar.keys_of(names[:m]), exp[:m])
t_cpu = time.perf_counter() - t0
got = out[:int(want[1][-1])].cpu().numpy()
assert np.array_equal(got, want[0]), "the GPU's bytes differ from the restatement's"

say(f"mixed batch (config 4): n={n} blob bytes={int(offs[-1])} descriptors={tot['n_elems']} key bytes={len(kd)} "
    f"expiries={int((exp != -1).sum())}")
say(f"  rr_aof_batch      {t_aof[0]:.3f}-{t_aof[1]:.3f} ms  {n / t_aof[0] / 1e3:.2f} M values/s  "
    f"{total / t_aof[0] / 1e6:.1f} GB/s of commands ({total} bytes)")
say(f"  rr_rdbsave_batch  {t_rdb[0]:.3f}-{t_rdb[1]:.3f} ms  {n / t_rdb[0] / 1e3:.2f} M values/s  "
    f"{rbytes / t_rdb[0] / 1e6:.1f} GB/s of payloads ({rbytes} bytes)")
say(f"  aof / rdbsave     x{t_aof[0] / t_rdb[0]:.2f} in time, x{total / rbytes:.2f} in bytes")
say(f"  CPU restatement (Python, first {m} values, checked equal): {t_cpu * 1e3:.1f} ms  {m / t_cpu / 1e6:.3f} M values/s")
if dest:
    with open(dest, "a") as f:
        f.write("\n".join(lines) + "\n")
