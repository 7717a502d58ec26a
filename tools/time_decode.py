"""Diagnostics: time rr_decode_batch (device-resident, HIP events) on a config batch.
Usage: [RR_LIB=...] [RR_DECODE_MODE=k] python tools/time_decode.py [--zl-raw] [config] [n] [steps]
--zl-raw: the context keeps ziplists raw (RR_CTX_ZL_RAW; the default is the strict walk)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

zl_raw = "--zl-raw" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != "--zl-raw"]
cfg = int(args[0]) if len(args) > 0 else 4
n = int(args[1]) if len(args) > 1 else 1_000_000
steps = int(args[2]) if len(args) > 2 else 10
data, offs = rr.gen_batch(cfg, n)
nb = int(offs[-1])
dev = torch.device("cuda:0")
eng = rr.Engine(0)
eng.reserve(n, nb)
if zl_raw:
    eng.set_options(rr.CTX_ZL_RAW)
d_data = torch.from_numpy(data).to(dev)
d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
cap = rr.elem_bound(n, nb)
d_vals = torch.empty(n * 16, dtype=torch.uint8, device=dev)
d_elems = torch.empty(cap * 16, dtype=torch.uint8, device=dev)
d_arena = torch.empty((nb + 15) & ~15, dtype=torch.uint8, device=dev)
d_tot = torch.zeros(4, dtype=torch.int64, device=dev)
s = torch.cuda.current_stream()
for _ in range(3):
    eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=s)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(s)
for _ in range(steps):
    eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=s)
e1.record(s)
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / steps
print(f"cfg={cfg} n={n} bytes={nb} mode={os.environ.get('RR_DECODE_MODE', '0')} lib={os.environ.get('RR_LIB', 'librr_serdes.so')}"
      f" zl={'raw' if zl_raw else 'strict'} ms={ms:.4f} GiB/s={nb / ms / 1e-3 / 2**30:.1f}")
