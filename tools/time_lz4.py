"""Diagnostics: time the GPU LZ4 block compression (include/rr_lz4.h) beside the snappy one on
config batches cut into 16 KiB RocksDB data blocks, device-resident, HIP events, both directions;
and pyarrow's lz4_raw on `threads` host threads for comparison.  Each figure is the call time
(every launch of the call) over `steps` calls after a warm-up call, three trials, fastest and
slowest shown.
Usage: python tools/time_lz4.py [configs, e.g. 2,3,4] [n] [steps] [block] [threads]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

cfgs = [int(c) for c in (sys.argv[1] if len(sys.argv) > 1 else "2,3,4").split(",")]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
bs = int(sys.argv[4]) if len(sys.argv) > 4 else 16384
threads = int(sys.argv[5]) if len(sys.argv) > 5 else 16
eng = rr.Engine(0)
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


for cfg in cfgs:
    data, offs = rr.gen_batch(cfg, n)
    nb = int(offs[-1])
    cuts = np.append(np.arange(0, nb, bs, dtype=np.uint64), np.uint64(nb))
    nblk = len(cuts) - 1
    d_data = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(cuts.view(np.int64)).cuda()
    L = rr.lib()
    cap = max(int(L.rr_snappy_compress_bound(nblk, d_data.numel())), int(L.rr_lz4_compress_bound(nblk, d_data.numel())))
    d_comp = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_coffs = torch.zeros(nblk + 1, dtype=torch.int64, device="cuda")
    d_back = torch.zeros(d_data.numel(), dtype=torch.uint8, device="cuda")
    d_boffs = torch.zeros(nblk + 1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(nblk, dtype=torch.uint8, device="cuda")
    print(f"cfg={cfg} n={n} blocks={nblk}x{bs} bytes={nb}")
    for name, comp, dec in (("snappy", eng.snappy_compress_device, eng.snappy_decompress_device),
                            ("lz4", eng.lz4_compress_device, eng.lz4_decompress_device)):
        tc = timed(lambda: comp(d_data, d_offs, d_comp, d_coffs, stream=s))
        zb = int(d_coffs[-1].item())
        d_back.zero_()
        td = timed(lambda: dec(d_comp[:((zb + 15) & ~15) or 16], d_coffs, d_back, d_boffs, d_st, stream=s))
        ok = int(d_st.max().item()) == 0 and torch.equal(d_back[:nb], d_data[:nb])
        print(f"  {name:6s} compressed={zb} ({zb / nb:.3f} of input) roundtrip={ok}")
        print(f"  {name:6s} compress   {tc[0]:.3f}-{tc[1]:.3f} ms  {nb / tc[0] / 1e6:.1f} GB/s of input")
        print(f"  {name:6s} decompress {td[0]:.3f}-{td[1]:.3f} ms  {nb / td[0] / 1e6:.1f} GB/s of output")
    if threads:
        import pyarrow as pa
        codec = pa.Codec("lz4_raw")
        sub = [data[int(cuts[i]):int(cuts[i + 1])].tobytes() for i in range(min(nblk, 4000))]
        sb = sum(len(b) for b in sub)
        with ThreadPoolExecutor(threads) as ex:
            t0 = time.perf_counter()
            z = list(ex.map(lambda b: codec.compress(b, asbytes=True), sub, chunksize=64))
            t1 = time.perf_counter()
            list(ex.map(lambda p: codec.decompress(p[0], decompressed_size=len(p[1]), asbytes=True), zip(z, sub), chunksize=64))
            t2 = time.perf_counter()
        zs = sum(len(b) for b in z)
        print(f"  pyarrow lz4_raw {threads} thr: compressed={zs / sb:.3f} of input, compress {sb / (t1 - t0) / 1e9:.2f} GB/s, "
              f"decompress {sb / (t2 - t1) / 1e9:.2f} GB/s (first {len(sub)} blocks)")
