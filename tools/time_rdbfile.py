"""Diagnostics: time rr_rdbfile_section (include/rr_rdbfile.h) and its CRC pass alone
(rr_crc64_device over the section's bytes), rr_rdbdump_batch and rr_rdbdump_verify_batch on the
payloads rr_rdbsave_batch writes for a config batch, beside rr_rdbsave_batch on the same batch, the
engine's copy kernel over the section's bytes (the ceiling a pass over those bytes has) and one host
core's rr_crc64 over the same section; device-resident, HIP events.  Each figure is the call time
(every launch of the call) over `steps` calls after a warm-up call, three trials, fastest and
slowest shown.  Keys are 16-40 bytes from a seeded generator.
Usage: python tools/time_rdbfile.py [configs, e.g. 2,3,4] [n] [steps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

cfgs = [int(c) for c in (sys.argv[1] if len(sys.argv) > 1 else "2,3,4").split(",")]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
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


def line(name, t, nbytes, extra=""):
    print(f"    {name:<26}{t[0]:.3f}-{t[1]:.3f} ms  {nbytes / t[0] / 1e6:.1f} GB/s{extra}")


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
    save = lambda: eng.rdbsave_device(d_vals, els, d_arena, pay, p_off, p_ty, p_st, d_tot, stream=s)
    ts = timed(save)
    pb = int(p_off[-1].item())
    rng = np.random.default_rng(1000 + cfg)
    klen = rng.integers(16, 41, nv)
    koffs = np.zeros(nv + 1, np.int64)
    np.cumsum(klen, out=koffs[1:])
    kb = int(koffs[-1])
    keys = torch.from_numpy(rng.integers(33, 127, kb, dtype=np.uint8)).cuda()
    k_off = torch.from_numpy(koffs).cuda()
    expires = torch.from_numpy(np.where(rng.integers(0, 4, nv) == 0, 1_700_000_000_000 + rng.integers(0, 1 << 30, nv), -1)).cuda()
    _, hd = rr.rdbfile_head("6.0.20", 1700000000, 1 << 33, (0, "a" * 40, 1))
    sd_need, sd = rr.rdbfile_selectdb(0, nv, nv // 4)
    head = torch.from_numpy(np.frombuffer(hd + sd[:sd_need], np.uint8).copy()).cuda()
    scap = rr.rdbfile_bound(nv, kb, pb, head.numel())
    out = torch.zeros(scap, dtype=torch.uint8, device="cuda")
    ro = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    rs = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    res = torch.zeros(24, dtype=torch.uint8, device="cuda")

    def section():   # (the checksum chains from call to call: the state is reset outside the timed calls)
        eng.rdbfile_section(pay[:pb], p_off, p_ty, p_st, keys, k_off, out, ro, rs, state, res, expires=expires, head=head,
                            flags=rr.RDBFILE_EOF, stream=s)

    tsec = timed(section)
    state.zero_()
    section()
    torch.cuda.synchronize()
    sb = int(state[1].item())
    crc_dev = int(state.cpu().numpy().view(np.uint64)[0])
    tcrc = timed(lambda: eng.crc64_device(out, sb - 8, state, stream=s))
    dump = torch.zeros(pb + 11 * nv + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    tdump = timed(lambda: eng.rdbdump(pay[:pb], p_off, p_ty, p_st, dump, d_off, d_st, res, stream=s))
    db, dbad = int(d_off[-1].item()), int(res[8:16].cpu().numpy().view(np.uint64)[0])
    back = torch.zeros(pb + 16, dtype=torch.uint8, device="cuda")
    b_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    b_ty = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    b_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    tver = timed(lambda: eng.rdbdump_verify(dump[:db], d_off, back, b_off, b_ty, b_st, res, stream=s))
    vbad = int(res[8:16].cpu().numpy().view(np.uint64)[0])
    dst = torch.empty(sb, dtype=torch.uint8, device="cuda")
    tcopy = timed(lambda: eng.copy_device(dst, out, sb, stream=s))
    host = out[:sb].cpu().numpy()
    t0 = time.perf_counter()
    crc_host = rr.crc64(0, host[:sb - 8])
    th = (time.perf_counter() - t0) * 1e3
    assert crc_host == crc_dev == int(host[sb - 8:].view(np.uint64)[0]), (hex(crc_host), hex(crc_dev))
    assert torch.equal(back[:pb], pay[:pb]) and dbad == vbad
    print(f"cfg={cfg} n={nv} payload bytes={pb} key bytes={kb} section bytes={sb} dump bytes={db} unsaveable={dbad}")
    line("rr_rdbsave_batch", ts, pb, " out")
    line("rr_rdbfile_section", tsec, sb, f" out  time vs save x{tsec[0] / ts[0]:.2f}")
    line("  its CRC pass alone", tcrc, sb - 8, f" in  {th / tcrc[0]:.0f}x one host core")
    line("rr_rdbdump_batch", tdump, db, " out")
    line("rr_rdbdump_verify_batch", tver, db, " in")
    line("copy kernel, same bytes", tcopy, sb, " copied (read + write: twice that in traffic)")
    print(f"    one host core rr_crc64    {th:.1f} ms  {(sb - 8) / th / 1e6:.2f} GB/s")


for c in cfgs:
    run(c)
