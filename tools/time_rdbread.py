"""Diagnostics: time the read side of a complete RDB stream (include/rr_rdbread.h) on the section
tools/time_rdbfile.py builds for a config batch (rr_rdbsave_batch's payloads, keys of 16-40 bytes,
expiries on a quarter, head, EOF and checksum): the host index (rr_rdbread_index, one core, wall
clock), rr_rdbread_split and rr_rdbread_verify (device-resident, HIP events), beside the engine's
copy kernel over the same bytes (the ceiling a pass over those bytes has) and
rr_rdbdump_verify_batch on the same values as DUMP payloads.  Each device figure is the call time
(every launch of the call) over `steps` calls after a warm-up call, three trials, fastest and
slowest shown.  The results are checked: the split's payloads are the section's inputs, the verdict 0.
Usage: python tools/time_rdbread.py [configs, e.g. 2,3,4] [n] [steps]"""
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
    eng.rdbsave_device(d_vals, els, d_arena, pay, p_off, p_ty, p_st, d_tot, stream=s)
    torch.cuda.synchronize()
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
    out = torch.zeros(rr.rdbfile_bound(nv, kb, pb, head.numel()), dtype=torch.uint8, device="cuda")
    ro = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    rs = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    eng.rdbfile_section(pay[:pb], p_off, p_ty, p_st, keys, k_off, out, ro, rs, state, res, expires=expires, head=head,
                        flags=rr.RDBFILE_EOF, stream=s)
    torch.cuda.synchronize()
    sb = int(state[1].item())
    host = out[:sb].cpu().numpy()

    # the host index, one core
    t0 = time.perf_counter()
    ix = rr.rdbread_index(host, max_recs=nv, max_items=64)
    th = (time.perf_counter() - t0) * 1e3
    nr = len(ix["rec_start"])
    assert ix["rc"] == rr.RDBREAD_DONE and nr == int((rs == 0).sum().item())

    d_rs = torch.from_numpy(ix["rec_start"].view(np.int64).copy()).cuda()
    d_re = torch.from_numpy(ix["rec_end"].view(np.int64).copy()).cuda()
    kd = torch.zeros(kb + 16, dtype=torch.uint8, device="cuda")
    pd = torch.zeros(pb + 16, dtype=torch.uint8, device="cuda")
    ko = torch.zeros(nr + 1, dtype=torch.int64, device="cuda")
    po = torch.zeros(nr + 1, dtype=torch.int64, device="cuda")
    ty, st = torch.zeros(nr, dtype=torch.uint8, device="cuda"), torch.zeros(nr, dtype=torch.uint8, device="cuda")
    ex, idl = torch.zeros(nr, dtype=torch.int64, device="cuda"), torch.zeros(nr, dtype=torch.int64, device="cuda")
    fq = torch.zeros(nr, dtype=torch.int16, device="cuda")
    tsplit = timed(lambda: eng.rdbread_split(out[:sb], d_rs, d_re, 9, kd, ko, pd, po, ty, ex, idl, fq, st, res, stream=s))
    bad = int(res[8:16].cpu().numpy().view(np.uint64)[0])
    good = (p_st == 0)
    assert bad == 0 and int(po[-1].item()) == int((p_off[1:] - p_off[:-1])[good].sum().item())
    if nr == nv:
        assert torch.equal(pd[:pb], pay[:pb]) and torch.equal(kd[:kb], keys) and torch.equal(ex, expires)

    vstate = torch.zeros(2, dtype=torch.int64, device="cuda")

    def verify():   # (the checksum chains from call to call: the state is reset inside the timed call)
        vstate.zero_()
        eng.rdbread_verify(out[:sb], ix["eof_at"], vstate, res, stream=s)

    tver = timed(verify)
    assert int(res[16:20].cpu().numpy().view(np.uint32)[0]) == 0

    dump = torch.zeros(pb + 11 * nv + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    eng.rdbdump(pay[:pb], p_off, p_ty, p_st, dump, d_off, d_st, res, stream=s)
    torch.cuda.synchronize()
    db = int(d_off[-1].item())
    back = torch.zeros(pb + 16, dtype=torch.uint8, device="cuda")
    b_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    b_ty = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    b_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    tdv = timed(lambda: eng.rdbdump_verify(dump[:db], d_off, back, b_off, b_ty, b_st, res, stream=s))
    dst = torch.empty(sb, dtype=torch.uint8, device="cuda")
    tcopy = timed(lambda: eng.copy_device(dst, out, sb, stream=s))
    print(f"cfg={cfg} n={nv} records={nr} stream bytes={sb} payload bytes={pb} key bytes={kb} dump bytes={db}")
    print(f"    rr_rdbread_index, one core {th:.1f} ms  {sb / th / 1e6:.2f} GB/s  {nr / th / 1e3:.2f} M records/s")
    line("rr_rdbread_split", tsplit, sb, f" in  {nr / tsplit[0] / 1e3:.1f} M records/s")
    line("rr_rdbread_verify", tver, sb, " in")
    line("rr_rdbdump_verify_batch", tdv, db, f" in  {nv / tdv[0] / 1e3:.1f} M values/s")
    line("copy kernel, same bytes", tcopy, sb, " copied (read + write: twice that in traffic)")


for c in cfgs:
    run(c)
