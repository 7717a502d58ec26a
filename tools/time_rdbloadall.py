"""Diagnostics: time rr_rdbmerge_batch and rr_rdbloadall_batch (include/rr_rdbloadall.h); device-resident, HIP
events.  Each figure is the time of the calls named over `steps` rounds after a warm-up round, three trials,
fastest and slowest shown.  The batch is a config batch as rr_rdbsave_batch writes it, with Hashes of 8 pairs
(rr_rdbconvert_batch's scenario) behind it so that the share named comes from stage 2.
  merge    rr_rdbmerge_batch alone over the three stages' batches, beside the engine's copy kernel over the
           same output bytes
  route    rr_rdbloadall_batch + one rr_decode_batch against the three stage calls + three rr_decode_batch
           calls over n
  stages   the three stage calls one by one (run it under RR_LIB=<another build> for an A/B)
Usage: python tools/time_rdbloadall.py [merge|route|stages|all] [n] [steps] [shares, e.g. 0,1,50]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
n_cfg = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
shares = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "0,1,50").split(",")]
eng = rr.Engine(0)
eng.set_options(rr.CTX_NO_SMALL)
s = torch.cuda.current_stream()
rng = np.random.default_rng(7)
z8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")
z64 = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")


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


def ms(t):
    return f"{t[0]:.3f}-{t[1]:.3f} ms"


def hashes(n):
    """n Hashes of 8 pairs, 8-letter fields and values: (data, offsets)."""
    rec = np.empty((n, 16, 9), np.uint8)
    rec[:, :, 0] = 8
    rec[:, :, 1:] = rng.integers(97, 123, (n, 16, 8), dtype=np.uint8)
    data = np.concatenate([np.full((n, 1), 8, np.uint8), rec.reshape(n, -1)], axis=1)
    return np.ascontiguousarray(data).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(data.shape[1])


def saved_config(cfg=4):
    """The config batch as rr_rdbsave_batch writes it, on the device: (payloads, offsets, types, n, bytes)."""
    data, offs = rr.gen_batch(cfg, n_cfg)
    nv, nb = len(offs) - 1, int(offs[-1])
    cap = rr.elem_bound(nv, nb)
    d_data, d_offs = torch.from_numpy(data).cuda(), torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_vals, d_elems, d_arena, d_tot = z8(nv * 16), z8(cap * 16), z8(d_data.numel()), z64(4)
    eng.decode_device(d_data, d_offs, d_vals, d_elems, d_arena, d_tot, stream=s)
    torch.cuda.synchronize()
    ne = int(d_tot[0].item())
    pay = z8(int(rr.lib().rr_rdbsave_bound(nv, ne, nb)) + 16)
    p_off, p_ty, p_st = z64(nv + 1), z8(nv), z8(nv)
    eng.rdbsave_device(d_vals, d_elems[:max(ne, 1) * 16], d_arena, pay, p_off, p_ty, p_st, d_tot, stream=s)
    torch.cuda.synchronize()
    pb = int(p_off[-1].item())
    return pay[:pb].clone(), p_off, p_ty, nv, pb


def with_share(base, share):
    pay, p_off, p_ty, nv, pb = base
    extra = nv * share // (100 - share) if share else 0
    if extra:
        hdata, hoffs = hashes(extra)
        pay = torch.cat([pay, torch.from_numpy(hdata).cuda()])
        p_off = torch.cat([p_off[:nv], torch.from_numpy((hoffs + np.uint64(pb)).view(np.int64).copy()).cuda()])
        p_ty = torch.cat([p_ty, torch.full((extra,), rr.T_HASH_HT, dtype=torch.uint8, device="cuda")])
        nv, pb = nv + extra, pb + len(hdata)
    return pay, p_off, p_ty, nv, pb


def scenario(base, share):
    pay, p_off, p_ty, nv, pb = with_share(base, share)
    caps = (rr.rdbload_bound(nv, pb), rr.rdbconvert_bound(nv, pb), rr.rdbzset_bound(nv, pb))   # rr_rdbloadall_caps
    st = [(z8(c + 16)[:c], z64(nv + 1), z8(nv)) for c in caps]
    conv_types, tot = z8(nv), [z64(4) for _ in range(4)]
    load = lambda: eng.rdbload(pay, p_off, p_ty, *st[0], tot[0], stream=s)
    conv = lambda: eng.rdbconvert(pay, p_off, p_ty, st[0][2], st[1][0], st[1][1], conv_types, st[1][2], tot[1], stream=s)
    zset = lambda: eng.rdbzset(pay, p_off, p_ty, st[1][2], *st[2], tot[2], stream=s)
    load(), conv(), zset()
    torch.cuda.synchronize()
    sb = [int(x[1][-1].item()) for x in st]
    held = int((st[1][2] == 0).sum().item()), int((st[2][2] == 0).sum().item())
    print(f"share {share} %: n={nv} payload bytes={pb} stage bytes={sb} values held by stage 2 / 3: {held[0]} / {held[1]}"
          f" ({100.0 * (held[0] + held[1]) / nv:.2f} %)")
    total = sum(sb)
    nb = (total + 15) & ~15
    out, o_off, o_ty, o_st = z8(nb + 16)[:nb], z64(nv + 1), z8(nv), z8(nv)
    if what in ("stages", "all"):
        print(f"  rr_rdbload_batch {ms(timed(load))}  rr_rdbconvert_batch {ms(timed(conv))}  rr_rdbzset_batch {ms(timed(zset))}")
    if not hasattr(rr.lib(), "rr_rdbmerge_batch"):
        return
    merge = lambda: eng.rdbmerge(st[0], st[1], st[2], conv_types, p_ty, out, o_off, o_ty, o_st, tot[3], stream=s)
    if what in ("merge", "all"):
        tm = timed(merge)
        t = tot[3].cpu().numpy().view(np.uint64)
        assert int(t[1]) == total and int(t[3]) == total, (t, total)
        src = z8(nb)
        tc = timed(lambda: eng.copy_device(out, src, nb, stream=s))
        print(f"  rr_rdbmerge_batch {ms(tm)}  {total / tm[0] / 1e6:.1f} GB/s out  n_bad={int(t[2])};"
              f"  copy kernel over {nb} bytes {ms(tc)}  {nb / tc[0] / 1e6:.1f} GB/s;  merge / copy x{tm[0] / tc[0]:.2f}")
    if what in ("route", "all"):
        cap = rr.elem_bound(nv, nb)
        vals, elems, arena, dt = z8(nv * 16), z8(cap * 16), z8(nb), z64(4)
        eng.reserve(nv, nb)
        ws = z8(rr.rdbloadall_ws_bytes(nv, caps))
        d_sb = z64(3)

        def one():
            eng.rdbloadall(pay, p_off, p_ty, ws, caps, out, o_off, o_ty, o_st, d_sb, tot[3], stream=s)
            eng.decode_device(out, o_off, vals, elems, arena, dt, stream=s)

        t1 = timed(one)
        assert d_sb.tolist() == sb
        bufs = []
        for k in range(3):                                                    # the parent's recipe: a batch, a decode and buffers a stage
            b = (sb[k] + 15) & ~15
            c = rr.elem_bound(nv, b)
            bufs.append((z8(caps[k] + 16)[:max(b, 16)], z8(nv * 16), z8(c * 16), z8(max(b, 16)), z64(4)))

        def three():
            eng.rdbload(pay, p_off, p_ty, bufs[0][0], st[0][1], st[0][2], tot[0], stream=s)
            eng.rdbconvert(pay, p_off, p_ty, st[0][2], bufs[1][0], st[1][1], conv_types, st[1][2], tot[1], stream=s)
            eng.rdbzset(pay, p_off, p_ty, st[1][2], bufs[2][0], st[2][1], st[2][2], tot[2], stream=s)
            for k in range(3):
                eng.decode_device(bufs[k][0], st[k][1], bufs[k][1], bufs[k][2], bufs[k][3], bufs[k][4], stream=s)

        t3 = timed(three)
        td = timed(lambda: eng.decode_device(out, o_off, vals, elems, arena, dt, stream=s))
        print(f"  rr_rdbloadall_batch + 1 decode {ms(t1)} (the decode alone {ms(td)});  3 stage calls + 3 decodes {ms(t3)};"
              f"  one call / three decodes x{t1[0] / t3[0]:.2f}")


base = saved_config()
for share in shares:
    scenario(base, share)
