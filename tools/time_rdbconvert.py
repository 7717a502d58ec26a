"""Diagnostics: time rr_rdbconvert_batch (include/rr_rdbconvert.h); device-resident, HIP events.  Each
figure is the call time (every launch of the call) over `steps` calls after a warm-up call, three
trials, fastest and slowest shown.
  shapes   batches where every value converts (Hashes of 8 pairs, ZSets of 32, integer Sets of 64 and of
           512), beside rr_rdbload_batch on the same values in their already-converted RDB forms: the
           ratio is the cost of converting over loading
  mixed    a config batch as rr_rdbsave_batch writes it and one convertible Hash per hundred values
           behind it, the status rr_rdbload_batch gives under the default thresholds: the cost of the
           second stage when few values are attempted
Usage: python tools/time_rdbconvert.py [shapes|mixed|all] [n shapes] [n mixed] [steps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import redrock_old_amd as rr  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
n_shapes = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
n_mixed = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
eng = rr.Engine(0)
eng.set_options(rr.CTX_NO_SMALL)
s = torch.cuda.current_stream()
rng = np.random.default_rng(7)


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


def save_len(m):
    return bytes([m]) if m < 64 else bytes([0x40 | (m >> 8), m & 0xFF])


def fixed(n, count, rec):
    """n values of `count` records (rec: uint8[n, count, w]) behind the count's length prefix."""
    pre = np.frombuffer(save_len(count), np.uint8)
    body = rec.reshape(n, -1)
    data = np.concatenate([np.broadcast_to(pre, (n, len(pre))), body], axis=1)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(data.shape[1])
    return np.ascontiguousarray(data).reshape(-1), offs


def letters(shape):
    return rng.integers(97, 123, shape, dtype=np.uint8)


def shape_batches(n):
    rec = np.empty((n, 16, 9), np.uint8)                                # Hashes of 8 pairs: 8-letter fields and values
    rec[:, :, 0] = 8
    rec[:, :, 1:] = letters((n, 16, 8))
    yield "Hashes of 8 pairs", rr.T_HASH_HT, fixed(n, 8, rec)
    rec = np.empty((n, 32, 17), np.uint8)                               # ZSets of 32: 8-letter members, integer scores
    rec[:, :, 0] = 8
    rec[:, :, 1:9] = letters((n, 32, 8))
    rec[:, :, 9:] = rng.integers(0, 1000, (n, 32)).astype(np.float64).view(np.uint8).reshape(n, 32, 8)
    yield "ZSets of 32", rr.T_ZSET_SKIPLIST, fixed(n, 32, rec)
    for m in (64, 512):                                                 # integer Sets: 0xC2 + int32
        rec = np.empty((n, m, 5), np.uint8)
        rec[:, :, 0] = 0xC2
        rec[:, :, 1:] = rng.integers(-2**31, 2**31, (n, m), dtype=np.int64).astype(np.int32).view(np.uint8).reshape(n, m, 4)
        yield f"integer Sets of {m}", rr.T_SET_HT, fixed(n, m, rec)


def rdb_form(blobs, offs, otypes):
    """The converted blobs as the RDB payloads of their new types: one string, the intset / the ziplist."""
    b = blobs.tobytes()
    out = []
    for i, t in enumerate(otypes.tolist()):
        body = b[int(offs[i]) + (5 if t == rr.T_SET_INTSET else 13):int(offs[i + 1])]
        ln = len(body)
        out.append((bytes([ln]) if ln < 64 else bytes([0x40 | (ln >> 8), ln & 0xFF]) if ln < 16384
                    else b"\x80" + ln.to_bytes(4, "big")) + body)
    o = np.zeros(len(out) + 1, np.uint64)
    np.cumsum([len(x) for x in out], out=o[1:])
    return np.frombuffer(b"".join(out), np.uint8).copy(), o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def dev_offs(o):
    return torch.from_numpy(np.ascontiguousarray(o, np.uint64).view(np.int64).copy()).cuda()


def run_convert(name, d_data, d_offs, d_types, d_load, nv, out_bytes):
    out = torch.zeros(out_bytes + 16, dtype=torch.uint8, device="cuda")
    o_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    o_ty = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    o_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    t = timed(lambda: eng.rdbconvert(d_data, d_offs, d_types, d_load, out, o_off, o_ty, o_st, d_tot, stream=s))
    st = np.bincount(o_st.cpu().numpy(), minlength=46)
    kinds = " ".join(f"{k}:{int(c)}" for k, c in enumerate(st) if c)
    ob = int(o_off[-1].item())
    print(f"  rr_rdbconvert_batch  {t[0]:.3f}-{t[1]:.3f} ms  blob bytes={ob} n_bad={int(d_tot[2].item())} status {kinds}")
    return t, out[:ob].cpu().numpy(), o_off.cpu().numpy().view(np.uint64), o_ty.cpu().numpy(), st


def shapes():
    for name, typ, (data, offs) in shape_batches(n_shapes):
        nv, nb = len(offs) - 1, int(offs[-1])
        print(f"{name}: n={nv} payload bytes={nb}")
        d_data, d_offs = dev(data), dev_offs(offs)
        d_types = torch.full((nv,), typ, dtype=torch.uint8, device="cuda")
        l_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
        l_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
        eng.rdbload(d_data, d_offs, d_types, empty, l_off, l_st, d_tot, stream=s)   # the first stage: its status
        torch.cuda.synchronize()
        assert int((l_st == 38).sum().item()) == nv, "every value of a shape batch is RDBLOAD_E_CONVERT"
        tc, blobs, boffs, otypes, st = run_convert(name, d_data, d_offs, d_types, l_st, nv, rr.rdbconvert_bound(nv, nb))
        assert st[0] == nv, "every value of a shape batch converts"
        fdata, foffs = rdb_form(blobs, boffs, otypes)
        f_data, f_offs, f_types = dev(fdata), dev_offs(foffs), dev(otypes)
        f_out = torch.zeros(rr.rdbload_bound(nv, len(fdata)) + 16, dtype=torch.uint8, device="cuda")
        tl = timed(lambda: eng.rdbload(f_data, f_offs, f_types, f_out, l_off, l_st, d_tot, stream=s))
        assert int(d_tot[2].item()) == 0 and int(l_off[-1].item()) == len(blobs), "the converted forms load to the same blob bytes"
        print(f"  rr_rdbload_batch     {tl[0]:.3f}-{tl[1]:.3f} ms  on the converted forms ({len(fdata)} payload bytes)"
              f"  convert / load x{tc[0] / tl[0]:.2f}  {nv / tc[0] / 1e3:.2f} M values/s converted")


def mixed(cfg=4):
    data, offs = rr.gen_batch(cfg, n_mixed)
    nv, nb = len(offs) - 1, int(offs[-1])
    cap = rr.elem_bound(nv, nb)
    d_data, d_offs = torch.from_numpy(data).cuda(), dev_offs(offs)
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
    # the defaults leave no value of a config batch to convert (rr_rdbsave_batch writes the encodings as
    # they are), so one value in a hundred is added: Hashes of 8 pairs, behind the batch
    extra = nv // 100
    _, htyp, (hdata, hoffs) = next(shape_batches(extra))
    pay = torch.cat([pay[:pb], dev(hdata)])
    p_off = torch.cat([p_off[:nv], dev_offs(hoffs + np.uint64(pb))])
    p_ty = torch.cat([p_ty, torch.full((extra,), htyp, dtype=torch.uint8, device="cuda")])
    nv, pb = nv + extra, pb + len(hdata)
    out = torch.zeros(nb + 64 * nv + 16, dtype=torch.uint8, device="cuda")
    o_off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
    l_st = torch.zeros(nv, dtype=torch.uint8, device="cuda")
    tl = timed(lambda: eng.rdbload(pay[:pb], p_off, p_ty, out, o_off, l_st, d_tot, stream=s))
    att = int((l_st == 38).sum().item())
    print(f"cfg={cfg} n={nv} payload bytes={pb}: rr_rdbload_batch {tl[0]:.3f}-{tl[1]:.3f} ms, RDBLOAD_E_CONVERT {att}"
          f" ({100.0 * att / nv:.2f} % of the values)")
    tc, *_ = run_convert("mixed", pay[:pb], p_off, p_ty, l_st, nv, rr.rdbconvert_bound(nv, pb))
    print(f"  convert / load x{tc[0] / tl[0]:.2f}")


if what in ("shapes", "all"):
    shapes()
if what in ("mixed", "all"):
    mixed()
