#!/usr/bin/env python3
"""block_sparse_extend (rsa_block_sparse_extend) next to what a caller does without it, on one device,
interleaved in one process, medians of device-event timings (the methodology of tools/perf_decode.py).

Shapes: bf16 q, D = 128, H = 32 query heads over Hkv = 8 K/V heads, 128-token blocks; the chunk is the last Sq tokens of a cache
of (B, Sk) = (1, 131072) and (8, 32768), Sq in 16 / 64 / 128 / 512 / 2048; one list per K/V head and query block from
select_blocks_pooled(causal=True, keep_first=1, keep_local=1) at top_k 16 and 64; the cache paged, bf16 and e4m3 (k_scale 0.5,
v_scale 2).

  (a) K5         rsa_block_sparse_gqa_fwd with the causal row ranges -- what block_sparse_attention(causal=True) launches -- on
                 a cache that is ALREADY contiguous and 2-byte (for the e4m3 rows: its dequantised twin).  The floor.
  (b) gather+K5  the gather of the whole cache through the table with torch (index_select, permute, copy; for e4m3 the cast
                 and the multiplication by the scale besides), then (a): what a caller must do today.
  decode         rsa_block_sparse_decode, where it serves the shape (Sq = 16: 64 rows a unit), default split
  extend         rsa_block_sparse_extend(_kv8) at the library's default split and at every blocks_per_split of --sweep
                 ("one" = NK, one split); a form whose workspace would pass --max-ws-gb is skipped and says so

All forms of a shape are timed interleaved, the order rotating, in --rounds rounds of --reps launches each; a round gives one
median per form.  Reported: the median of the rounds' medians, the SPREAD of (a) (largest minus smallest of its rounds' medians: a
difference below it is not a difference), and the largest |K5 - extend| of the outputs.

    python tools/perf_extend.py [--reps 5] [--rounds 3] [--out profiles/extend_perf.txt]

--ab-decode name=path: instead, rsa_block_sparse_decode of this tree's library and of the library at path (the parent commit's
build), loaded side by side, interleaved on the six shapes of tools/perf_decode.py at the default split (tools/ab_libs.py --decode
runs this).  Reported per shape: both medians and the spread of the other library's own rounds.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rectified_spaattn_amd import _core, _lib, block_sparse  # noqa: E402

K_SCALE, V_SCALE = 0.5, 2.0
E4M3 = torch.float8_e4m3fn
H, HKV, D, BLK = 32, 8, 128, 128


def _ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _round(fns, reps):
    """One median (ms) per function: reps launches each, interleaved, the order rotating."""
    evs = [[] for _ in fns]
    for i in range(reps):
        for j in range(len(fns)):
            w = (i + j) % len(fns)
            evs[w].append(_ev(fns[w]))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) for e in evs]


def _pages(t, perm, B, NK):
    """[B, Hkv, Sk, D] -> the page pool [B * NK, Hkv, BLK, D] with block j of item b at page perm[b * NK + j]."""
    seq = t.view(B, HKV, NK, BLK, D).permute(0, 2, 1, 3, 4).reshape(B * NK, HKV, BLK, D)
    out = torch.empty_like(seq)
    out[perm] = seq
    return out


_LUT = {}


def dequantise(x8, sc):
    """e4m3 codes -> bf16 code * scale on the device: torch's cast where this build has one that agrees with the CPU cast, else
    a 256-entry table of the CPU cast's values (said once)."""
    dev = x8.device
    if not _LUT:
        lut = torch.arange(256, dtype=torch.uint8).view(E4M3).float().nan_to_num(0.0).to(torch.bfloat16).to(dev)
        try:
            cast = torch.arange(256, dtype=torch.uint8, device=dev).view(E4M3).to(torch.bfloat16).float().nan_to_num(0.0)
            ok = bool(torch.equal(cast, lut.float()))
        except (RuntimeError, NotImplementedError):
            ok = False
        _LUT.update(lut=lut, cast=ok)
        print(f"dequantisation by {'the device cast of torch' if ok else 'a table lookup (this torch build has no usable device cast)'}",
              flush=True)
    if _LUT["cast"]:
        return x8.to(torch.bfloat16) * sc
    return _LUT["lut"].index_select(0, x8.view(torch.uint8).reshape(-1).int()).view(x8.shape) * sc


class Cache:
    """One (B, Sk): the contiguous bf16 cache (and the dequantised twin of the e4m3 one), both as page pools, the table, the
    pooled keys."""

    def __init__(self, B, Sk, dev):
        g = torch.Generator(device=dev).manual_seed(B * 7 + Sk)
        self.B, self.Sk, self.NK = B, Sk, Sk // BLK
        k = torch.randn(B, HKV, Sk, D, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(B, HKV, Sk, D, device=dev, generator=g).to(torch.bfloat16)
        perm = torch.randperm(B * self.NK, device=dev, generator=g)
        self.table = perm.view(B, self.NK).to(torch.int32).contiguous()
        k8, v8 = (torch.empty((B, HKV, Sk, D), dtype=torch.uint8, device=dev).view(E4M3) for _ in range(2))
        block_sparse.append_kv_e4m3(k, v, k8, v8, start=0, k_scale=K_SCALE, v_scale=V_SCALE)       # the cache's own writer
        kd, vd = dequantise(k8, K_SCALE), dequantise(v8, V_SCALE)
        self.contig = {"bf16": (k, v), "e4m3": (kd, vd)}
        self.pools = {"bf16": (_pages(k, perm, B, self.NK), _pages(v, perm, B, self.NK)),
                      "e4m3": tuple(_pages(t.view(torch.uint8), perm, B, self.NK).view(E4M3) for t in (k8, v8))}
        self.scales = [torch.full((HKV,), s, dtype=torch.float32, device=dev) for s in (K_SCALE, V_SCALE)]
        self.pooled = {form: block_sparse.pool_keys(self.contig[form][0]) for form in ("bf16", "e4m3")}
        self.gen = g


def shape_row(say, args, cache, form, Sq, top_k, sweep):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B, Sk, NK = cache.B, cache.Sk, cache.NK
    NQ = -(-Sq // BLK)
    q = torch.randn(B, H, Sq, D, device=dev, generator=cache.gen).to(torch.bfloat16)
    lists = block_sparse.select_blocks_pooled(q, cache.pooled[form], top_k, causal=True, keep_first=1, keep_local=1, as_lists=True)
    cols, counts = lists["cols"], lists["counts"]
    kept = int(counts.sum())
    kc, vc = cache.contig[form]
    kp, vp = cache.pools[form]
    _, hi = block_sparse._window_ranges(dev, B, Sq, Sk, [Sk] * B, -1, 0)
    hi = hi.contiguous()
    tpart = block_sparse._tail_buffer(dev)
    outs = [torch.zeros((B, H, Sq, D), dtype=q.dtype, device=dev) for _ in range(3)]
    o4 = [_lib.RsaOut4(o.data_ptr(), o.stride(0), o.stride(1), o.stride(2)) for o in outs]
    dt = _core.dtype_code(q.dtype)
    st = _core._stream()
    scale = D ** -0.5
    tq = _core._t4(q)
    table = cache.table
    idx = table.reshape(-1).long()

    def k5_on(k, v):
        _lib.check(L.rsa_block_sparse_gqa_fwd(B, H, HKV, HKV, Sq, Sk, D, dt, BLK, NQ, NK, Sk, scale, tq, _core._t4(k), _core._t4(v),
                                              cols.data_ptr(), counts.data_ptr(), None, hi.data_ptr(), 0 if hi.shape[0] == 1 else Sq,
                                              tpart.data_ptr(), tpart.numel() * 4, o4[0], st), "rsa_block_sparse_gqa_fwd")

    def k5():
        k5_on(kc, vc)

    def gather(pool, sc):
        x = pool.view(torch.uint8).index_select(0, idx).view(E4M3) if form == "e4m3" else pool.index_select(0, idx)
        x = x.view(B, NK, HKV, BLK, D).permute(0, 2, 1, 3, 4)
        if form == "e4m3":
            return dequantise(x.reshape(B, HKV, Sk, D), sc)
        return x.reshape(B, HKV, Sk, D)

    def gather_k5():
        k5_on(gather(kp, K_SCALE), gather(vp, V_SCALE))

    tail = (cache.scales[0].data_ptr(), cache.scales[1].data_ptr(), st) if form == "e4m3" else (st,)
    suffix = "_kv8" if form == "e4m3" else ""
    tkp, tvp = _core._t4(kp), _core._t4(vp)
    skipped = []

    def sized(entry, bytes_entry, bargs, bps, out):
        need = ctypes.c_size_t(0)
        _lib.check(getattr(L, bytes_entry)(*bargs, bps, ctypes.byref(need)), bytes_entry)
        if need.value > args.max_ws_gb * 2 ** 30:
            skipped.append((bps, need.value))
            return None, need.value
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)

        def run():
            _lib.check(getattr(L, entry + suffix)(B, H, HKV, HKV, Sq, Sk, D, dt, BLK, NK, None, Sk, 1, scale, tq, tkp, tvp,
                                                  table.data_ptr(), NK, B * NK, cols.data_ptr(), counts.data_ptr(), bps,
                                                  ws.data_ptr(), need.value, out, None, *tail), entry + suffix)
        return run, need.value

    names, fns, ws_of = ["K5", "gather+K5"], [k5, gather_k5], {}
    if Sq * (H // HKV) <= 64:
        run, _ = sized("rsa_block_sparse_decode", "rsa_block_sparse_decode_bytes", (B, H, HKV, HKV, Sq, D, NK), 0, o4[2])
        names.append("decode")
        fns.append(run)
    for bps in [0] + [c for c in sweep if c < NK] + [NK]:
        run, need = sized("rsa_block_sparse_extend", "rsa_block_sparse_extend_bytes", (B, H, HKV, HKV, Sq, D, BLK, NK), bps, o4[1])
        label = "extend" if bps == 0 else f"extend/{'one' if bps == NK else bps}"
        ws_of[label] = need
        if run is not None:
            names.append(label)
            fns.append(run)
    if "extend" not in names:
        raise SystemExit(f"the default split's workspace ({ws_of['extend'] / 2 ** 30:.1f} GiB) passes --max-ws-gb")
    for _ in range(2):
        for f in fns:
            f()
    fns[0]()
    fns[names.index("extend")]()
    torch.cuda.synchronize()
    diff = float((outs[0].float() - outs[1].float()).abs().max())
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    med = {n: statistics.median(r[i] for r in rounds) for i, n in enumerate(names)}
    spread = max(r[0] for r in rounds) - min(r[0] for r in rounds)
    groups = block_sparse.extend_row_groups(B, H, HKV, HKV, Sq, BLK)["groups"]
    say(f"B = {B}, Sk = {Sk} ({NK} blocks), {form} paged, Sq = {Sq}, top_k = {top_k}: {groups} row groups, {kept} kept (list row, "
        f"block) pairs; default split = {block_sparse.extend_default_split(groups, NK)}, workspace {ws_of['extend'] / 2 ** 20:.1f} MiB")
    say(f"  (a) K5 on a contiguous 2-byte cache: {1e3 * med['K5']:.1f} us (spread {1e3 * spread:.1f});  (b) gather"
        f"{' + dequantise' if form == 'e4m3' else ''} + K5: {1e3 * med['gather+K5']:.1f} us"
        + (f";  decode: {1e3 * med['decode']:.1f} us" if "decode" in med else ""))
    say("  extend: default " + f"{1e3 * med['extend']:.1f} us;  by blocks_per_split: "
        + "  ".join(f"{n.split('/')[1]}: {1e3 * med[n]:.1f}" for n in names if n.startswith("extend/"))
        + ("  (skipped, workspace: " + ", ".join(f"{c}: {w / 2 ** 30:.1f} GiB" for c, w in skipped) + ")" if skipped else ""))
    best = min((n for n in names if n.startswith("extend")), key=lambda n: med[n])
    say(f"  extend / (b) = {med['extend'] / med['gather+K5']:.2f}, extend / (a) = {med['extend'] / med['K5']:.2f}; beats (b): "
        f"{med['gather+K5'] - med['extend'] > spread}, beats (a): {med['K5'] - med['extend'] > spread}; best form {best} "
        f"({1e3 * med[best]:.1f} us); largest |K5 - extend| of the outputs: {diff:.3e}")
    return dict(B=B, Sk=Sk, form=form, Sq=Sq, top_k=top_k, groups=groups, spread_us=round(1e3 * spread, 2), out_diff=diff,
                us={n: round(1e3 * t, 2) for n, t in med.items()}, ws_mib={n: round(w / 2 ** 20, 1) for n, w in ws_of.items()})


DECODE_ROWS = [("long-16", 1, 131072, 1, 16, False), ("long-64", 1, 131072, 1, 64, False), ("batch-16", 8, 32768, 1, 16, False),
               ("batch-64", 8, 32768, 1, 64, False), ("batch-64-Sq4", 8, 32768, 4, 64, False), ("batch-64-paged", 8, 32768, 1, 64, True)]


def ab_decode(say, args, other_name, other_path):
    """rsa_block_sparse_decode of two builds, side by side: the six rows of tools/perf_decode.py at the default split."""
    dev = torch.device("cuda:0")
    libs = [("this tree", _lib.lib()), (other_name, ctypes.CDLL(os.path.abspath(other_path)))]
    for _, L in libs:
        for name in ("rsa_block_sparse_decode", "rsa_block_sparse_decode_bytes"):
            getattr(L, name).restype, getattr(L, name).argtypes = _lib.PROTOTYPES[name]
    say(f"block_sparse_decode, this tree's library against {other_name} ({os.path.basename(other_path)}), loaded side by side: bf16, "
        f"D = 128, H = 32 over Hkv = 8, 128-token blocks, default split; {args.rounds} rounds x {args.reps} launches per library, "
        "interleaved")
    res = []
    for name, B, Sk, Sq, top_k, paged in DECODE_ROWS:
        NK = Sk // BLK
        g = torch.Generator(device=dev).manual_seed(B * 7 + Sq + top_k)
        q = torch.randn(B, H, Sq, D, device=dev, generator=g).to(torch.bfloat16)
        k = torch.randn(B, HKV, Sk, D, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(B, HKV, Sk, D, device=dev, generator=g).to(torch.bfloat16)
        lists = block_sparse.select_blocks(q, k, top_k, causal=True, as_lists=True)
        cols, counts = lists["cols"], lists["counts"]
        targs = (None, 0, 0)
        if paged:
            perm = torch.randperm(B * NK, device=dev, generator=g)
            k, v = _pages(k, perm, B, NK), _pages(v, perm, B, NK)
            table = perm.view(B, NK).to(torch.int32).contiguous()
            targs = (table.data_ptr(), NK, B * NK)
        outs = [torch.zeros((B, H, Sq, D), dtype=q.dtype, device=dev) for _ in libs]
        need = ctypes.c_size_t(0)
        _lib.check(libs[0][1].rsa_block_sparse_decode_bytes(B, H, HKV, HKV, Sq, D, NK, 0, ctypes.byref(need)), "decode_bytes")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
        st = _core._stream()

        def make(L, out):
            o4 = _lib.RsaOut4(out.data_ptr(), out.stride(0), out.stride(1), out.stride(2))

            def run():
                rc = L.rsa_block_sparse_decode(B, H, HKV, HKV, Sq, Sk, D, _lib.RSA_BF16, BLK, NK, None, Sk, 1, D ** -0.5, _core._t4(q),
                                               _core._t4(k), _core._t4(v), *targs, cols.data_ptr(), counts.data_ptr(), 0,
                                               ws.data_ptr(), need.value, o4, None, st)
                assert rc == 0, rc
            return run
        fns = [make(L, o) for (_, L), o in zip(libs, outs)]
        for _ in range(3):
            for f in fns:
                f()
        torch.cuda.synchronize()
        equal = bool(torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)))
        rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
        med = [statistics.median(r[i] for r in rounds) for i in range(2)]
        spread = max(r[1] for r in rounds) - min(r[1] for r in rounds)
        say(f"  {name}: this tree {1e3 * med[0]:.1f} us, {other_name} {1e3 * med[1]:.1f} us (its rounds: "
            f"{' '.join(f'{1e3 * r[1]:.1f}' for r in rounds)}; spread {1e3 * spread:.1f} us); agree within the spread: "
            f"{abs(med[0] - med[1]) <= spread}; outputs byte-equal: {equal}")
        res.append(dict(name=name, this_us=round(1e3 * med[0], 2), other_us=round(1e3 * med[1], 2), spread_us=round(1e3 * spread, 2),
                        agree=bool(abs(med[0] - med[1]) <= spread), byte_equal=equal))
        del k, v
        torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", default="1,2,4,8,16")
    ap.add_argument("--sqs", default="16,64,128,512,2048")
    ap.add_argument("--top-ks", default="16,64")
    ap.add_argument("--max-ws-gb", type=float, default=4.0)
    ap.add_argument("--ab-decode", default=None, metavar="NAME=PATH")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    if args.ab_decode:
        name, path = args.ab_decode.split("=", 1)
        res["ab_decode"] = ab_decode(say, args, name, path)
    else:
        sweep = [int(x) for x in args.sweep.split(",")]
        say(f"block_sparse_extend against (a) K5 on a contiguous 2-byte cache and (b) gather (+ dequantise) + K5: bf16 q, D = {D}, "
            f"H = {H} over Hkv = {HKV}, {BLK}-token blocks, causal, lists per K/V head from select_blocks_pooled(keep_first=1, "
            f"keep_local=1); {args.rounds} rounds x {args.reps} launches per form, interleaved")
        res["rows"] = []
        for B, Sk in ((1, 131072), (8, 32768)):
            cache = Cache(B, Sk, torch.device("cuda:0"))
            for form in ("bf16", "e4m3"):
                for top_k in [int(x) for x in args.top_ks.split(",")]:
                    for Sq in [int(x) for x in args.sqs.split(",")]:
                        res["rows"].append(shape_row(say, args, cache, form, Sq, top_k, sweep))
            del cache
            torch.cuda.empty_cache()
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
