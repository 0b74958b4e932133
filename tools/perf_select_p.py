#!/usr/bin/env python3
"""What a per-row top-p budget costs in the selection and saves in the decode call, on one device (the
methodology of tools/perf_pooled_select.py): the C entries alone, device events, all forms of a row interleaved in one process,
the order rotating, --rounds rounds of --reps launches each, one median per form and round, the median of those reported.

Shapes: those of profiles/pooled_select_perf.txt -- bf16, D = 128, H = 32 query heads over Hkv = 8 K/V heads, 128-token blocks,
one list per K/V head, causal, Sq = 1, a full cache; (B, Sk) = (1, 131072) and (8, 32768).  Inputs: `flat` (q and k standard
normal: pooled logits of a few hundredths at the default score_scale, a near-uniform row) and `concentrated` (eight hashed key
blocks per K/V head carry a common offset along q's mean direction: they hold nearly all of the row's mass).

  (a) the selection   rsa_block_select_pooled (top_k = 64) against rsa_block_select_pooled_p (cap 64, --top-p) on the same pooled
                      cache, both at the library's score_splits.  The difference is the weight passes; it is stated, not gated.
  (b) the decode      rsa_block_sparse_decode over the top_k = 64 lists against the top-p lists capped at 64, with the mean and
                      the largest count and the mean kept mass of the top-p rows.

"Faster" / "slower" is said only where the difference exceeds the SPREAD of the baseline (largest minus smallest of its rounds'
medians).  Every row runs in a child process of its own under a time limit; the first one that fails ends the run.  Prints one
line per measurement and a final JSON line; --out FILE appends them.

    python tools/perf_select_p.py [--reps 8] [--rounds 5] [--top-p 0.9] [--out profiles/select_p_perf.txt]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.perf_pooled_select import _round  # noqa: E402

CAP = 64
ROWS = [(f"{shape}-{kind}", B, Sk, kind) for shape, B, Sk in (("long", 1, 131072), ("batch", 8, 32768))
        for kind in ("flat", "concentrated")]


def shape_row(say, args, name, B, Sk, kind):
    import torch
    from rectified_spaattn_amd import _core, _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    H, Hkv, D, blk, Sq = 32, 8, 128, 128, 1
    NK, NW = Sk // blk, (Sk // blk + 31) // 32
    g = torch.Generator(device=dev).manual_seed(B * 7 + len(kind))
    q = torch.randn(B, H, Sq, D, device=dev, generator=g)
    k = torch.randn(B, Hkv, Sk, D, device=dev, generator=g)
    if kind == "concentrated":
        q += 1.0
        hot = torch.stack([torch.randperm(NK, device=dev, generator=g)[:8] for _ in range(B * Hkv)]).view(B, Hkv, 8)
        k.view(B, Hkv, NK, blk, D).scatter_add_(2, hot[..., None, None].expand(B, Hkv, 8, blk, D),
                                                torch.full((B, Hkv, 8, blk, D), 2.0, device=dev))
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    v = torch.randn(B, Hkv, Sk, D, device=dev, generator=g).to(torch.bfloat16)
    dt, st = _core.dtype_code(q.dtype), _core._stream()
    tq, tk, tv = _core._t4(q), _core._t4(k), _core._t4(v)
    rows = B * Hkv
    c = (1.0 / ((H // Hkv) * math.sqrt(D))) * 1.4426950408889634        # the default score_scale
    p16 = int(round(args.top_p * 65536.0))

    def lists():
        return (torch.zeros((rows, 1, NW), dtype=torch.int32, device=dev), torch.zeros((rows, 1, NK), dtype=torch.int32, device=dev),
                torch.zeros((rows, 1), dtype=torch.int32, device=dev))
    by_k, by_p = lists(), lists()
    mass = torch.zeros((rows, 1), dtype=torch.float32, device=dev)
    cache = torch.zeros((B, Hkv, NK, D), dtype=torch.float32, device=dev)
    n = ctypes.c_size_t(0)
    _lib.check(L.rsa_block_select_pooled_bytes(B, Hkv, Hkv, D, 1, NK, ctypes.byref(n)), "rsa_block_select_pooled_bytes")
    ws, nb = torch.empty((n.value,), dtype=torch.uint8, device=dev), n.value
    _lib.check(L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hkv, Sq, D, NK, 0, ctypes.byref(n)), "rsa_block_sparse_decode_bytes")
    ws_dec, nb_dec = torch.empty((n.value,), dtype=torch.uint8, device=dev), n.value
    outs = [torch.zeros((B, H, Sq, D), dtype=q.dtype, device=dev) for _ in range(2)]
    o4 = [_lib.RsaOut4(o.data_ptr(), o.stride(0), o.stride(1), o.stride(2)) for o in outs]
    _lib.check(L.rsa_pool_keys(B, Hkv, Sk, D, dt, blk, NK, tk, None, 0, 0, None, Sk, None, 0, 0, cache.data_ptr(), st), "rsa_pool_keys")

    def select_k():
        _lib.check(L.rsa_block_select_pooled(B, H, Hkv, Hkv, Sq, D, dt, blk, 1, NK, tq, cache.data_ptr(), None, Sk, 1, CAP, 0, 0, 0,
                                             ws.data_ptr(), nb, by_k[0].data_ptr(), by_k[1].data_ptr(), by_k[2].data_ptr(), None, st),
                   "rsa_block_select_pooled")

    def select_p():
        _lib.check(L.rsa_block_select_pooled_p(B, H, Hkv, Hkv, Sq, D, dt, blk, 1, NK, tq, cache.data_ptr(), None, Sk, 1, CAP, 0, 0, 0,
                                               ws.data_ptr(), nb, by_p[0].data_ptr(), by_p[1].data_ptr(), by_p[2].data_ptr(), None,
                                               p16, c, mass.data_ptr(), st), "rsa_block_select_pooled_p")

    def decode(which):
        ls = (by_k, by_p)[which]
        return lambda: _lib.check(L.rsa_block_sparse_decode(B, H, Hkv, Hkv, Sq, Sk, D, dt, blk, NK, None, Sk, 1, D ** -0.5, tq, tk, tv,
                                                            None, 0, 0, ls[1].data_ptr(), ls[2].data_ptr(), 0, ws_dec.data_ptr(),
                                                            nb_dec, o4[which], None, st), "rsa_block_sparse_decode")
    fns = [select_k, select_p, decode(0), decode(1)]
    for _ in range(2):
        for f in fns:
            f()
    torch.cuda.synchronize()
    cnt_k, cnt_p = by_k[2].float(), by_p[2].float()
    rounds = [_round(torch, fns, args.reps) for _ in range(args.rounds)]
    med = [1e3 * statistics.median(r[i] for r in rounds) for i in range(len(fns))]
    spread = [1e3 * (max(r[i] for r in rounds) - min(r[i] for r in rounds)) for i in range(len(fns))]
    say(f"{name}: B = {B}, Sk = {Sk} ({NK} blocks), top_p = {args.top_p}, cap {CAP}")
    say(f"  (a) select top_k {med[0]:.1f} us (spread {spread[0]:.1f}), select top_p {med[1]:.1f} us (spread {spread[1]:.1f}): "
        f"{med[1] - med[0]:+.1f} us; beyond the spread: {abs(med[1] - med[0]) > spread[0]}")
    say(f"  (b) decode over top_k lists {med[2]:.1f} us (spread {spread[2]:.1f}; count {cnt_k.mean().item():.1f}), over top_p lists "
        f"{med[3]:.1f} us (spread {spread[3]:.1f}; count mean {cnt_p.mean().item():.1f} max {int(cnt_p.max().item())}, kept mass mean "
        f"{mass.mean().item():.4f} min {mass.min().item():.4f}): {med[3] - med[2]:+.1f} us; beyond the spread: "
        f"{abs(med[3] - med[2]) > spread[2]}")
    return dict(name=name, B=B, Sk=Sk, kind=kind, top_p=args.top_p, cap=CAP, select_k_us=round(med[0], 2), select_p_us=round(med[1], 2),
                select_k_spread_us=round(spread[0], 2), decode_k_us=round(med[2], 2), decode_p_us=round(med[3], 2),
                decode_k_spread_us=round(spread[2], 2), count_k_mean=round(cnt_k.mean().item(), 2),
                count_p_mean=round(cnt_p.mean().item(), 2), count_p_max=int(cnt_p.max().item()), mass_mean=round(mass.mean().item(), 5),
                mass_min=round(mass.min().item(), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child process (one row) may take")
    ap.add_argument("--row", default=None, help="(internal) run this one row in this process and print its JSON as the last line")
    args = ap.parse_args()
    if args.row:
        res = shape_row(lambda s: print(s, flush=True), args, *[r for r in ROWS if r[0] == args.row][0])
        print("JSON " + json.dumps(res), flush=True)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"top-k against top-p block selection and the decode call over their lists: bf16, D = 128, H = 32 over Hkv = 8, 128-token "
        f"blocks, lists per K/V head, causal, Sq = 1; {args.rounds} rounds x {args.reps} launches per form, interleaved")
    res = dict(reps=args.reps, rounds=args.rounds, rows=[])
    status = 0
    for name in [r[0] for r in ROWS]:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--reps", str(args.reps), "--rounds", str(args.rounds),
               "--top-p", str(args.top_p)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            say(f"{name}: no result within {args.limit} s; the run ends here")
            status = 1
            break
        out = p.stdout.splitlines()
        for s in out:
            if not s.startswith("JSON "):
                say(s)
        if p.returncode != 0 or not out or not out[-1].startswith("JSON "):
            say(f"{name}: the child process ended with status {p.returncode}; the run ends here")
            status = 1
            break
        res["rows"].append(json.loads(out[-1][5:]))
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
