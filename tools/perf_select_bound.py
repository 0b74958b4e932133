#!/usr/bin/env python3
"""The selection from the bounds cache beside the selection from the mean cache, on one device (the
methodology of tools/perf_pooled_select.py): the C entries alone, device events, all forms of a shape interleaved in one process,
the order rotating, --rounds rounds of --reps launches each, one median per form and round, the median of those reported.

Shapes: section 5.13's -- bf16, D = 128, H = 32 query heads over Hkv = 8 K/V heads, 128-token blocks, one list per K/V head, causal,
a full cache (kv_len = Sk), one query row, top_k 16; (B, Sk) = (1, 131072) and (8, 32768).

  select            rsa_block_select_pooled beside rsa_block_select_bound, both at the library's score_splits: the bound's score
                    pass reads twice the bytes; the ratio is what the run says
  update            rsa_pool_keys(start = Sk - 1) beside rsa_pool_key_bounds(start = Sk - 1): one block per (b, K/V head)
  prefill           the two over the whole cache, as bytes of K over time beside the 6.3 TB/s the microarchitecture guide gives as
                    achievable (a description, not a gate)
  score_splits      rsa_block_select_bound at every count of --sweep and at the default (0), to confirm or replace the default

A difference is called one only where it exceeds the SPREAD of the baseline (largest minus smallest of its rounds' medians).
Every row, and the device's own box_ref (dense attention 1 x 24 x 16384 x 128 bf16), runs in a child process of its own under a
time limit; the first one that fails ends the run.  Prints one line per measurement and a final JSON line; --out FILE appends them.

    python tools/perf_select_bound.py [--reps 8] [--rounds 5] [--out profiles/select_bound_perf.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from perf_pooled_select import HBM_TBS, _round, box_ref  # noqa: E402

ROWS = [("long-16", 1, 131072, 1, 16), ("batch-16", 8, 32768, 1, 16)]


def default_splits(rows, NK, D):
    """sel_default_splits of rsa_block_select.hip: what score_splits = 0 resolves to."""
    if rows >= 512:
        return 1
    return max(1, min(-(-NK // (4096 // D)), -(-1024 // rows), 64, NK))


def shape_row(say, args, name, B, Sk, Sq, top_k, sweep):
    import torch
    from rectified_spaattn_amd import _core, _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    H, Hkv, D, blk = 32, 8, 128, 128
    NK, NW = Sk // blk, (Sk // blk + 31) // 32
    g = torch.Generator(device=dev).manual_seed(B * 7 + Sq + top_k)
    q = torch.randn(B, H, Sq, D, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Hkv, Sk, D, device=dev, generator=g).to(torch.bfloat16)
    dt, st = _core.dtype_code(q.dtype), _core._stream()
    tq, tk = _core._t4(q), _core._t4(k)
    rows = B * Hkv

    def lists():
        return (torch.zeros((rows, 1, NW), dtype=torch.int32, device=dev), torch.zeros((rows, 1, NK), dtype=torch.int32, device=dev),
                torch.zeros((rows, 1), dtype=torch.int32, device=dev))
    by_mean, by_bound = lists(), lists()
    means = torch.zeros((B, Hkv, NK, D), dtype=torch.float32, device=dev)
    bounds = torch.zeros((B, Hkv, NK, 2, D), dtype=torch.float32, device=dev)
    n = ctypes.c_size_t(0)
    _lib.check(L.rsa_block_select_bound_bytes(B, Hkv, Hkv, D, 1, NK, ctypes.byref(n)), "rsa_block_select_bound_bytes")
    ws, nb = torch.empty((n.value,), dtype=torch.uint8, device=dev), n.value

    def pool(entry, out, start):
        return lambda: _lib.check(getattr(L, entry)(B, Hkv, Sk, D, dt, blk, NK, tk, None, 0, 0, None, Sk, None, start, 0, out.data_ptr(),
                                                    st), entry)
    update_mean, prefill_mean = pool("rsa_pool_keys", means, Sk - Sq), pool("rsa_pool_keys", means, 0)
    update_bound, prefill_bound = pool("rsa_pool_key_bounds", bounds, Sk - Sq), pool("rsa_pool_key_bounds", bounds, 0)

    def select_mean():
        _lib.check(L.rsa_block_select_pooled(B, H, Hkv, Hkv, Sq, D, dt, blk, 1, NK, tq, means.data_ptr(), None, Sk, 1, top_k, 0, 0, 0,
                                             ws.data_ptr(), nb, by_mean[0].data_ptr(), by_mean[1].data_ptr(), by_mean[2].data_ptr(),
                                             None, st), "rsa_block_select_pooled")

    def select_bound(splits):
        return lambda: _lib.check(L.rsa_block_select_bound(B, H, Hkv, Hkv, Sq, D, dt, blk, 1, NK, tq, bounds.data_ptr(), None, Sk, 1,
                                                           top_k, 0, 0, splits, ws.data_ptr(), nb, by_bound[0].data_ptr(),
                                                           by_bound[1].data_ptr(), by_bound[2].data_ptr(), None, -1, 0.0, None, None,
                                                           st), "rsa_block_select_bound")
    forms = [s for s in sweep if s <= NK]
    # (the prefills, which sweep all of K through the caches, go last)
    fns = [select_mean, select_bound(0), update_mean, update_bound] + [select_bound(s) for s in forms] + [prefill_mean, prefill_bound]
    prefill_mean()
    prefill_bound()
    for _ in range(2):
        for f in fns:
            f()
    torch.cuda.synchronize()
    kept = (int(by_mean[2].min()), int(by_bound[2].min()))
    rounds = [_round(torch, fns, args.reps) for _ in range(args.rounds)]
    med = [1e3 * statistics.median(r[i] for r in rounds) for i in range(len(fns))]
    spread = [1e3 * (max(r[i] for r in rounds) - min(r[i] for r in rounds)) for i in range(len(fns))]
    k_bytes = k.numel() * 2
    dflt = default_splits(rows, NK, D)
    say(f"{name}: B = {B}, Sk = {Sk} ({NK} blocks), Sq = {Sq}, top_k = {top_k}; K = {k_bytes / 1e6:.1f} MB, the mean cache "
        f"{means.numel() * 4 / 1e6:.2f} MB, the bounds cache {bounds.numel() * 4 / 1e6:.2f} MB; kept per row {kept[0]} / {kept[1]}; "
        f"score_splits = 0 is {dflt}")
    say(f"  select_blocks_pooled: {med[0]:.1f} us (rounds: {' '.join(f'{1e3 * r[0]:.1f}' for r in rounds)}; spread {spread[0]:.1f} us)")
    say(f"  select_blocks_bound:  {med[1]:.1f} us (rounds: {' '.join(f'{1e3 * r[1]:.1f}' for r in rounds)}): {med[1] - med[0]:+.1f} us, "
        f"{med[1] / med[0]:.2f} x; beyond the spread: {abs(med[1] - med[0]) > spread[0]}")
    say(f"  update (start = Sk - {Sq}): pool_keys {med[2]:.1f} us (spread {spread[2]:.1f}), pool_key_bounds {med[3]:.1f} us: "
        f"{med[3] / med[2]:.2f} x; beyond the spread: {abs(med[3] - med[2]) > spread[2]}")
    say("  select_blocks_bound by score_splits: " + "  ".join(f"{s}: {med[4 + i]:.1f}" for i, s in enumerate(forms)) +
        f"  default ({dflt}): {med[1]:.1f}  (us; spread of the default {spread[1]:.1f})")
    say(f"  prefill: pool_keys {med[-2]:.1f} us = {k_bytes / med[-2] / 1e6:.3f} TB/s of K, pool_key_bounds {med[-1]:.1f} us = "
        f"{k_bytes / med[-1] / 1e6:.3f} TB/s of K: {med[-1] / med[-2]:.2f} x (achievable HBM: {HBM_TBS} TB/s)")
    return dict(name=name, B=B, Sk=Sk, Sq=Sq, top_k=top_k, default_splits=dflt, select_pooled_us=round(med[0], 2),
                select_pooled_spread_us=round(spread[0], 2), select_bound_us=round(med[1], 2),
                select_bound_spread_us=round(spread[1], 2), update_mean_us=round(med[2], 2), update_mean_spread_us=round(spread[2], 2),
                update_bound_us=round(med[3], 2), prefill_mean_us=round(med[-2], 2), prefill_bound_us=round(med[-1], 2),
                sweep_us={str(s): round(med[4 + i], 2) for i, s in enumerate(forms)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", default="1,4,8,16,32,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child process (one row) may take")
    ap.add_argument("--row", default=None, help="(internal) run this one row in this process and print its JSON as the last line")
    args = ap.parse_args()
    sweep = [int(x) for x in args.sweep.split(",")]
    if args.row:
        say = lambda s: print(s, flush=True)      # noqa: E731
        if args.row == "box_ref":
            res = box_ref(say, args)
        else:
            res = shape_row(say, args, *[r for r in ROWS if r[0] == args.row][0], sweep)
        print("JSON " + json.dumps(res), flush=True)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"select_blocks_pooled against select_blocks_bound, pool_keys against pool_key_bounds: bf16, D = 128, H = 32 over Hkv = 8, "
        f"128-token blocks, lists per K/V head, causal; {args.rounds} rounds x {args.reps} launches per form, interleaved")
    res = dict(reps=args.reps, rounds=args.rounds, rows=[])
    status = 0
    for name in ["box_ref"] + [r[0] for r in ROWS]:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--reps", str(args.reps), "--rounds", str(args.rounds),
               "--sweep", args.sweep]
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
