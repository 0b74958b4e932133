#!/usr/bin/env python3
"""select_blocks_observed beside what it replaces and beside its floor, on one device (the methodology of
tools/perf_pooled_select.py): every form of a shape is captured in a HIP graph of its own, the replays are timed by device events,
all forms interleaved in one process, the order rotating, --rounds rounds of --reps replays each, one median per form and round,
the median of those reported with the spread (largest minus smallest of the rounds' medians).

Shapes: the README's serving shapes -- bf16, D = 128, H = 32 query heads over Hkv = 8 K/V heads, 128-token blocks, a paged cache
behind a shuffled table, causal, a full cache, one list per K/V head, top_k 64; (B, Sk) = (1, 131072) and (8, 32768); W = 64 and 16.

  observed          select_blocks_observed at the library's score_splits, and at every count of --sweep
  torch             the composition it replaces, on a gathered contiguous K: bf16 matmul, masked fp32 softmax over [B, H, W, Sk],
                    block sums, log, and torch.topk for the select step -- no forced blocks and no lists, so it undercounts
                    slightly what the call replaces
  copy              a device copy of K's bytes: the floor of a one-pass kernel
  bound step        one decode step of the bounds criterion: pool_key_bounds(start = Sk - 1) and select_blocks_bound at one row

Every row, and the device's own box_ref (dense attention 1 x 24 x 16384 x 128 bf16), runs in a child process of its own under a
time limit; the first one that fails ends the run.  Prints one line per measurement and a final JSON line; --out FILE appends them.

    python tools/perf_select_observed.py [--reps 8] [--rounds 5] [--out profiles/select_observed_perf.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from perf_pooled_select import HBM_TBS, _round, box_ref  # noqa: E402

ROWS = [("long-W64", 1, 131072, 64), ("long-W16", 1, 131072, 16), ("batch-W64", 8, 32768, 64), ("batch-W16", 8, 32768, 16)]
H, HKV, D, BLK, TOP_K = 32, 8, 128, 128, 64


def default_splits(B, NK):
    """What score_splits = None resolves to (rsa_select_observed.hip): 512 score workgroups where the key blocks allow it."""
    base = B * HKV * ((H // HKV + 3) // 4)
    return max(1, min(-(-512 // base), NK, 256))


def shape_row(say, args, name, B, Sk, W, sweep):
    import torch
    from rectified_spaattn_amd import pool_key_bounds, select_blocks_bound, select_blocks_observed
    dev = torch.device("cuda:0")
    NK, g = Sk // BLK, H // HKV
    gen = torch.Generator(device=dev).manual_seed(B * 7 + W)
    q = torch.randn(B, H, W, D, device=dev, generator=gen).to(torch.bfloat16)
    k = torch.randn(B, HKV, Sk, D, device=dev, generator=gen).to(torch.bfloat16)
    table = torch.randperm(B * NK, device=dev, generator=gen).view(B, NK).to(torch.int32)
    pool = torch.empty((B * NK, HKV, BLK, D), dtype=k.dtype, device=dev)
    pool[table.reshape(-1).long()] = k.view(B, HKV, NK, BLK, D).transpose(1, 2).reshape(B * NK, HKV, BLK, D)
    floor_dst, bounds = torch.empty_like(pool), pool_key_bounds(pool, block_table=table)
    causal = (torch.arange(Sk, device=dev)[None, :] <= torch.arange(W, device=dev)[:, None] + Sk - W)

    def observed(splits):
        return lambda: select_blocks_observed(q, pool, TOP_K, causal=True, block_table=table, as_lists=True, score_splits=splits)

    def composition():
        x = torch.matmul(q.view(B, HKV, g * W, D), k.transpose(2, 3)).float().view(B, H, W, Sk) * D ** -0.5
        p = torch.softmax(x.masked_fill(~causal, float("-inf")), -1)
        t = torch.log(p.view(B, HKV, g * W, NK, BLK).sum((2, 4)).clamp_min(2.0 ** -126))
        return torch.topk(t, TOP_K, -1).indices

    def bound_step():
        pool_key_bounds(pool, block_table=table, out=bounds, start=Sk - 1)
        return select_blocks_bound(q[:, :, -1:], bounds, TOP_K, causal=True, as_lists=True)
    forms = [s for s in sweep if s <= NK]
    fns = [observed(None), composition, lambda: floor_dst.copy_(pool), bound_step] + [observed(s) for s in forms]
    graphs, held = [], []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for f in fns:
            f()     # (warm: code objects, the allocator's pool)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                held.append(f())
            graphs.append(graph)
    replays = [gr.replay for gr in graphs]
    for _ in range(2):
        for r in replays:
            r()
    torch.cuda.synchronize()
    want = observed(None)()
    assert torch.equal(want["counts"], held[0]["counts"]) and torch.equal(want["bitmask"], held[0]["bitmask"])     # replay = eager
    rounds = [_round(torch, replays, args.reps) for _ in range(args.rounds)]
    med = [1e3 * statistics.median(r[i] for r in rounds) for i in range(len(fns))]
    spread = [1e3 * (max(r[i] for r in rounds) - min(r[i] for r in rounds)) for i in range(len(fns))]
    k_bytes, dflt = k.numel() * 2, default_splits(B, NK)
    say(f"{name}: B = {B}, Sk = {Sk} ({NK} blocks), W = {W}; K = {k_bytes / 1e6:.1f} MB; score_splits = None is {dflt}")
    say(f"  select_blocks_observed: {med[0]:.1f} us (rounds: {' '.join(f'{1e3 * r[0]:.1f}' for r in rounds)}; spread {spread[0]:.1f} us) "
        f"= {k_bytes / med[0] / 1e6:.3f} TB/s of K (achievable HBM: {HBM_TBS} TB/s)")
    say(f"  the torch composition:  {med[1]:.1f} us (spread {spread[1]:.1f}): {med[1] / med[0]:.2f} x the call")
    say(f"  a device copy of K:     {med[2]:.1f} us (spread {spread[2]:.1f}): the call takes {med[0] / med[2]:.2f} x the copy")
    say(f"  one bounds step:        {med[3]:.1f} us (spread {spread[3]:.1f}): pool_key_bounds(start = Sk - 1) + select_blocks_bound")
    say("  by score_splits: " + "  ".join(f"{s}: {med[4 + i]:.1f}" for i, s in enumerate(forms)) +
        f"  default ({dflt}): {med[0]:.1f}  (us; spread of the default {spread[0]:.1f})")
    return dict(name=name, B=B, Sk=Sk, W=W, default_splits=dflt, observed_us=round(med[0], 2), observed_spread_us=round(spread[0], 2),
                torch_us=round(med[1], 2), copy_us=round(med[2], 2), bound_step_us=round(med[3], 2),
                sweep_us={str(s): round(med[4 + i], 2) for i, s in enumerate(forms)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", default="1,4,16,64,256")
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

    say(f"select_blocks_observed: bf16, D = {D}, H = {H} over Hkv = {HKV}, {BLK}-token blocks, paged, causal, lists per K/V head, "
        f"top_k {TOP_K}; graph replays, {args.rounds} rounds x {args.reps} replays per form, interleaved")
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
