#!/usr/bin/env python3
"""select_blocks (rsa_block_select: block_select_pool_kernel + block_select_kernel) at the HunyuanVideo
720p shape -- S = 115 456, D = 128, bf16, top_k = 90, 128-token blocks, H = 24 query heads over Hkv = 24 and 12 K/V heads, one
list per K/V head -- on one device, in one process, next to that device's own box_ref (dense attention 1 x 24 x 16384 x 128 bf16,
as bench.py measures it).

  default      the whole call (as_lists=True: workspace, both kernels, no mask round trip) against the torch composition it
               replaces -- reshape-mean of q and k, group sum, einsum, masked topk, scatter into a bool mask, block_mask_to_lists --
               for the plain top-k and for the MoBA-style call (causal, keep_first = 1, keep_local = 1).  Interleaved, the order
               rotating, --rounds rounds of --reps calls; the median of the rounds' medians and the spread of ours.  The two
               selections are compared row by row first (they differ only where fp32 rounding orders two near-equal scores).
  --kernels    only a few calls of select_blocks for one --hkv: the program for a kernel trace of its own,
               `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_select_blocks.py --kernels --hkv 12`
  --stats CSV  no device: the two kernels' lines of such a run's kernel_stats.csv, and the pooling pass's bytes per time (it reads q
               and k once and writes the pooled vectors) for --hkv.  K1 (pool_stats) moves 2.13 GB at the chip's copy ceiling
               (DESIGN.md section 11).

Prints one line per measurement (and a final JSON line in the default mode); --out FILE appends the lines there.

    python tools/perf_select_blocks.py [--reps 6] [--rounds 5] [--out profiles/block_select_perf.txt]
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, D, H, BLK, TOP_K = 115456, 128, 24, 128, 90


def pool_bytes(Hkv):
    N = S // BLK
    return 2 * S * D * (H + Hkv) + 4 * D * N * 2 * Hkv       # q and k once, the pooled query sums and keys (fp32) written


def stats(path, Hkv, say):
    for r in csv.DictReader(open(path)):
        if "block_select" not in r["Name"]:
            continue
        name = "block_select_pool_kernel" if "pool" in r["Name"] else "block_select_kernel"
        avg, lo, hi = (float(r[c]) / 1e3 for c in ("AverageNs", "MinNs", "MaxNs"))
        line = f"Hkv = {Hkv}: {name}: {r['Calls']} calls, avg {avg:.1f} us (min {lo:.1f}, max {hi:.1f})"
        if name.endswith("pool_kernel"):
            line += f"; {pool_bytes(Hkv) / 1e9:.3f} GB -> {pool_bytes(Hkv) / avg / 1e6:.2f} TB/s at the average"
        say(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hkv", type=int, default=12)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if args.stats:
        stats(args.stats, args.hkv, say)
        return finish()

    import torch
    from rectified_spaattn_amd import _core, block_sparse, select_blocks
    dev = torch.device("cuda:0")
    N = S // BLK
    g0 = torch.Generator(device=dev).manual_seed(7)
    q = torch.randn(1, H, S, D, device=dev, generator=g0).to(torch.bfloat16)
    k_all = torch.randn(1, H, S, D, device=dev, generator=g0).to(torch.bfloat16)

    if args.kernels:
        k = k_all[:, :args.hkv].contiguous()
        for _ in range(5):
            select_blocks(q, k, TOP_K, as_lists=True)
        torch.cuda.synchronize()
        return

    def ev(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    def one_round(fns, reps):
        evs = [[] for _ in fns]
        for i in range(reps):
            for j in range(len(fns)):
                w = (i + j) % len(fns)
                evs[w].append(ev(fns[w]))
        torch.cuda.synchronize()
        return [statistics.median(a.elapsed_time(b) for a, b in e) for e in evs]

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(dev))
    S0 = 16384
    x = torch.randn(1, 24, S0, 128, device=dev, generator=g0).to(torch.bfloat16)
    for _ in range(2):
        _core.dense_attention(x, x, x)
    torch.cuda.synchronize()
    dense_ms = statistics.median(one_round([lambda: _core.dense_attention(x, x, x)], args.reps)[0] for _ in range(3))
    say(f"box_ref: dense attention 1 x 24 x {S0} x 128 bf16: {dense_ms:.3f} ms = {4.0 * S0 * S0 * 128 * 24 / dense_ms / 1e9:.0f} TFLOP/s")
    res.update(box_ref_ms=round(dense_ms, 4))
    del x

    i_, j_ = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
    lower = j_ <= i_                                        # Sq = Sk, whole blocks: block j is visible to block i iff j <= i
    keep = (j_ == 0) | (j_ == i_)                           # keep_first = 1, keep_local = 1

    def torch_select(k, Hkv, moba):
        grp = H // Hkv
        qbar = q.view(1, H, N, BLK, D).mean(3, dtype=torch.float32)
        kbar = k.view(1, Hkv, N, BLK, D).mean(3, dtype=torch.float32)
        t = torch.einsum("bhid,bhjd->bhij", qbar.view(1, Hkv, grp, N, D).sum(2), kbar)
        if moba:
            t = t.masked_fill(~lower, float("-inf")).masked_fill(keep, float("inf"))
        idx = t.topk(TOP_K, dim=-1).indices
        mask = torch.zeros((1, Hkv, N, N), dtype=torch.bool, device=dev).scatter_(-1, idx, True)
        if moba:
            mask &= lower
        return block_sparse.block_mask_to_lists(mask, 1, Hkv)

    for Hkv in (24, 12):
        k = k_all[:, :Hkv].contiguous()
        for moba in (False, True):
            kw = dict(causal=True, keep_first=1, keep_local=1) if moba else {}
            fns = [lambda: select_blocks(q, k, TOP_K, as_lists=True, **kw), lambda: torch_select(k, Hkv, moba)]
            for _ in range(2):
                ours, theirs = fns[0](), fns[1]()
            torch.cuda.synchronize()
            same_counts = bool(torch.equal(ours["counts"], theirs["counts"]))
            rows_differ = int((ours["bitmask"] != theirs["bitmask"]).any(-1).sum())
            rounds = [one_round(fns, args.reps) for _ in range(args.rounds)]
            med = [statistics.median(r[i] for r in rounds) for i in range(2)]
            spread = max(r[0] for r in rounds) - min(r[0] for r in rounds)
            name = "causal, keep_first 1, keep_local 1" if moba else "plain top-k"
            say(f"H = {H} over Hkv = {Hkv}, {name}, top_k {TOP_K}, lists [{Hkv},{N},{N}]; {args.rounds} rounds x {args.reps} calls, "
                f"interleaved")
            say(f"  select_blocks(as_lists=True): {med[0]:.3f} ms   (rounds: {' '.join(f'{r[0]:.3f}' for r in rounds)}; spread "
                f"{spread:.3f} ms)")
            say(f"  torch composition:            {med[1]:.3f} ms   (rounds: {' '.join(f'{r[1]:.3f}' for r in rounds)})")
            say(f"  ratio torch / select_blocks: {med[1] / med[0]:.2f};  counts equal: {same_counts};  rows whose kept set differs: "
                f"{rows_differ} of {Hkv * N} (fp32 summation orders differ)")
            res[f"hkv{Hkv}_{'moba' if moba else 'plain'}"] = dict(select_ms=round(med[0], 4), torch_ms=round(med[1], 4),
                                                                 spread_ms=round(spread, 4), rows_differ=rows_differ)
    say(json.dumps(res))
    finish()


if __name__ == "__main__":
    main()
