#!/usr/bin/env python3
"""merge_partials (rsa_merge_partials) next to the torch expression of the same contract -- what a caller
runs without it -- on the same tensors, on one device, interleaved in one process, medians of device-event timings (the methodology
of tools/perf_extend.py).

Shapes: bf16 partials, H = 32, D = 128.
  serving steps   packed [T, H, D] / [T, H] with T = 8 and 576, N = 2 and 8 partials
  HBM-sized       padded [1, 32, 32768, 128], N = 2: 256 MiB per out; beside the times, the bytes the merge must move (N outs and
                  lses in, one out and lse back) per second, and the rate of a device copy of as many bytes (a torch copy_ of half
                  of them: read once, written once), measured by this script on this device

  torch           m = max_i lse_i; w_i = exp(lse_i - m); out = (sum_i w_i out_i / sum_i w_i).to(dtype); lse = m + log(sum_i w_i) on
                  the stacked tensors, rows without a live entry patched to 0 / -inf with where (the contract; without the patch the
                  expression gives NaN there)
  merge           merge_partials into preallocated results, list form; "stacked": the same from one stacked [N, ...] tensor

Both forms of a shape are timed interleaved, the order rotating, in --rounds rounds of --reps launches each; a round gives one
median per form.  Reported: the median of the rounds' medians, the SPREAD of the torch form (largest minus smallest of its rounds'
medians: a difference below it is not a difference), the speedup, and the largest |torch - merge| of the outputs.  On an idle stream
the small shapes measure the host: the Python layer and one launch against about ten.  So each of the two forms is also captured in
a graph of its own and the replays are timed the same way: the device's time without the host's.

    python tools/perf_merge.py [--reps 20] [--rounds 5] [--out profiles/merge_perf.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rectified_spaattn_amd import block_sparse  # noqa: E402

H, D = 32, 128


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


def torch_merge(outs, lses):
    """The contract in torch, on stacked [N, ...] tensors: what a caller writes today."""
    m = lses.max(0).values
    live = m > float("-inf")
    w = torch.exp(lses - torch.where(live, m, torch.zeros_like(m)))
    l = w.sum(0)
    acc = (w.unsqueeze(-1) * outs.float()).sum(0)
    out = torch.where(live.unsqueeze(-1), acc / l.unsqueeze(-1), torch.zeros_like(acc)).to(outs.dtype)
    return out, torch.where(live, m + torch.log(l), m)


def merge_bytes(N, rows):
    """What the merge must move: N outs and lses read, one out and lse written."""
    return (N + 1) * rows * (D * 2 + 4)


def shape_row(say, args, name, shape, N, rate=False):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N * 1000 + shape[0] + shape[-2])
    outs = torch.randn((N,) + shape, device=dev, generator=g).to(torch.bfloat16)
    lses = 3.0 * torch.randn((N,) + shape[:-1], device=dev, generator=g)
    lses[torch.rand(lses.shape, device=dev, generator=g) < 0.05] = float("-inf")      # a few dead entries, as extend writes them
    po, pl = [o.clone() for o in outs], [x.clone() for x in lses]
    res, res_l = torch.empty_like(po[0]), torch.empty_like(pl[0])
    res2, res2_l = torch.empty_like(po[0]), torch.empty_like(pl[0])
    names = ["torch", "merge", "merge, stacked"]
    fns = [lambda: torch_merge(outs, lses),
           lambda: block_sparse.merge_partials(po, pl, out=res, lse=res_l),
           lambda: block_sparse.merge_partials(outs, lses, out=res2, lse=res2_l)]
    rows = res_l.numel()
    moved = merge_bytes(N, rows)
    if rate:        # a copy of as many bytes: moved / 2 read and moved / 2 written
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        names.append("copy")
        fns.append(lambda: dst.copy_(src))
    for _ in range(3):
        for f in fns:
            f()
    t_out, t_lse = torch_merge(outs, lses)
    torch.cuda.synchronize()
    diff = float((t_out.float() - res.float()).abs().max())
    ldiff = float((torch.nan_to_num(t_lse, neginf=0.0) - torch.nan_to_num(res_l, neginf=0.0)).abs().max())
    same = bool(torch.equal(res.view(torch.int16), res2.view(torch.int16)) and torch.equal(res_l.view(torch.int32), res2_l.view(torch.int32)))
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    med = {n: statistics.median(r[i] for r in rounds) for i, n in enumerate(names)}
    spread = max(r[0] for r in rounds) - min(r[0] for r in rounds)
    say(f"{name} {list(shape)}, N = {N} ({rows} rows, {moved / 2 ** 20:.2f} MiB to move): torch {1e3 * med['torch']:.1f} us (spread "
        f"{1e3 * spread:.1f}), merge {1e3 * med['merge']:.1f} us, stacked {1e3 * med['merge, stacked']:.1f} us; speedup "
        f"{med['torch'] / med['merge']:.2f}x, faster beyond the spread: {med['torch'] - med['merge'] > spread}; largest |torch - merge|: "
        f"out {diff:.3e}, lse {ldiff:.3e}; list and stacked forms byte-equal: {same}")
    row = dict(name=name, shape=list(shape), N=N, rows=rows, bytes=moved, spread_us=round(1e3 * spread, 2), out_diff=diff, lse_diff=ldiff,
               forms_equal=same, us={n: round(1e3 * t, 2) for n, t in med.items()})
    # the same two forms, each captured in a graph of its own and replayed: the device's time without the host's
    graphs = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for f in fns[:2]:
        with torch.cuda.stream(side):
            f()
        side.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            keep = f()
        graphs.append((gr, keep))
    replays = [gr.replay for gr, _ in graphs]
    for f in replays:
        f()
    grounds = [_round(replays, args.reps) for _ in range(args.rounds)]
    gmed = [statistics.median(r[i] for r in grounds) for i in range(2)]
    gspread = max(r[0] for r in grounds) - min(r[0] for r in grounds)
    say(f"  replayed from a captured graph: torch {1e3 * gmed[0]:.1f} us (spread {1e3 * gspread:.1f}), merge {1e3 * gmed[1]:.1f} us; "
        f"speedup {gmed[0] / gmed[1]:.2f}x, faster beyond the spread: {gmed[0] - gmed[1] > gspread}")
    row["graph_us"] = dict(torch=round(1e3 * gmed[0], 2), merge=round(1e3 * gmed[1], 2), spread=round(1e3 * gspread, 2))
    if rate:
        row["merge_graph_TBps"] = moved / (1e-3 * gmed[1]) / 1e12
    del graphs, replays
    if rate:
        row["merge_TBps"] = moved / (1e-3 * med["merge"]) / 1e12
        row["torch_TBps"] = moved / (1e-3 * med["torch"]) / 1e12
        row["copy_TBps"] = moved / (1e-3 * med["copy"]) / 1e12
        say(f"  bytes the merge must move per second: merge {row['merge_TBps']:.2f} TB/s ({row['merge_graph_TBps']:.2f} replayed), torch {row['torch_TBps']:.2f} TB/s (it moves "
            f"more than that: its fp32 temporaries); a device copy of as many bytes: {1e3 * med['copy']:.1f} us = {row['copy_TBps']:.2f} "
            f"TB/s; merge / copy = {med['merge'] / med['copy']:.2f}")
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0), rows=[])
    say(f"merge_partials against the torch expression of its contract: bf16, H = {H}, D = {D}; {args.rounds} rounds x {args.reps} launches "
        f"per form, interleaved, device events; {res['device']}")
    for T in (8, 576):
        for N in (2, 8):
            res["rows"].append(shape_row(say, args, "serving step, packed", (T, H, D), N))
    res["rows"].append(shape_row(say, args, "HBM-sized, padded", (1, H, 32768, D), 2, rate=True))
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
