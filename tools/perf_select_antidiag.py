#!/usr/bin/env python3
"""select_blocks_antidiag beside the torch composition it replaces, beside select_blocks and beside the block_sparse_attention call it
feeds, on one device (the methodology of tools/perf_pooled_select.py): device events, all forms of a shape
interleaved in one process, --rounds rounds of --reps launches each, one median per form and round, the median of those reported,
next to the device's own box_ref.  Every row runs in a child process of its own under a time limit; the first that fails ends the run.

Shape: B = 1, H = 32 over Hkv = 8, D = 128, bf16, causal, 128-token blocks, top_k 64 with top_p 0.9, keep_first = keep_local = 1;
S = 32768 and 131072, stride 8 and 16.  The torch composition (reshape, flip, matmul, masked softmax, block sums, topk,
block_mask_to_lists) runs head by head over chunks of query groups so that its logits fit; where it still does not, the row says so.
The score pass's share of the MFMA peak counts 2 H Sq Sk D / s causal-halved flops per walk, two walks, against --peak TFLOP/s.

    python tools/perf_select_antidiag.py [--reps 4] [--rounds 5] [--out profiles/select_antidiag_perf.txt]
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

from perf_pooled_select import _round, box_ref  # noqa: E402

ROWS = [(f"S{S}-s{s}", S, s) for S in (32768, 131072) for s in (8, 16)]
B, H, HKV, D, BLK, TOP_K = 1, 32, 8, 128, 128, 64


def torch_composition(torch, q, k, s, chunk=2048):
    """The mask by torch: per head and chunk of row groups the strided logits, the causal softmax and the block sums; then topk."""
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    S, G = q.shape[2], BLK // s
    NQ = NK = S // BLK
    kr = k[0].view(HKV, S // s, s * D)
    w = torch.arange(S // s, device=q.device)[None, :]
    P = torch.zeros(HKV, NQ, NK, device=q.device)
    for h in range(H):
        qr = q[0, h].view(S // s, s, D).flip(1).reshape(S // s, s * D)
        for u0 in range(0, S // s, chunk):
            x = (qr[u0:u0 + chunk] @ kr[h // (H // HKV)].T).float() * (D ** -0.5 / s)
            u = torch.arange(u0, u0 + x.shape[0], device=q.device)[:, None]
            p = torch.softmax(x.masked_fill(w > u, -torch.inf), -1)
            P[h // (H // HKV), u0 // G:(u0 + x.shape[0]) // G] += p.view(-1, G, NK, G).sum((1, 3))
    t = torch.log(P.clamp_min(2.0 ** -126))
    idx = t.topk(TOP_K, -1).indices
    mask = torch.zeros(1, HKV, NQ, NK, dtype=torch.bool, device=q.device).scatter_(-1, idx[None], True)
    return block_mask_to_lists(mask, 1, HKV)


def shape_row(say, args, name, S, s):
    import torch
    from rectified_spaattn_amd import block_sparse_attention, select_blocks, select_blocks_antidiag
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(S + s)
    q = torch.randn(B, H, S, D, device=dev, generator=g).to(torch.bfloat16)
    k, v = (torch.randn(B, HKV, S, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    kw = dict(causal=True, keep_first=1, keep_local=1)
    mask = select_blocks_antidiag(q, k, TOP_K, stride=s, top_p=0.9, **kw)
    fns = [lambda: select_blocks_antidiag(q, k, TOP_K, stride=s, top_p=0.9, **kw), lambda: select_blocks(q, k, TOP_K, **kw),
           lambda: block_sparse_attention(q, k, v, mask, causal=True)]
    names = ["select_blocks_antidiag", "select_blocks", "block_sparse_attention"]
    try:
        torch_composition(torch, q, k, s)
        fns.append(lambda: torch_composition(torch, q, k, s))
        names.append("torch composition")
    except torch.cuda.OutOfMemoryError:
        say(f"{name}: the torch composition does not fit on the device at this shape: not run")
    for f in fns:
        f()
    torch.cuda.synchronize()
    rounds = [_round(torch, fns, args.reps) for _ in range(args.rounds)]
    med = [1e3 * statistics.median(r[i] for r in rounds) for i in range(len(fns))]
    spread = [1e3 * (max(r[i] for r in rounds) - min(r[i] for r in rounds)) for i in range(len(fns))]
    flops = 2 * (2.0 * H * S * S * D / s / 2)
    say(f"{name}: S = {S}, stride {s}; kept fraction {float(mask.float().mean()):.3f}")
    for n, m, sp in zip(names, med, spread):
        say(f"  {n}: {m:.1f} us (spread {sp:.1f} us): {m / med[0]:.2f} x the anti-diagonal call")
    say(f"  both walks: {flops / 1e12:.2f} TFLOP in at most {med[0]:.1f} us: at least {flops / med[0] / 1e6 / args.peak:.3f} of the "
        f"{args.peak} TFLOP/s MFMA peak (the selection launch is inside the time)")
    return dict(name=name, S=S, stride=s, us={n: round(m, 2) for n, m in zip(names, med)},
                spread_us={n: round(x, 2) for n, x in zip(names, spread)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--peak", type=float, default=2500.0, help="dense bf16 MFMA peak of the device, TFLOP/s")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process (one row) may take")
    ap.add_argument("--row", default=None, help="(internal) run this one row in this process and print its JSON as the last line")
    args = ap.parse_args()
    if args.row:
        say = lambda x: print(x, flush=True)      # noqa: E731
        res = box_ref(say, args) if args.row == "box_ref" else shape_row(say, args, *[r for r in ROWS if r[0] == args.row][0])
        print("JSON " + json.dumps(res), flush=True)
        return 0
    lines, res, status = [], dict(reps=args.reps, rounds=args.rounds, rows=[]), 0

    def say(x):
        print(x, flush=True)
        lines.append(x)
    say(f"select_blocks_antidiag: bf16, B = {B}, H = {H} over Hkv = {HKV}, D = {D}, causal, {BLK}-token blocks, top_k {TOP_K}, top_p "
        f"0.9; {args.rounds} rounds x {args.reps} launches per form, interleaved")
    for name in ["box_ref"] + [r[0] for r in ROWS]:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--reps", str(args.reps), "--rounds", str(args.rounds),
               "--peak", str(args.peak)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            say(f"{name}: no result within {args.limit} s; the run ends here")
            status = 1
            break
        out = p.stdout.splitlines()
        for x in out:
            if not x.startswith("JSON "):
                say(x)
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
