#!/usr/bin/env python3
"""block_sparse_attention_backward (rsa_block_sparse_bwd) measured two ways, on one device, in one process,
medians of device-event timings over interleaved rounds (the methodology of tools/perf_merge.py).

(a) Against what a caller runs without it: torch autograd of scaled_dot_product_attention with the expanded dense bool mask, on the
    same tensors.  B = 1, H = 32 over Hkv = 8, D = 128, bf16, S = 8192, causal, select_blocks masks at top_k 8 and 16 (per K/V head).
    The K/V heads are the batch of the torch call ([Hkv, H / Hkv, S, D] beside a [Hkv, 1, S, S] mask), so the mask is not repeated per
    query head.  Timed: the backward alone on both sides (torch.autograd.grad of a kept graph; the explicit backward call, lists
    included) and, for the record, both forwards.  The expectation to report against: "faster than that baseline".
(b) At S = 32768 on its own: the three kernels' times (torch.profiler's device records), the fraction of the 2-byte MFMA peak with
    FLOPs counted as 2 * 5 products x kept tiles x 128 * 128 * D (the kernels run eight products a tile: the fraction counts the
    useful five), and the backward / forward time ratio against block_sparse_attention on the same mask.

    python tools/perf_bwd.py [--reps 5] [--rounds 5] [--out profiles/bwd_perf.txt]
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

H, HKV, D, BLK = 32, 8, 128, 128
PEAK = 2.5e15       # dense bf16 MFMA rate of the MI355X (datasheet)


def _ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _round(fns, reps):
    evs = [[] for _ in fns]
    for i in range(reps):
        for j in range(len(fns)):
            w = (i + j) % len(fns)
            evs[w].append(_ev(fns[w]))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) for e in evs]


def measure(fns, args):
    for f in fns:
        f()
        f()
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    med = [statistics.median(r[i] for r in rounds) for i in range(len(fns))]
    spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(len(fns))]
    return med, spread


def inputs(S, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    mk = lambda h: torch.randn((1, h, S, D), device=dev, generator=g).to(torch.bfloat16)     # noqa: E731
    return mk(H), mk(HKV), mk(HKV), mk(H)


def kept_tiles(mask):
    return int(mask.sum().item()) * (H // mask.shape[1])


def against_torch(say, args, S, top_k):
    q, k, v, dout = inputs(S, top_k)
    mask = block_sparse.select_blocks(q, k, top_k, block_size=BLK, causal=True, keep_first=1, keep_local=1)
    opts = dict(block_size=BLK, causal=True)
    out = block_sparse.block_sparse_attention(q, k, v, mask, **opts)
    # the dense form: the K/V heads as the batch, one [S, S] bool mask per K/V head
    g = H // HKV
    r = torch.arange(S, device=q.device)
    dense = mask[0].repeat_interleave(BLK, 1).repeat_interleave(BLK, 2)[:, :S, :S] & (r[None, :, None] >= r[None, None, :])
    dense = dense[:, None]
    qt = q[0].view(HKV, g, S, D).clone().requires_grad_()
    kt, vt = (t[0][:, None].clone().requires_grad_() for t in (k, v))
    dt = dout[0].view(HKV, g, S, D)
    sdpa = torch.nn.functional.scaled_dot_product_attention
    ot = sdpa(qt, kt.expand(HKV, g, S, D), vt.expand(HKV, g, S, D), attn_mask=dense)
    fns = [lambda: torch.autograd.grad(ot, (qt, kt, vt), dt, retain_graph=True),
           lambda: block_sparse.block_sparse_attention_backward(dout, q, k, v, out, mask, **opts),
           lambda: sdpa(qt, kt.expand(HKV, g, S, D), vt.expand(HKV, g, S, D), attn_mask=dense),
           lambda: block_sparse.block_sparse_attention(q, k, v, mask, **opts)]
    med, spread = measure(fns, args)
    tq, tk, tv = fns[0]()
    dq, dk, dv = fns[1]()
    torch.cuda.synchronize()
    diff = [float((a.float().reshape(-1) - b.float().reshape(-1)).abs().max()) for a, b in ((tq, dq), (tk, dk), (tv, dv))]
    density = kept_tiles(mask) / (H * (S // BLK) * (S // BLK + 1) / 2)
    faster = med[0] - med[1] > max(spread[0], spread[1])
    say(f"(a) S = {S}, top_k = {top_k} ({density:.3f} of the causal tiles kept): backward torch {med[0]:.2f} ms (spread {spread[0]:.2f}), "
        f"sparse {med[1]:.2f} ms (spread {spread[1]:.2f}): {med[0] / med[1]:.2f}x, sparse faster beyond the spread: {faster}; forward "
        f"torch {med[2]:.2f} ms, sparse {med[3]:.2f} ms; largest |torch - sparse|: dq {diff[0]:.3e}, dk {diff[1]:.3e}, dv {diff[2]:.3e}")
    return dict(S=S, top_k=top_k, density=density, ms=dict(torch_bwd=med[0], sparse_bwd=med[1], torch_fwd=med[2], sparse_fwd=med[3]),
                spread_ms=spread, faster=bool(faster), diff=diff)


def kernel_times(fn, names):
    """Median device time (ms) of each kernel whose name holds one of `names`, over a few profiled calls; None if the profiler
    attributes nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        got = {n: [] for n in names}
        for e in prof.events():
            for n in names:
                if n in e.name and getattr(e, "device_time", 0) > 0:
                    got[n].append(e.device_time / 1e3)
        return {n: (statistics.median(t) if t else None) for n, t in got.items()}
    except Exception as exc:      # the tool still reports the totals
        print(f"(no per-kernel times: {exc!r})")
        return {n: None for n in names}


def alone(say, args, S, top_k):
    q, k, v, dout = inputs(S, 100 + top_k)
    mask = block_sparse.select_blocks(q, k, top_k, block_size=BLK, causal=True, keep_first=1, keep_local=1)
    opts = dict(block_size=BLK, causal=True)
    out = block_sparse.block_sparse_attention(q, k, v, mask, **opts)
    fns = [lambda: block_sparse.block_sparse_attention_backward(dout, q, k, v, out, mask, **opts),
           lambda: block_sparse.block_sparse_attention(q, k, v, mask, **opts)]
    med, spread = measure(fns, args)
    tiles = kept_tiles(mask)
    flops = 2 * 5 * tiles * BLK * BLK * D
    kt = kernel_times(fns[0], ("bwd_row_kernel", "bwd_dq_kernel", "bwd_dkdv_kernel"))
    ks = ", ".join(f"{n} {t:.2f} ms" if t is not None else f"{n} n/a" for n, t in kt.items())
    say(f"(b) S = {S}, top_k = {top_k} ({tiles} kept tiles): backward {med[0]:.2f} ms (spread {spread[0]:.2f}) = "
        f"{flops / (1e-3 * med[0]) / 1e12:.1f} TFLOP/s of the five useful products = {flops / (1e-3 * med[0]) / PEAK:.3f} of the 2-byte "
        f"MFMA peak; kernels: {ks}; forward {med[1]:.2f} ms (spread {spread[1]:.2f}); backward / forward = {med[0] / med[1]:.2f}")
    return dict(S=S, top_k=top_k, tiles=tiles, flops=flops, ms=dict(bwd=med[0], fwd=med[1]), spread_ms=spread, kernels_ms=kt,
                peak_fraction=flops / (1e-3 * med[0]) / PEAK)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0), rows=[])
    say(f"block_sparse_attention_backward: bf16, B = 1, H = {H} over Hkv = {HKV}, D = {D}, causal, 128-token blocks; {args.rounds} rounds x "
        f"{args.reps} calls per form, interleaved, device events; {res['device']}")
    for top_k in (8, 16):
        res["rows"].append(against_torch(say, args, 8192, top_k))
    for top_k in (8, 16):
        res["rows"].append(alone(say, args, 32768, top_k))
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
