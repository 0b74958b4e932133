#!/usr/bin/env python3
"""Per-row key ranges of block_sparse_attention (causal= / window= / row_range=; the RANGED instantiations of the 64-row K5), on
one device, interleaved in one process, medians of device-event timings, next to that device's own box_ref (dense attention
1 x 24 x 16384 x 128 bf16 through the same kernel, as bench.py measures it):

  (a) causal over an ALL-ONES block mask at S = 16 384, 24 heads, D = 128, bf16, against rsa_dense_causal_fwd on the same shape:
      the dense kernel doing the same arithmetic (in 256-row tiles) -- the ratio is what the list walk and the trim cost;
  (b) the HunyuanVideo 720p plain launch of tools/perf_block_mask.py (the selection pass's own lists at top_k 90) with neutral
      ranges (lo = 0, hi = kv_valid for every row) against without: what the ranged prologue costs a walk that needs none of it;
  (c) window (4 680, 0) over an all-ones mask at S = 32 768 against the same call with the block mask cut to the band beforehand:
      what leaving the trim to the kernel costs.

(a) and (c) time the whole Python call (the mask -> list conversion included, on both sides of (c)); (b) times the C entry alone.
Prints one line per measurement and a final JSON line; --out FILE appends the lines there.

    python tools/perf_ranged.py [--reps 20] [--out profiles/ranged_perf.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rectified_spaattn_amd import _core, _lib, block_sparse  # noqa: E402


def _ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _ab(fa, fb, reps):
    """Medians (ms) of fa and fb, interleaved, the order alternating."""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    ea, eb = [], []
    for i in range(reps):
        for which in ((0, 1) if i % 2 else (1, 0)):
            (ea if which == 0 else eb).append(_ev(fa if which == 0 else fb))
    torch.cuda.synchronize()
    return (statistics.median(a.elapsed_time(c) for a, c in ea), statistics.median(a.elapsed_time(c) for a, c in eb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, device=torch.cuda.get_device_name(dev))
    H, D, b = 24, 128, 128

    # ---- box_ref and (a): S = 16 384 ----
    S = 16384
    g = torch.Generator(device=dev).manual_seed(11)
    q = torch.randn(1, H, S, D, device=dev, generator=g).to(torch.bfloat16)
    ones = torch.ones(1, 1, S // b, S // b, dtype=torch.bool, device=dev)
    dense_ms, causal_ms = _ab(lambda: _core.dense_attention(q, q, q), lambda: _core.dense_attention(q, q, q, causal=True), args.reps)
    ranged_ms, causal2_ms = _ab(lambda: block_sparse.block_sparse_attention(q, q, q, ones, causal=True),
                                lambda: _core.dense_attention(q, q, q, causal=True), args.reps)
    flops = 4.0 * S * S * D * H
    say(f"box_ref: dense attention 1 x {H} x {S} x {D} bf16: {dense_ms:.3f} ms = {flops / dense_ms / 1e9:.0f} TFLOP/s")
    say(f"(a) causal, S = {S}: block_sparse_attention(all-ones mask, causal=True) {ranged_ms:.3f} ms; rsa_dense_causal_fwd "
        f"{causal2_ms:.3f} ms ({causal_ms:.3f} beside box_ref); ranged / dense causal = {ranged_ms / causal2_ms:.4f}")
    res.update(box_ref_ms=round(dense_ms, 4), a_ranged_causal_ms=round(ranged_ms, 4), a_dense_causal_ms=round(causal2_ms, 4),
               a_ratio=round(ranged_ms / causal2_ms, 4))
    del q, ones

    # ---- (b): the HunyuanVideo 720p plain launch, neutral ranges against none ----
    wl = bench.WORKLOADS["hunyuan_720p_128f"]
    spec = bench.make_spec(wl)
    Hh, NQ, NK = wl["H"], spec.NBv, spec.NB_total
    q, k, v = bench.gen_inputs(wl, Hh, 0, dev, "iid")
    call = _core.StagedCall(q, k, v, spec, 90, 0.0, None, reuse_buffers=False)
    call.select()
    bufs = call.bufs
    out = torch.empty((1, Hh, NQ * b, 128), dtype=q.dtype, device=dev)
    o4 = _lib.RsaOut4(out.data_ptr(), out.stride(0), out.stride(1), out.stride(2))
    tpart = torch.empty((_lib.TAIL_PIECES, b, 130), dtype=torch.float32, device=dev)
    tq, tk, tv = call.t
    hi = torch.full((1, NQ * b), spec.kv_valid, dtype=torch.int32, device=dev)
    lo = torch.zeros((1, NQ * b), dtype=torch.int32, device=dev)
    head = (1, Hh, NQ * b, spec.S, 128, _core.dtype_code(q.dtype), b, NQ, NK, spec.kv_valid, 128 ** -0.5, tq, tk, tv,
            bufs["cols"].data_ptr(), bufs["counts"].data_ptr())
    tail = (tpart.data_ptr(), tpart.numel() * 4, o4, _core._stream())

    def plain():
        _lib.check(L.rsa_block_sparse_plain_fwd(*head, *tail), "rsa_block_sparse_plain_fwd")

    def neutral():
        _lib.check(L.rsa_block_sparse_ranged_fwd(*head, lo.data_ptr(), hi.data_ptr(), 0, *tail), "rsa_block_sparse_ranged_fwd")

    plain_ms, neutral_ms = _ab(plain, neutral, args.reps)
    say(f"(b) HunyuanVideo 720p plain launch [1,{Hh},{NQ},{NK}], top_k 90: without ranges {plain_ms:.3f} ms; neutral ranges "
        f"{neutral_ms:.3f} ms; ranged / plain = {neutral_ms / plain_ms:.4f}")
    res.update(b_plain_ms=round(plain_ms, 4), b_neutral_ms=round(neutral_ms, 4), b_ratio=round(neutral_ms / plain_ms, 4))
    del q, k, v, call, bufs, out

    # ---- (c): window (4 680, 0) at S = 32 768, all-ones mask against the mask cut to the band ----
    S, left = 32768, 4680
    g = torch.Generator(device=dev).manual_seed(12)
    q = torch.randn(1, H, S, D, device=dev, generator=g).to(torch.bfloat16)
    NB = S // b
    ones = torch.ones(1, 1, NB, NB, dtype=torch.bool, device=dev)
    i = torch.arange(NB, device=dev)
    # block j holds a key some row of block i sees: rows 128 i .. 128 i + 127 see keys r - left .. r
    band = ((i[None, :] * b <= i[:, None] * b + b - 1) & (i[None, :] * b + b - 1 >= i[:, None] * b - left))[None, None]
    full_ms, cut_ms = _ab(lambda: block_sparse.block_sparse_attention(q, q, q, ones, window=(left, 0)),
                          lambda: block_sparse.block_sparse_attention(q, q, q, band, window=(left, 0)), args.reps)
    say(f"(c) window ({left}, 0), S = {S}: all-ones mask (the kernel trims {NB} entries per walk) {full_ms:.3f} ms; mask cut to "
        f"the band ({int(band.sum())} of {NB * NB} blocks) {cut_ms:.3f} ms; all-ones / cut = {full_ms / cut_ms:.4f}")
    res.update(c_all_ones_ms=round(full_ms, 4), c_cut_ms=round(cut_ms, 4), c_ratio=round(full_ms / cut_ms, 4))
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
