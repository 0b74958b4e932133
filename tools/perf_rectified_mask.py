#!/usr/bin/env python3
"""Rectified attention over a caller's block mask at the HunyuanVideo 720p shape (the bench headline: [1, 24, 115456, 128] bf16,
regime R2: top_k 90, p 0, no neighbours), the mask being the selection's own, on one device, in one process:

  (a) rsa_select_from_mask (select_from_mask_kernel) against K3 (rsa_select_mask: select_mask_kernel), both after the same K2.
      Device events around loops of 20 launches from Python bound the kernels from above (host enqueue included); the kernel
      times come from a kernel trace of a run of its own:
      `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_rectified_mask.py`;
  (b) the whole masked call (K1, K2, rsa_select_from_mask, K4, K5) against the rectified call (K1..K5): medians of device events,
      interleaved with the order alternating.  Both outputs are checked byte for byte first.

Prints one line per measurement and a final JSON line; --out FILE writes the JSON there too.

    python tools/perf_rectified_mask.py [--reps 20] [--out profiles/rectified_mask_perf.json]
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
import bench  # noqa: E402
from rectified_spaattn_amd import _core, _lib, block_sparse  # noqa: E402


def _ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _median_ms(pairs):
    return statistics.median(a.elapsed_time(c) for a, c in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["hunyuan_720p_128f"]
    spec = bench.make_spec(wl)
    H = wl["H"]
    q, k, v = bench.gen_inputs(wl, H, 0, dev, "iid")
    L = _lib.lib()

    rect = _core.StagedCall(q, k, v, spec, wl["top_k"], 0.0, None)
    rect.select()
    rect.attend()
    mask = block_sparse.lists_to_block_mask(rect.bufs["bitmask"], 1, H, spec.NBv, spec.NB_total)
    masked = _core.StagedCall(q, k, v, spec, 0, 0.0, None, block_mask=mask)
    masked.select()
    masked.attend()
    torch.cuda.synchronize()
    same = torch.equal(rect.out.view(torch.int16), masked.out.view(torch.int16)) and all(
        torch.equal(rect.bufs[n], masked.bufs[n]) for n in ("probs", "w", "R", "comp", "bitmask", "counts"))
    if not same:
        raise SystemExit("the masked call on the selection's own mask differs from the rectified call")
    kept = float(rect.bufs["counts"].sum()) / (H * spec.NBv * spec.NB_total)

    # ---- (a) the select passes alone, after the same K2 (scores / unrel in each call's own buffers) ----
    lay = ctypes.byref(rect.lay)
    cb_r, cb_m = ctypes.byref(rect.cb), ctypes.byref(masked.cb)
    mp, ms = masked.mask.data_ptr(), masked.mask_strides

    def k3x20():
        for _ in range(20):
            _lib.check(L.rsa_select_mask(lay, None, wl["top_k"], 0.0, cb_r, _core._stream()), "rsa_select_mask")

    def maskx20():
        for _ in range(20):
            _lib.check(L.rsa_select_from_mask(lay, mp, *ms, cb_m, _core._stream()), "rsa_select_from_mask")

    k3x20()
    maskx20()
    torch.cuda.synchronize()
    ek3, emask = [], []
    for i in range(args.reps):
        for fn, acc in ((k3x20, ek3), (maskx20, emask)) if i % 2 else ((maskx20, emask), (k3x20, ek3)):
            acc.append(_ev(fn))
    torch.cuda.synchronize()
    k3_us, mask_us = _median_ms(ek3) * 1e3 / 20, _median_ms(emask) * 1e3 / 20
    BH, NBv, NS, Lr, NB = H, spec.NBv, spec.NBv + spec.n_txt, spec.L, spec.NB_total
    moved = BH * NBv * (NS * 4 + NBv + NB + 2 * Lr * 4 + 4 + (NB + 31) // 32 * 4 + 4) + int(rect.bufs["counts"].sum()) * 4
    print(f"select passes [1,{H},{NBv},{NB}] ({kept:.3f} kept): K3 rsa_select_mask {k3_us:.1f} us, rsa_select_from_mask "
          f"{mask_us:.1f} us per launch in loops of 20 (medians of {args.reps}, interleaved; host enqueue included, kernel times: "
          f"see the trace); the masked pass moves {moved / 1e6:.1f} MB")

    # ---- (b) the whole layer ----
    def rect_layer():
        rect.select()
        rect.attend()

    def masked_layer():
        masked.select()
        masked.attend()

    for _ in range(2):
        rect_layer()
        masked_layer()
    torch.cuda.synchronize()
    er, em = [], []
    for i in range(args.reps):
        for fn, acc in ((rect_layer, er), (masked_layer, em)) if i % 2 else ((masked_layer, em), (rect_layer, er)):
            acc.append(_ev(fn))
    torch.cuda.synchronize()
    rect_ms, masked_ms = _median_ms(er), _median_ms(em)
    print(f"layer: rectified {rect_ms:.3f} ms, masked {masked_ms:.3f} ms, masked / rectified = {masked_ms / rect_ms:.4f} "
          f"(medians of {args.reps}, interleaved); outputs byte-identical")
    res = dict(shape=[1, H, spec.S, 128], regime="r2", top_k=wl["top_k"], kept=round(kept, 4),
               k3_loop_us=round(k3_us, 2), select_from_mask_loop_us=round(mask_us, 2), select_from_mask_mb=round(moved / 1e6, 1),
               layer_rectified_ms=round(rect_ms, 4), layer_masked_ms=round(masked_ms, 4),
               masked_over_rectified=round(masked_ms / rect_ms, 4), identical=same, reps=args.reps,
               device=torch.cuda.get_device_name(dev))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
