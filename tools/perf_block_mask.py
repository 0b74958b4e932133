#!/usr/bin/env python3
"""Caller-supplied block masks at the HunyuanVideo 720p shape (the bench headline: 24 heads, 900 visual x 902 key blocks), on one
device, interleaved in one process:

  * rsa_block_mask_to_lists over a [1, 24, 900, 902] bool mask (about 10 % kept), against its traffic (the mask read, the kept
    share of cols, the bitmask and counts written).  Device events around 100 launches from a Python loop (arguments marshalled
    once): that figure is bounded below by the host's enqueue rate, so it is NOT the kernel's time -- take that from a kernel
    trace of the same run, `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_block_mask.py`
    (kernel `block_mask_to_lists_kernel`);
  * K5 through the plain entry (rsa_block_sparse_plain_fwd) against K5 inside the rectified call (rsa_block_sparse_fwd), both over
    the SAME lists: the selection pass's own at top_k 90.  The rectified launch also walks the 2 dense text query blocks of every
    head (902 key blocks each, split-KV + a combine pass) and reads R / comp in its epilogue; the plain launch has no text rows.

Prints one line per measurement and a final JSON line; --out FILE writes the JSON there too.

    python tools/perf_block_mask.py [--reps 30] [--out profiles/block_mask_perf.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["hunyuan_720p_128f"]
    spec = bench.make_spec(wl)
    H, NQ, NK, b = wl["H"], spec.NBv, spec.NB_total, 128
    L = _lib.lib()

    # ---- mask -> lists at [1, 24, 900, 902] ----
    g = torch.Generator(device=dev).manual_seed(1)
    mask = torch.rand((1, H, NQ, NK), generator=g, device=dev) < 0.10
    lists = block_sparse.block_mask_to_lists(mask, 1, H)
    m8 = mask.view(torch.uint8)

    cargs = (1, H, NQ, NK, m8.data_ptr(), m8.stride(0), m8.stride(1), m8.stride(2), lists["bitmask"].data_ptr(),
             lists["cols"].data_ptr(), lists["counts"].data_ptr(), _core._stream())
    fn = L.rsa_block_mask_to_lists

    def convert100():
        for _ in range(100):
            if fn(*cargs):
                raise _lib.RsaError("rsa_block_mask_to_lists failed")

    convert100()
    torch.cuda.synchronize()
    ev = [_ev(convert100) for _ in range(args.reps)]
    torch.cuda.synchronize()
    conv_us = statistics.median(a.elapsed_time(c) for a, c in ev) * 1e3 / 100
    kept = int(lists["counts"].sum())
    moved = m8.numel() + kept * 4 + lists["bitmask"].numel() * 4 + lists["counts"].numel() * 4
    print(f"rsa_block_mask_to_lists [1,{H},{NQ},{NK}]: {conv_us:.2f} us per launch in a loop of 100 (median of {args.reps}; "
          f"host enqueue included, kernel time: see the trace), {moved / 1e6:.1f} MB moved; kept {kept / m8.numel():.3f}")

    # ---- K5: plain entry vs the rectified call, same lists ----
    q, k, v = bench.gen_inputs(wl, H, 0, dev, "iid")
    call = _core.StagedCall(q, k, v, spec, 90, 0.0, None, reuse_buffers=False)
    call.select()
    bufs = call.bufs
    out = torch.empty((1, H, NQ * b, 128), dtype=q.dtype, device=dev)
    o4 = _lib.RsaOut4(out.data_ptr(), out.stride(0), out.stride(1), out.stride(2))
    tpart = torch.empty((_lib.TAIL_PIECES, b, 130), dtype=torch.float32, device=dev)
    tq, tk, tv = call.t

    def plain():
        _lib.check(L.rsa_block_sparse_plain_fwd(1, H, NQ * b, spec.S, 128, _core.dtype_code(q.dtype), b, NQ, NK, spec.kv_valid,
                                                128 ** -0.5, tq, tk, tv, bufs["cols"].data_ptr(), bufs["counts"].data_ptr(),
                                                tpart.data_ptr(), tpart.numel() * 4, o4, _core._stream()),
                   "rsa_block_sparse_plain_fwd")

    for _ in range(3):
        call.attend()
        plain()
    torch.cuda.synchronize()
    rect, pl = [], []
    for i in range(args.reps):   # interleaved, the order alternating
        if i % 2:
            rect.append(_ev(call.attend))
            pl.append(_ev(plain))
        else:
            pl.append(_ev(plain))
            rect.append(_ev(call.attend))
    torch.cuda.synchronize()
    rect_ms = statistics.median(a.elapsed_time(c) for a, c in rect)
    plain_ms = statistics.median(a.elapsed_time(c) for a, c in pl)
    print(f"K5 rectified (rsa_block_sparse_fwd): {rect_ms:.3f} ms; plain (rsa_block_sparse_plain_fwd): {plain_ms:.3f} ms; "
          f"plain / rectified = {plain_ms / rect_ms:.4f} (medians of {args.reps}, interleaved)")
    res = dict(shape=[1, H, NQ, NK], mask_to_lists_loop_us=round(conv_us, 3), mask_to_lists_mb=round(moved / 1e6, 2),
               k5_rectified_ms=round(rect_ms, 4), k5_plain_ms=round(plain_ms, 4),
               plain_over_rectified=round(plain_ms / rect_ms, 4), reps=args.reps, device=torch.cuda.get_device_name(dev))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
