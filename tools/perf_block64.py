#!/usr/bin/env python3
"""64- against 128-token blocks on one device, interleaved in one process: K5 (rsa_block_sparse_fwd[_ex]) and the selection
pass (K2 + K3 + K4, and K1) of one call per shape and block size, the same inputs at both block sizes.  Prints one line per
(shape, block) with ms, algorithmic TFLOP/s (4 D b^2 per kept (query block, key block) pair + the dense text rows) and the
fraction of the 2.5 PF dense bf16 peak; the last line is JSON.

    python tools/perf_block64.py            # all shapes;  RSA_PERF_SHAPES=hunyuan_r2,flux to choose
    python tools/perf_block64.py pmc        # a few launches of ONE shape (RSA_PERF_SHAPES) at RSA_PERF_BLOCK (default 64),
                                            # for rocprofv3 --pmc passes: bash tools/pmc_traffic.sh <dir> <shape> "" b64

At block 64 one K5 workgroup runs the MFMAs of its two query blocks over the UNION of their lists (the tiles only one of
them kept are masked, not skipped): `mfma_factor` = issued matrix work / algorithmic work = 2 |union| / (|list 2i| + |list 2i+1|)
summed over the pairs.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import gen_inputs  # noqa: E402
from rectified_spaattn_amd import _core, synth  # noqa: E402
from rectified_spaattn_amd.utils import jenga_gilbert  # noqa: E402

PEAK = 2.5e15
# name -> workload (bench.WORKLOADS conventions), centroid model, neighbours, p_remain, kept fraction of the visual blocks
SHAPES = {
    # HunyuanVideo 720p 128 frames (the bench headline shape): exactly 10 % of the visual blocks per row, no neighbours
    "hunyuan_r2": (dict(H=24, S_vis=115200, text=256, text_valid=200, variant="hunyuan", latent=(32, 45, 80)), "iid", "none",
                   0.0, 0.10),
    # ... the same with Gilbert-curve neighbours and spatially smooth centroids (adjacent blocks' lists overlap)
    "hunyuan_gilbert": (dict(H=24, S_vis=115200, text=256, text_valid=200, variant="hunyuan", latent=(32, 45, 80)), "spatial",
                        "gilbert", 0.05, 0.10),
    # Flux 1024^2 (4096 image tokens + 512 text), Wan2.1 480p 81 frames (21 x 30 x 52 latent)
    "flux": (dict(H=24, S_vis=4096, text=512, text_valid=512, variant="flux", latent=(1, 64, 64)), "iid", "none", 0.0, 0.3),
    "wan480": (dict(H=40, S_vis=32760, text=0, text_valid=0, variant="wan", latent=(21, 30, 52)), "iid", "gilbert", 0.05, 0.3),
}


def spec_of(wl, block):
    S = wl["S_vis"] + wl["text"]
    if wl["variant"] == "hunyuan":
        return _core.LayoutSpec.hunyuan(S, wl["S_vis"] + wl["text_valid"], block=block)
    if wl["variant"] == "flux":
        return _core.LayoutSpec.flux(S, wl["text"], block=block)
    return _core.LayoutSpec.wan(S, 0, block=block)


def timeit(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2]


def pmc():
    """Three select + K5 launches of one shape at one block size and nothing else (counter passes)."""
    dev = torch.device("cuda:0")
    name = os.environ.get("RSA_PERF_SHAPES", "hunyuan_r2").split(",")[0]
    blk = int(os.environ.get("RSA_PERF_BLOCK", "64"))
    wl, cent, nbr_kind, p, frac = SHAPES[name]
    q, k, v = gen_inputs(wl, wl["H"], 0, dev, cent, D=128)
    spec = spec_of(wl, blk)
    nbr = (jenga_gilbert.gilbert_block_neighbor_mapping(*wl["latent"], block_size=blk, axis_order=("w", "h", "t"))
           if nbr_kind == "gilbert" else None)
    call = _core.StagedCall(q, k, v, spec, max(1, int(round(frac * spec.NBv))), p, nbr)
    for _ in range(3):
        call.select()
        call.attend()
    torch.cuda.synchronize()


def main():
    if sys.argv[1:] == ["pmc"]:
        return pmc()
    dev = torch.device("cuda:0")
    names = os.environ.get("RSA_PERF_SHAPES", ",".join(SHAPES)).split(",")
    rounds = int(os.environ.get("RSA_PERF_ROUNDS", "3"))
    res = {}
    for name in names:
        wl, cent, nbr_kind, p, frac = SHAPES[name]
        H, D = wl["H"], 128
        q, k, v = gen_inputs(wl, H, 0, dev, cent, D=D)
        calls = {}
        for blk in (128, 64):
            spec = spec_of(wl, blk)
            if nbr_kind == "gilbert":
                nbr = jenga_gilbert.gilbert_block_neighbor_mapping(*wl["latent"], block_size=blk, axis_order=("w", "h", "t"))
            else:
                nbr = None
            call = _core.StagedCall(q, k, v, spec, max(1, int(round(frac * spec.NBv))), p, nbr)
            call.select()
            torch.cuda.synchronize()
            pairs = float(call.bufs["counts"].sum().item())
            mfma = 1.0
            if blk == 64:
                kept = _core.unpack_bitmask(call.bufs["bitmask"], spec.NB_total)     # [BH, NBv, NB]
                if spec.NBv % 2:
                    kept = torch.cat([kept, torch.zeros_like(kept[:, :1])], 1)
                union = (kept[:, 0::2] | kept[:, 1::2]).sum().item()
                mfma = 2.0 * union / pairs
            flops = 4.0 * D * blk * blk * pairs + 4.0 * D * spec.q_text_valid * spec.kv_text_valid * H
            calls[blk] = (call, spec, flops, pairs / (H * spec.NBv * spec.NB_total), mfma)
        t = {blk: dict(k5=[], sel=[], k1=[]) for blk in calls}
        for _ in range(rounds):   # interleaved: 128, 64, 128, 64, ...
            for blk, (call, spec, flops, kept, mfma) in calls.items():
                t[blk]["k5"].append(timeit(call.attend))
                t[blk]["sel"].append(timeit(call.select_rest))
                t[blk]["k1"].append(timeit(call.select_pool))
        for blk, (call, spec, flops, kept, mfma) in calls.items():
            k5 = sorted(t[blk]["k5"])[len(t[blk]["k5"]) // 2]
            sel = sorted(t[blk]["sel"])[len(t[blk]["sel"]) // 2]
            k1 = sorted(t[blk]["k1"])[len(t[blk]["k1"]) // 2]
            tf = flops / (k5 * 1e-3) / 1e12
            res[f"{name}_b{blk}"] = dict(k5_ms=round(k5, 3), k2_k3_k4_ms=round(sel, 3), k1_ms=round(k1, 3),
                                          tflops=round(tf, 1), peak_frac=round(tf * 1e12 / PEAK, 3), kept=round(kept, 4),
                                          mfma_factor=round(mfma, 3),
                                          flop=flops, NBv=spec.NBv)
            print(f"{name:16s} block {blk:3d}: K5 {k5:8.3f} ms  {tf:7.1f} TFLOP/s = {tf * 1e12 / PEAK:.3f} of peak  "
                  f"K2-K4 {sel:7.3f} ms  K1 {k1:6.3f} ms  kept {kept:.4f}  mfma x{mfma:.3f}  ({flops:.3e} FLOP)", flush=True)
        del calls, q, k, v
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
