#!/usr/bin/env python3
"""Grouped-query K/V heads of block_sparse_attention (rsa_block_sparse_gqa_fwd), on one device, interleaved in one process,
medians of device-event timings, next to that device's own box_ref (dense attention 1 x 24 x 16384 x 128 bf16 through the same
kernel, as bench.py measures it).

Shape: the HunyuanVideo 720p plain launch of tools/perf_block_mask.py (S = 115 456, D = 128, bf16; the selection pass's own lists
at top_k 90, regime R2: about 10 % of the key blocks kept) with H = 24 query heads over Hkv = 12 K/V heads and one list per K/V head:

  (i)   the MHA entry on repeat_interleave'd K / V and repeated lists -- the only way without the grouped entry;
  (ii)  the grouped entry, form (a): every query head a walk of its own (tuning key k5_gqa_pair = 0);
  (iii) the grouped entry, form (b): two query heads of one K/V head on one K/V ring (k5_gqa_pair = 1).

The three are timed interleaved, the order rotating, in --rounds rounds of --reps launches each; a round gives one median per form.
Reported: the median of the rounds' medians, and the SPREAD of (ii) = the largest minus the smallest of its rounds' medians -- a
difference between two forms below that spread is not a difference.  All three time the C entry alone.  The outputs are compared as
well: (i) against (ii) byte for byte, (iii) against (ii) by the largest difference (this grid has a split tail in (i) and (ii) and
none in (iii), so the rows of the split walks agree within rounding only).
Prints one line per measurement and a final JSON line; --out FILE appends the lines there.

    python tools/perf_gqa.py [--reps 8] [--rounds 5] [--out profiles/gqa_perf.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

os.environ.setdefault("RSA_TUNING", "1")   # (the two forms are chosen through rsa_set_tuning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rectified_spaattn_amd import _core, _lib  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(dev))
    b = 128

    # ---- box_ref ----
    S0 = 16384
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(1, 24, S0, 128, device=dev, generator=g).to(torch.bfloat16)
    for _ in range(2):
        _core.dense_attention(x, x, x)
    torch.cuda.synchronize()
    dense_ms = statistics.median(_round([lambda: _core.dense_attention(x, x, x)], args.reps)[0] for _ in range(3))
    say(f"box_ref: dense attention 1 x 24 x {S0} x 128 bf16: {dense_ms:.3f} ms = {4.0 * S0 * S0 * 128 * 24 / dense_ms / 1e9:.0f} TFLOP/s")
    res.update(box_ref_ms=round(dense_ms, 4))
    del x

    # ---- the HunyuanVideo 720p plain launch, 24 query heads over 12 K/V heads, one list per K/V head ----
    wl = bench.WORKLOADS["hunyuan_720p_128f"]
    spec = bench.make_spec(wl)
    H, Hkv, NQ, NK = 24, 12, spec.NBv, spec.NB_total
    grp = H // Hkv
    q, _, _ = bench.gen_inputs(wl, H, 0, dev, "iid")
    qs, k, v = bench.gen_inputs(wl, Hkv, 0, dev, "iid")
    call = _core.StagedCall(qs, k, v, spec, 90, 0.0, None, reuse_buffers=False)     # the selection of the K/V heads' own queries
    call.select()
    cols, counts = call.bufs["cols"], call.bufs["counts"]
    kept = float(counts.float().mean()) / NK
    kx, vx = k.repeat_interleave(grp, dim=1), v.repeat_interleave(grp, dim=1)
    colsx = cols.view(Hkv, NQ, NK).repeat_interleave(grp, dim=0).contiguous()
    countsx = counts.view(Hkv, NQ).repeat_interleave(grp, dim=0).contiguous()
    outs = [torch.zeros((1, H, NQ * b, 128), dtype=q.dtype, device=dev) for _ in range(3)]
    tpart = torch.empty((_lib.TAIL_PIECES, b, 130), dtype=torch.float32, device=dev)
    dt = _core.dtype_code(q.dtype)
    shape = (NQ * b, spec.S, 128, dt, b, NQ, NK, spec.kv_valid, 128 ** -0.5)
    tail = (tpart.data_ptr(), tpart.numel() * 4)
    o4 = [_lib.RsaOut4(o.data_ptr(), o.stride(0), o.stride(1), o.stride(2)) for o in outs]
    tq, tk, tv, tkx, tvx = (_core._t4(t) for t in (q, k, v, kx, vx))
    st = _core._stream()

    def mha():
        _lib.check(L.rsa_block_sparse_plain_fwd(1, H, *shape, tq, tkx, tvx, colsx.data_ptr(), countsx.data_ptr(), *tail, o4[0], st),
                   "rsa_block_sparse_plain_fwd")

    def gqa(form):
        def run():
            assert L.rsa_set_tuning(b"k5_gqa_pair", form) == 0
            _lib.check(L.rsa_block_sparse_gqa_fwd(1, H, Hkv, Hkv, *shape, tq, tk, tv, cols.data_ptr(), counts.data_ptr(), None, None,
                                                  0, *tail, o4[1 + form], st), "rsa_block_sparse_gqa_fwd")
        return run

    fns = [mha, gqa(0), gqa(1)]
    for _ in range(2):
        for f in fns:
            f()
    torch.cuda.synchronize()
    same_a = torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    diff_b = float((outs[2].float() - outs[1].float()).abs().max())
    rows_b = int((outs[2].view(torch.int16) != outs[1].view(torch.int16)).any(-1).sum())
    finite = bool(torch.isfinite(outs[2].float()).all()) and float(outs[2].float().abs().max()) > 0
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    L.rsa_set_tuning(b"k5_gqa_pair", _lib.GQA_PAIR_DEFAULT)
    med = [statistics.median(r[i] for r in rounds) for i in range(3)]
    spread = max(r[1] for r in rounds) - min(r[1] for r in rounds)
    say(f"HunyuanVideo 720p plain launch, H = {H} over Hkv = {Hkv}, lists per K/V head [{Hkv},{NQ},{NK}], top_k 90 "
        f"({100 * kept:.1f} % of the key blocks kept); {args.rounds} rounds x {args.reps} launches per form, interleaved")
    for name, i in (("(i)   MHA entry, K / V and lists repeated", 0), ("(ii)  grouped entry, form (a), per head", 1),
                    ("(iii) grouped entry, form (b), head pairs", 2)):
        say(f"{name}: {med[i]:.3f} ms   (rounds: {' '.join(f'{r[i]:.3f}' for r in rounds)})")
    say(f"spread of the (ii) medians: {spread:.3f} ms;  (ii) - (i) = {med[1] - med[0]:+.3f} ms;  (iii) - (ii) = {med[2] - med[1]:+.3f} ms "
        f"({100 * (med[2] / med[1] - 1):+.2f} %)")
    say(f"outputs: (ii) == (i) byte for byte: {same_a};  (iii) against (ii): {rows_b} of {H * NQ * b} rows differ, largest difference "
        f"{diff_b:.3e} (split tail in (ii), none in (iii)); (iii) finite and non-zero: {finite}")
    res.update(mha_ms=round(med[0], 4), gqa_head_ms=round(med[1], 4), gqa_pair_ms=round(med[2], 4), spread_ms=round(spread, 4),
               head_equals_mha=same_a, pair_max_diff=diff_b, pair_rows_differing=rows_b, kept_fraction=round(kept, 4))
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
