#!/usr/bin/env python3
"""The ragged extend call (rsa_block_sparse_extend_ragged[_kv8]) next to what a caller does without it, on
one device, interleaved in one process, medians of device-event timings (the method and the cache of tools/perf_extend.py).

Shapes: bf16 q, D = 128, H = 32 over Hkv = 8, 128-token blocks, B = 8 x 32 768 keys, paged bf16 and e4m3, lists per K/V head from
select_blocks_pooled(causal=True, keep_first=1, keep_local=1, q_len=) at top_k 16 / 64, padded Sq = 512, C entries on prebuilt lists.

  (i)  mixed    one item of 512 rows and seven of one row.  ragged: ONE call on the padded batch, at the library's default split
                (one split: the padded shape has 2048 row groups) and at blocks_per_split = 8.  today: rsa_block_sparse_extend at
                B = 1 (default split) plus rsa_block_sparse_decode at B = 7 (default split), on views of the same cache, table
                rows and q; the decode call's lists are the items' first list rows copied side by side once, outside the timing
                (its entry takes one list row per head, the ragged lists hold four).
  (ii) padding  q_len = 1 everywhere at padded Sq = 512, against rsa_block_sparse_decode at Sq = 1 on the same q rows and lists.

Reported per shape: the median of the rounds' medians of every form, the round-median spread of the reference form (today's two
calls; decode), the ratios, and whether the ragged output's live rows are the reference's bytes.

    python tools/perf_ragged.py [--reps 5] [--rounds 3] [--out profiles/extend_ragged_perf.txt]

The existing extend and select entries run the parent's kernels (the ragged ones are instantiations of their own), so there is no
A/B against another build here.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import perf_extend as pe  # noqa: E402
from rectified_spaattn_amd import _core, _lib, block_sparse  # noqa: E402

H, HKV, D, BLK = pe.H, pe.HKV, pe.D, pe.BLK
SQ = 512


def _o4(t):
    return _lib.RsaOut4(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


class Calls:
    """The C entries of one library over one cache form, on prebuilt lists."""

    def __init__(self, L, cache, form):
        self.L, self.c, self.form = L, cache, form
        self.kp, self.vp = cache.pools[form]
        self.tail = (cache.scales[0].data_ptr(), cache.scales[1].data_ptr()) if form == "e4m3" else ()
        self.sfx = "_kv8" if form == "e4m3" else ""
        self.st = _core._stream()

    def attend(self, entry, q, b0, B, Sq, cols, counts, bps, out, q_len=None):
        """entry: "extend" | "extend_ragged" | "decode" on batch items [b0, b0 + B) of the cache; -> the launch."""
        c, L = self.c, self.L
        need = ctypes.c_size_t(0)
        if entry == "decode":
            _lib.check(L.rsa_block_sparse_decode_bytes(B, H, HKV, HKV, Sq, D, c.NK, bps, ctypes.byref(need)), "decode_bytes")
        else:
            _lib.check(L.rsa_block_sparse_extend_bytes(B, H, HKV, HKV, Sq, D, BLK, c.NK, bps, ctypes.byref(need)), "extend_bytes")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=q.device)
        name = "rsa_block_sparse_" + entry + self.sfx
        table = c.table[b0:b0 + B]
        tq, tk, tv, o4 = _core._t4(q), _core._t4(self.kp), _core._t4(self.vp), _o4(out)
        extra = (q_len.data_ptr(),) if entry == "extend_ragged" else ()
        fn = getattr(L, name)

        def run():
            rc = fn(B, H, HKV, HKV, Sq, c.Sk, D, _lib.RSA_BF16, BLK, c.NK, None, c.Sk, 1, D ** -0.5, tq, tk, tv, table.data_ptr(),
                    c.NK, c.B * c.NK, cols.data_ptr(), counts.data_ptr(), bps, ws.data_ptr(), need.value, o4, None, *self.tail,
                    *extra, self.st)
            assert rc == 0, (name, rc)
        run.keep = (ws, table, q_len)
        return run


def _measure(names, fns, args):
    for _ in range(2):
        for f in fns:
            f()
    torch.cuda.synchronize()
    rounds = [pe._round(fns, args.reps) for _ in range(args.rounds)]
    med = {n: statistics.median(r[i] for r in rounds) for i, n in enumerate(names)}
    spread = {n: max(r[i] for r in rounds) - min(r[i] for r in rounds) for i, n in enumerate(names)}
    return med, spread


def shape_rows(say, args, cache, form, top_k):
    dev = torch.device("cuda:0")
    B, NK = cache.B, cache.NK
    NQ = SQ // BLK
    calls = Calls(_lib.lib(), cache, form)
    q = torch.randn(B, H, SQ, D, device=dev, generator=cache.gen).to(torch.bfloat16)
    sel = dict(causal=True, keep_first=1, keep_local=1, as_lists=True)
    res = []
    for label, ns in (("(i) mixed: q_len = 512, 1 x 7", [SQ] + [1] * (B - 1)), ("(ii) padding: q_len = 1 x 8", [1] * B)):
        q_len = torch.tensor(ns, dtype=torch.int32, device=dev)
        lists = block_sparse.select_blocks_pooled(q, cache.pooled[form], top_k, q_len=q_len, **sel)
        cols, counts = lists["cols"], lists["counts"]          # [B * HKV, NQ, NK], [B * HKV, NQ]
        out_r, out_r8, out_e, out_d = (torch.zeros((B, H, SQ, D), dtype=q.dtype, device=dev) for _ in range(4))
        names = ["ragged", "ragged/8"]
        fns = [calls.attend("extend_ragged", q, 0, B, SQ, cols, counts, 0, out_r, q_len),
               calls.attend("extend_ragged", q, 0, B, SQ, cols, counts, 8, out_r8, q_len)]
        b0 = 1 if ns[0] == SQ else 0            # the decode items
        cols1 = cols.view(B, HKV, NQ, NK)[b0:, :, 0].contiguous()
        counts1 = counts.view(B, HKV, NQ)[b0:, :, 0].contiguous()
        dec = calls.attend("decode", q[b0:, :, :1], b0, B - b0, 1, cols1, counts1, 0, out_d[b0:, :, :1])
        if b0:
            ext1 = calls.attend("extend", q[:1], 0, 1, SQ, cols, counts, 0, out_e[:1])

            def today():
                ext1()
                dec()
            names += ["today", "extend B=1", "decode B=7"]
            fns += [today, ext1, dec]
            ref = "today"
        else:
            names.append("decode")
            fns.append(dec)
            ref = "decode"
        med, spread = _measure(names, fns, args)
        # the live rows of the ragged call at the reference's split sizes are the reference's bytes (decode: min(8, NK) = ragged/8)
        same_dec = bool(torch.equal(out_r8[b0:, :, :1].view(torch.int16), out_d[b0:, :, :1].view(torch.int16)))
        same_ext = bool(torch.equal(out_r[:1].view(torch.int16), out_e[:1].view(torch.int16))) if b0 else None
        zero = bool((out_r[b0:, :, 1:] == 0).all())
        us = {n: round(1e3 * t, 2) for n, t in med.items()}
        say(f"B = {B} x {cache.Sk} keys, {form} paged, top_k = {top_k}, padded Sq = {SQ}; {label}; "
            f"{block_sparse.extend_row_groups(B, H, HKV, HKV, SQ, BLK)['groups']} row groups, kept pairs {int(counts.sum())}")
        say("  " + ";  ".join(f"{n}: {us[n]:.1f} us" for n in names) + f"  (round-median spread of {ref}: {1e3 * spread[ref]:.1f} us, "
            f"of ragged: {1e3 * spread['ragged']:.1f} us)")
        say(f"  ragged / {ref} = {med['ragged'] / med[ref]:.2f}, ragged/8 / {ref} = {med['ragged/8'] / med[ref]:.2f}; decode rows "
            f"byte-equal at split 8: {same_dec}" + (f"; the chunk's rows byte-equal to extend B=1: {same_ext}" if b0 else "")
            + f"; padding rows zero: {zero}")
        res.append(dict(form=form, top_k=top_k, case=label, us=us, spread_us={n: round(1e3 * s, 2) for n, s in spread.items()},
                        same_decode=same_dec, same_extend=same_ext, padding_zero=zero))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--top-ks", default="16,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    say(f"ragged extend against today's calls: bf16 q, D = {D}, H = {H} over Hkv = {HKV}, {BLK}-token blocks, causal, B = 8 x 32768 "
        f"keys paged, padded Sq = {SQ}; {args.rounds} rounds x {args.reps} launches per form, interleaved")
    cache = pe.Cache(8, 32768, torch.device("cuda:0"))
    res["rows"] = []
    for form in ("bf16", "e4m3"):
        for top_k in [int(x) for x in args.top_ks.split(",")]:
            res["rows"] += shape_rows(say, args, cache, form, top_k)
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
