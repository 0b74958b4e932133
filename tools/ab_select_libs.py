#!/usr/bin/env python3
"""Two builds of librsa_hip.so on the selection unit's kernels, loaded side by side in one process on one device (the methodology of
tools/ab_libs.py and tools/perf_select_bound.py): the shapes of tools/perf_select_bound.py, every form launched from both builds.

    python tools/ab_select_libs.py OTHER_LIBRSA_HIP_SO OUT.md [--rounds 8] [--reps 8]

Forms: the select pass from the mean cache and from the bounds cache at the library's score_splits, the one-block update and the
prefill of both caches, the e4m3 prefills of both, and rsa_block_select (the pool kernel's key jobs).  A round launches all forms of
one build, then all forms of the other, --reps times, the starting form rotating (perf_pooled_select._round); so a launch of either
build follows the same form of the same build, and the rounds alternate which build goes first.  One median per form, build and
round; reported: the median of the rounds, the other build's spread (largest minus smallest round) and whether this tree's build is
slower by more than that spread.  Every output of every form is compared between the builds byte for byte before timing."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from perf_pooled_select import _round  # noqa: E402
from rectified_spaattn_amd import _core, _lib  # noqa: E402

ROWS = [("long-16", 1, 131072), ("batch-16", 8, 32768)]


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def forms(L, B, Sk, q, k, k8, ks, st):
    dev = q.device
    H, Hkv, D, blk, Sq, top_k = 32, 8, 128, 128, 1, 16
    NK, NW = Sk // blk, (Sk // blk + 31) // 32
    dt = _core.dtype_code(q.dtype)
    tq, tk, tk8 = _core._t4(q), _core._t4(k), _core._t4(k8)
    rows = B * Hkv
    bm, cols, cnt = (torch.zeros((rows, 1, NW), dtype=torch.int32, device=dev), torch.zeros((rows, 1, NK), dtype=torch.int32, device=dev),
                     torch.zeros((rows, 1), dtype=torch.int32, device=dev))
    means = torch.zeros((B, Hkv, NK, D), dtype=torch.float32, device=dev)
    bounds = torch.zeros((B, Hkv, NK, 2, D), dtype=torch.float32, device=dev)
    n = ctypes.c_size_t(0)
    assert L.rsa_block_select_bound_bytes(B, Hkv, Hkv, D, 1, NK, ctypes.byref(n)) == 0
    n2 = ctypes.c_size_t(0)
    assert L.rsa_block_select_bytes(B, Hkv, Hkv, D, 1, NK, ctypes.byref(n2)) == 0
    ws = torch.empty((max(n.value, n2.value),), dtype=torch.uint8, device=dev)
    nb = ws.numel()

    def ok(rc):
        assert rc == 0, rc

    def pool(entry, out, start):
        return lambda: ok(getattr(L, entry)(B, Hkv, Sk, D, dt, blk, NK, tk, None, 0, 0, None, Sk, None, start, 0, out.data_ptr(), st))

    def pool8(entry, out):
        return lambda: ok(getattr(L, entry)(B, Hkv, Sk, D, blk, NK, tk8, None, 0, 0, None, Sk, None, 0, 0, out.data_ptr(), ks.data_ptr(), st))

    def sel_mean():
        ok(L.rsa_block_select_pooled(B, H, Hkv, Hkv, Sq, D, dt, blk, 1, NK, tq, means.data_ptr(), None, Sk, 1, top_k, 0, 0, 0,
                                     ws.data_ptr(), nb, bm.data_ptr(), cols.data_ptr(), cnt.data_ptr(), None, st))

    def sel_bound():
        ok(L.rsa_block_select_bound(B, H, Hkv, Hkv, Sq, D, dt, blk, 1, NK, tq, bounds.data_ptr(), None, Sk, 1, top_k, 0, 0, 0,
                                    ws.data_ptr(), nb, bm.data_ptr(), cols.data_ptr(), cnt.data_ptr(), None, -1, 0.0, None, None, st))

    def sel_plain():
        ok(L.rsa_block_select(B, H, Hkv, Hkv, Sq, Sk, D, dt, blk, 1, NK, tq, tk, None, Sk, 1, top_k, 0, 0, ws.data_ptr(), nb,
                              bm.data_ptr(), cols.data_ptr(), cnt.data_ptr(), None, st))
    named = [("select_pooled", sel_mean), ("select_bound", sel_bound), ("update_mean", pool("rsa_pool_keys", means, Sk - 1)),
             ("update_bounds", pool("rsa_pool_key_bounds", bounds, Sk - 1)), ("select_blocks", sel_plain),
             ("prefill_mean", pool("rsa_pool_keys", means, 0)), ("prefill_bounds", pool("rsa_pool_key_bounds", bounds, 0)),
             ("prefill_mean_e4m3", pool8("rsa_pool_keys_kv8", means)), ("prefill_bounds_e4m3", pool8("rsa_pool_key_bounds_kv8", bounds))]
    return named, (bm, cols, cnt, means, bounds)


def main(other_path, out_path):
    dev = torch.device("cuda:0")
    st = _core._stream()
    libs = [("other", load(other_path)), ("tree", _lib.lib())]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for name, B, Sk in ROWS:
        g = torch.Generator(device=dev).manual_seed(B * 7 + 17)
        q = torch.randn(B, 32, 1, 128, device=dev, generator=g).to(torch.bfloat16)
        k = torch.randn(B, 8, Sk, 128, device=dev, generator=g).to(torch.bfloat16)
        k8 = torch.randint(0, 120, (B, 8, Sk, 128), device=dev, generator=g, dtype=torch.uint8)       # (positive finite codes)
        ks = torch.full((8,), 0.5, dtype=torch.float32, device=dev)
        sets = [forms(L, B, Sk, q, k, k8, ks, st) for _, L in libs]
        names = [n for n, _ in sets[0][0]]
        nf = len(names)
        per = [[f for _, f in sets[0][0]], [f for _, f in sets[1][0]]]
        for f in per[0][5:7] + per[1][5:7] + per[0] + per[1]:       # the prefills first: the caches hold values before a select reads them
            f()
        torch.cuda.synchronize()
        # the same bytes from both builds, form by form
        for i, nm in enumerate(names):
            per[0][i](); per[1][i]()
            torch.cuda.synchronize()
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sets[0][1], sets[1][1]))
            assert same, nm
        rounds = []
        for r in range(ROUNDS):                 # all forms of one build, then of the other; the first build alternates
            t = _round(torch, per[r % 2] + per[1 - r % 2], REPS)
            a, b = (t[:nf], t[nf:]) if r % 2 == 0 else (t[nf:], t[:nf])
            rounds.append([x for pair in zip(a, b) for x in pair])
        say(f"{name}: B = {B}, Sk = {Sk}; {ROUNDS} rounds x {REPS} launches per form, the two builds alternating; same bytes: yes")
        say("| form | other median (us) | other spread (us) | tree median (us) | tree - other (us) | slower beyond the spread |")
        say("|---|---|---|---|---|---|")
        for i, nm in enumerate(names):
            pa, br = [1e3 * r[2 * i] for r in rounds], [1e3 * r[2 * i + 1] for r in rounds]
            mp, mb, sp = statistics.median(pa), statistics.median(br), max(pa) - min(pa)
            say(f"| {nm} | {mp:.1f} | {sp:.1f} | {mb:.1f} | {mb - mp:+.1f} | {'yes' if mb - mp > sp else 'no'} |")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("out")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    ROUNDS, REPS = a.rounds, a.reps
    main(a.other, a.out)
