#!/usr/bin/env python3
"""Monte-Carlo of what an XCD's L2 sees under K5's sparse walks (CPU only, no GPU needed): 64 workgroups walk ascending lists of
K kept key blocks out of NB (independent random lists = regime R2), one block per time step (+- jitter), the L2 = an LRU of C
key blocks (4 MiB / 64 KiB per K + V block = 64 nominal; ~48 effective reproduces the measured hit rates).

Scheduling policies compared:
  free      the workgroups start at unrelated times (round 3)
  aligned   they start together and run freely (the product since round 4: rsa_attn.h, aligned starts)
  sorted    aligned + the 64 walks of a generation sorted by their first kept block
  window W  aligned + a walk may not begin a key block more than W block positions ahead of the slowest walk of its XCD
            (a position-synchronised sweep: what "walks that stay together" would have to mean for independent lists)

Prints hit rate, time per step relative to an unconstrained walk (1.0 = no stall) and the stall share.  The result the round-5
write-up quotes (profiles/r05_k5_walk_sim.md): every window that raises the hit rate noticeably costs more in stalls than the
aligned-start change gained per hit-rate point, because the work per key range is uneven across independent walks (a window of
w positions holds w K / NB +- sqrt(..) blocks of a walk).

`python tools/sim_walks.py product` models the PRODUCT's work mapping instead (profiles/k5_walk_order.md): the policies above put 64
walks of ONE head in every generation, the product's rsa_walk_map gave XCD x the x-th contiguous eighth of every head's units --
113 per head and XCD at the HunyuanVideo shape, cut into generations of 64, so about every second generation holds walks of two
heads, which share nothing.  Three mappings of the (XCD, generation) slots, aligned starts, LRU of C blocks, 8 heads:
  eighth    the contiguous eighth per head and XCD (the map without an order table)
  runs      runs of 64 consecutive units of one head dealt to the XCDs, units in index order
  sorted    the same runs, the head's units sorted by mean kept key block (rsa_walk_order.h + the walk_order kernels)
each on independent lists (R2) and on lists that share 60 % / 90 % of their entries with the previous query block's."""
import heapq
import sys
from collections import OrderedDict

import numpy as np

NB, K, NW = 900, 90, 64


def run(rng, C, W, jitter=0.03, gens=6, aligned=True, sort_first=False, nb=NB, k=K):
    hits = acc = 0
    cache = OrderedDict()
    tot_time, stall = 0.0, 0.0
    for _ in range(gens):
        lists = [np.sort(rng.choice(nb, k, replace=False)) for _ in range(NW)]
        if sort_first:
            lists.sort(key=lambda l: l[0])
        idx = [0] * NW
        t0 = tot_time
        ev = [((t0 if aligned else t0 + rng.uniform(0, k)), i) for i in range(NW)]
        heapq.heapify(ev)
        pos = [lists[i][0] for i in range(NW)]
        waiting = []
        tend = t0

        def release(t):
            nonlocal waiting, stall
            mn = min(pos)
            keep = []
            for tw, j in waiting:
                if lists[j][idx[j]] <= mn + W:
                    stall += t - tw
                    heapq.heappush(ev, (t, j))
                else:
                    keep.append((tw, j))
            waiting = keep

        while ev or waiting:
            t, i = heapq.heappop(ev)
            if idx[i] >= k:
                pos[i] = 10 ** 9
                tend = max(tend, t)
                if W is not None:
                    release(t)
                continue
            b = lists[i][idx[i]]
            pos[i] = b
            if W is not None and b > min(pos) + W:
                waiting.append((t, i))
                release(t)
                continue
            acc += 1
            if b in cache:
                hits += 1
                cache.move_to_end(b)
            else:
                cache[b] = 1
                if len(cache) > C:
                    cache.popitem(last=False)
            idx[i] += 1
            heapq.heappush(ev, (t + max(1.0 + rng.normal(0, jitter), 0.5), i))
            if W is not None and waiting:
                release(t)
        tot_time = tend
    return hits / acc, tot_time / (gens * k), stall / (gens * k * NW)


def make_lists(rng, n, nb, k, share):
    """n ascending lists of k of nb blocks; share > 0: list i + 1 keeps that fraction of list i's entries and redraws the rest"""
    out = [np.sort(rng.choice(nb, k, replace=False))]
    for _ in range(n - 1):
        if share <= 0:
            out.append(np.sort(rng.choice(nb, k, replace=False)))
            continue
        keep = rng.choice(out[-1], int(round(share * k)), replace=False)
        rest = np.setdiff1d(np.arange(nb), keep)
        out.append(np.sort(np.concatenate([keep, rng.choice(rest, k - len(keep), replace=False)])))
    return out


def run_product(rng, C, mapping, nb=NB, k=K, heads=8, share=0.0, gen=NW, jitter=0.03, xcd=0):
    """Hit rate of ONE XCD's L2 (LRU of C key blocks, keyed by (head, block)) over a launch of `heads` heads of nb query blocks."""
    nbp = (nb + 7) & ~7
    lists = [make_lists(rng, nb, nb, k, share) for _ in range(heads)]
    order = [sorted(range(nb), key=lambda u, h=h: (lists[h][u].mean(), u)) if mapping == "sorted" else list(range(nb)) for h in range(heads)]
    walks = []                                   # the walks this XCD receives, in the order it receives them
    if mapping == "eighth":
        for h in range(heads):
            walks += [(h, u) for u in range(xcd * (nbp >> 3), (xcd + 1) * (nbp >> 3)) if u < nb]
    else:
        n_sparse = heads * nbp
        for run0 in range(xcd * gen, n_sparse, 8 * gen):          # run r = p // gen goes to XCD r % 8
            for p in range(run0, min(run0 + gen, n_sparse)):
                h, r = divmod(p, nbp)
                if r < nb:
                    walks.append((h, order[h][r]))
    hits = acc = 0
    cache = OrderedDict()
    t0 = 0.0
    for g0 in range(0, len(walks), gen):
        grp = walks[g0:g0 + gen]
        ev = [(t0, i, 0) for i in range(len(grp))]
        heapq.heapify(ev)
        while ev:
            t, i, j = heapq.heappop(ev)
            t0 = max(t0, t)
            if j >= k:
                continue
            h, u = grp[i]
            key = (h, int(lists[h][u][j]))
            acc += 1
            if key in cache:
                hits += 1
                cache.move_to_end(key)
            else:
                cache[key] = 1
                if len(cache) > C:
                    cache.popitem(last=False)
            heapq.heappush(ev, (t + max(1.0 + rng.normal(0, jitter), 0.5), i, j + 1))
    return hits / acc


def main_product():
    print("product mapping, R2 shape (90 of 900 key blocks kept, 8 heads, generations of 64 per XCD); hit rate of one XCD's L2")
    for share, name in ((0.0, "independent lists (R2)"), (0.6, "adjacent lists share 60 %"), (0.9, "adjacent lists share 90 %")):
        print(f"== {name}")
        for mapping in ("eighth", "runs", "sorted"):
            row = []
            for C in (64, 48):
                rng = np.random.default_rng(1)
                row.append(np.mean([run_product(rng, C, mapping, share=share) for _ in range(3)]))
            print(f"  {mapping:7s}: hits C = 64 {row[0]:.3f} | C = 48 {row[1]:.3f}")
        sys.stdout.flush()


def main():
    if "product" in sys.argv[1:]:
        return main_product()
    rng = np.random.default_rng(0)
    dens = [(900, 90, "R2: 10 % of 900 key blocks"), (900, 180, "script: 20 %"), (591, 147, "Wan2.1 script: 25 % of 591")]
    for nb, k, name in dens:
        print(f"== {name}")
        for C in (48, 64):
            f = run(rng, C, None, aligned=False, nb=nb, k=k)
            a = run(rng, C, None, nb=nb, k=k)
            s = run(rng, C, None, sort_first=True, nb=nb, k=k)
            print(f"  L2 = {C} blocks: free {f[0]:.3f} | aligned {a[0]:.3f} | aligned + sorted by first block {s[0]:.3f}")
            for W in (32, 64, 96, 128, 192):
                h, tt, st = run(rng, C, W, nb=nb, k=k)
                print(f"     window {W:4d}: hits {h:.3f}  time per step {tt:.3f}  stalled {st:.3f}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
