"""The designed rows of tests/select_rows.py without a GPU: the independent model equals the oracle on every row, the builder's
claims hold on the oracle's output, and every model mutant changes some row of every shape that holds a class aimed at it."""
import numpy as np
import pytest

import select_rows as sr

SHAPES = {sh.name: sh for sh in sr.SHAPES}
F32 = np.float32


def _sorted(pr):
    return np.lexsort((np.arange(len(pr)), -pr))


def _crossing(pr, p):
    """(np.cumsum in float32 is the sequential sum: test_cumsum_in_float32_is_the_sequential_sum)"""
    return int((np.cumsum(pr[_sorted(pr)], dtype=np.float32) <= F32(p)).sum())


@pytest.mark.parametrize("name,pname", [(n, k) for n, sh in SHAPES.items() for k in sr.param_sets(sh)])
def test_model_equals_oracle(name, pname):
    """kept, n_needed, probs, R and w of model_row == oracle.select_rows_from_scores: every row of head 0 under every parameter
    set, every row of the permuted head under the designed one."""
    sh = SHAPES[name]
    for bh in range(2 if pname == "designed" else 1):
        ref = sr.reference(sh, pname, bh)
        for r in range(sh.NBv):
            kept, n_needed, R, w, _ = sr.model_case_row(sh, bh, r, pname)
            src = r if bh == 0 else int(sr.case(sh).perm[r])
            assert np.array_equal(sr.probs_of(sh, src), ref["probs"][r]), (name, pname, bh, r)
            assert np.array_equal(kept, ref["kept"][r]), (name, pname, bh, r)
            assert n_needed == ref["n_needed"][r] and R == ref["R"][r], (name, pname, bh, r)
            assert np.array_equal(w, ref["w"][r]), (name, pname, bh, r)


def test_cumsum_in_float32_is_the_sequential_sum():
    """model_row sums with np.cumsum(dtype=float32); the contract's sum is a loop."""
    for sh in (SHAPES["63+3txt"], SHAPES["520"]):
        for r in range(0, sh.NBv, 7):
            pr = sr.probs_of(sh, r)
            sp = pr[_sorted(pr)]
            assert np.array_equal(np.cumsum(sp, dtype=np.float32), sr.seq_sum_loop(sp))


@pytest.mark.parametrize("pname,shift", [("designed", 2), ("exact half", 1)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_class_A_analytic(name, pname, shift):
    """Exact cuts, at p_remain = 0.25 (shift 2) and 0.5 (shift 1).  A1, the whole row equal, where the row length is a power of two and
    there is no text: p = 1 / L, count = L >> shift, n = count + 1 -- n = 17 at L = 64 and p_remain 0.25, n = 65 at L = 128 and 0.5.
    A2, a plateau of 2^k at p = 2^-k in a longer row: count = 2^k >> shift, n = count + 1 (17 for the 64-plateau at 0.25, 65 for 128 at
    0.5); the kept ones are the plateau's lowest columns."""
    sh = SHAPES[name]
    ref = sr.reference(sh, pname)
    seen = set()
    for r, row in enumerate(sr.case(sh).rows):
        if row.cls != "A":
            continue
        if row.info["whole"]:
            if sh.n_txt == 0 and sh.L & (sh.L - 1) == 0:
                assert np.all(ref["probs"][r] == F32(1.0 / sh.L)) and ref["n_needed"][r] == max((sh.L >> shift) + 1, sr.TOP_K)
                seen.add("whole")
            continue
        k, cols = row.info["k"], row.info["plateau"]
        assert np.all(ref["probs"][r][cols] == F32(2.0 ** -k)) and ref["probs"][r].sum() == 1.0
        n = ((1 << k) >> shift) + 1
        assert ref["n_needed"][r] == max(n, sr.TOP_K), (name, r, k)
        sel = ref["kept"][r].astype(bool).copy()
        nbr = sh.neighbor()
        union = np.zeros(sh.NB_total, bool)
        union[:sh.NBv] |= nbr[r] != 0
        if sh.ffb and r < sh.ffb:
            union[:sh.ffb] = True
        if sh.n_txt:
            union[sh.NBv] = True
        want = np.zeros(sh.NB_total, bool)
        want[cols[:max(n, sr.TOP_K)]] = True
        assert np.array_equal(sel | union, want | union) and sel[cols[:n]].all(), (name, r)
        seen.add(k)
    assert seen - {"whole"}, name
    if name in ("64", "128", "256"):
        assert "whole" in seen
        whole = [r for r, row in enumerate(sr.case(sh).rows) if row.cls == "A" and row.info["whole"]][0]
        if (name, pname) == ("64", "designed"):
            assert ref["n_needed"][whole] == 17
        if (name, pname) == ("128", "exact half"):
            assert ref["n_needed"][whole] == 65
    if sh.NBv >= 64:
        assert 6 in seen          # the 64-plateau: n = 17 at 0.25, 33 at 0.5


@pytest.mark.parametrize("name", list(SHAPES))
def test_bookkeeping(name):
    """What the builder recorded is true of the oracle's output, and every class that applies to the shape is there in every form."""
    sh = SHAPES[name]
    ref = sr.reference(sh, "designed")
    c = sr.case(sh)
    got = {}
    for r, row in enumerate(c.rows):
        pr, n = ref["probs"][r], int(ref["n_needed"][r])
        order = _sorted(pr)
        info = row.info
        if row.cls == "B":
            cols = info["plateau"]
            pos = np.nonzero(np.isin(order, cols))[0]
            assert len(set(pr[cols].tolist())) == 1 and np.array_equal(pos, np.arange(pos[0], pos[0] + len(cols)))
            assert n == sr.TOP_K and pos[0] < n < pos[-1] + 1, (name, r, "the top_k cut is not strictly inside the plateau")
            assert _crossing(pr, sr.P_REMAIN) + 1 <= sr.TOP_K
            assert {0, sh.NBv - 1} <= set(cols.tolist())
            got["B"] = got.get("B", 0) + 1
        elif row.cls == "C":
            cols = info["plateau"]
            pos = np.nonzero(np.isin(order, cols))[0]
            assert len(set(pr[cols].tolist())) == 1 and np.array_equal(pos, np.arange(pos[0], pos[0] + len(cols)))
            x = _crossing(pr, sr.P_REMAIN)
            assert x == info["crossing"] and n == x + 1 > sr.TOP_K
            assert pos[0] < x < pos[-1], (name, r, "the crossing element is not inside the plateau")
            K = info["lane_keys"]
            assert x % K == (K - 1 if info["lane_last"] else 0)
            got[("C", K, info["lane_last"])] = 1
        elif row.cls == "D":
            cols = info["plateau"]
            assert len(set(pr[cols].tolist())) == 1
            if info["count"] is not None:
                t = pr[info["second"]].max() if len(info["second"]) else -1.0
                assert int((pr > t).sum()) == info["count"] and int((pr >= pr[cols[0]]).sum()) == info["count"]
                if len(info["second"]):
                    assert int((pr >= t).sum()) > 256 or info["count"] >= 256
                got[("D", info["count"])] = 1
            else:
                lo, hi = info["jump"]
                assert int((pr > pr[cols[0]]).sum()) == lo < 128 and int((pr >= pr[cols[0]]).sum()) == hi > 256
                got[("D", "jump")] = 1
        elif row.cls == "E":
            a, b = info["hi"], info["lo"]
            assert (a > b) == info["hi_higher"] and pr[b] == np.nextafter(pr[a], F32(0)), (name, r, "not adjacent floats")
            cut = n if n <= sh.L else sh.L
            assert order[cut - 1] == a and order[cut] == b, (name, r, "the pair does not straddle the cut")
            assert (n == sr.TOP_K) == (info["cut"] == "top_k")
            got[("E", info["cut"], info["hi_higher"])] = 1
        elif row.cls == "F":
            sub = (pr > 0) & (pr < sr.TINY)
            assert sub.sum() >= 1 and (pr == 0).sum() >= 2, (name, r)
            assert n == sr.TOP_K
            last = pr[order[n - 1]]
            kind = "zero" if last == 0 else "subnormal" if last < sr.TINY else "normal"
            assert kind == info["cut"], (name, r, kind)
            if kind == "zero":
                z = np.nonzero(pr == 0)[0]
                nz = n - int((pr > 0).sum())
                assert np.array_equal(np.sort(order[n - nz:n]), z[:nz])
            got[("F", kind)] = 1
        elif row.cls == "A":
            got["A"] = 1
    want = ["A", "B"] + [("F", k) for k in ("normal", "subnormal", "zero")]
    want += [("C", sh.KPL, False), ("C", sh.KPL, True)]
    if sh.long:
        want += [("C", 4, False), ("C", 4, True)] + [("D", t) for t in sr.D_COUNTS + ("jump",)] + [("E", c_, hh) for c_ in ("top_k", "p_remain") for hh in (True, False)]
    assert not [w for w in want if w not in got], (name, [w for w in want if w not in got])
    # G: the extremes do what they are there for
    g = {k: sr.reference(sh, k) for k in sr.param_sets(sh)}
    assert (g["p below the first probability, top_k 0"]["n_needed"] == 1).all()
    assert (g["p 0, top_k 1"]["n_needed"] == 1).all()
    assert (g["p 1, top_k L"]["n_needed"] >= sh.L).all() and (g["p 1, top_k L"]["kept"][:, :sh.L] == 1).all()
    # ... and with a small top_k n = L + 1 comes from the COUNT of a sum that never passes: on every row above 1.0, and at 1.0 on the
    # rows whose probabilities sum to exactly 1 (A2: 1.0 <= 1.0) or below it; the clamp is what keeps n at L
    for k_ in ("p above 1, top_k 8", "p above 1, top_k 0"):
        assert (g[k_]["n_needed"] == sh.L + 1).all() and (g[k_]["kept"][:, :sh.L] == 1).all()
    one = g["p 1, top_k 8"]
    cnt = np.array([_crossing(one["probs"][r], 1.0) for r in range(sh.NBv)])
    assert np.array_equal(one["n_needed"], np.maximum(cnt + 1, sr.TOP_K))
    a2 = [r for r, row in enumerate(c.rows) if row.cls == "A" and not row.info["whole"]]
    assert a2 and (cnt[a2] == sh.L).all() and (one["n_needed"][a2] == sh.L + 1).all() and (one["kept"][a2][:, :sh.L] == 1).all()
    assert (cnt < sh.L).any(), "no row whose sum passes 1.0 before the end"
    assert (g["p above 1, top_k L + 5"]["n_needed"] == sh.L + 5).all()
    if sh.long:
        assert any(int(g["top_k 256"]["n_needed"][r]) == 256 and row.cls == "D" and row.info.get("count") == 256
                   for r, row in enumerate(c.rows)), "no row whose decided n equals the 256 candidates of the sorted head"
    # H: some plateau of a B or C row has members outside M both kept and dropped, so w depends on which ones were kept
    h = 0
    for r, row in enumerate(c.rows):
        if row.cls in "BC":
            cols = row.info["plateau"]
            free = c.unrel[0, r][cols] == 0
            k = ref["kept"][r][cols] != 0
            h += bool((free & k).any() and (free & ~k).any())
    assert h >= 2, name


def _changed(a, b):
    return (not np.array_equal(a[0], b[0])) or a[2] != b[2] or (not np.array_equal(a[3], b[3])) or a[4] != b[4]


def _exempt(sh, mut):
    """The rule by which a shape cannot show a mutant at all (None: it can)."""
    aimed = sr.MUTANTS[mut]
    if not sh.long and (set(aimed) <= set("DE") or mut.startswith("sum restarted")):
        return "classes D and E, and a sum that runs past position 256, need L > 256"
    if mut.startswith("ties broken by the load order") and sh.NBv <= 64:
        return "the load order of the visual columns is their column order up to 64 columns"
    if mut.startswith("first-frame") and not sh.ffb:
        return "the layout has no first-frame square (HunyuanVideo-style text layouts)"
    if mut == "subnormals flushed in the sums of R":
        return "equivalent: R >= the row's largest probability >= 1 / L, and L subnormals are far below half an ulp of that"
    return None


@pytest.mark.parametrize("name", list(SHAPES))
def test_mutants(name, capsys):
    """Each model mutant changes kept (hence counts), R or w on some row (looked for among the first 240 of each head) of every shape that holds a class
    aimed at it; the table is printed.  G aims at every row under the extreme parameter sets, H at the rows of classes B and C."""
    table, missed = [], []
    for sh in (SHAPES[name],):
        c = sr.case(sh)
        base = {}
        for mut, aimed in sr.MUTANTS.items():
            rule = _exempt(sh, mut)
            psets = [k for k in sr.param_sets(sh) if k != "designed"] if aimed == "G" else \
                [k for k in ("designed", "deep cut") if k in sr.param_sets(sh)] if mut.startswith("sum restarted") else ["designed"]
            rows_cls = "BC" if aimed == "H" else sr.classes(sh) if aimed == "G" else aimed
            hit = 0
            for pname in psets:
                for bh in (0, 1):
                    for r in range(min(sh.NBv, 240)):        # (every variant of every class recurs within 48 rows)
                        if c.row_of(bh, r).cls not in rows_cls:
                            continue
                        key = (pname, bh, r)
                        if key not in base:
                            base[key] = sr.model_case_row(sh, bh, r, pname)
                        hit += _changed(base[key], sr.model_case_row(sh, bh, r, pname, mut))
                    if hit:
                        break
                if hit:
                    break
            table.append((sh.name, mut, aimed, hit, rule))
            if rule is None and not hit:
                missed.append((sh.name, mut))
            if rule is not None and mut == "subnormals flushed in the sums of R":
                assert not hit
    # the clamp is reached through count + 1 = L + 1, not through top_k: the unclamped n shows under each small-top_k set
    sh = SHAPES[name]
    for pname in ("p 1, top_k 8", "p above 1, top_k 8", "p above 1, top_k 0"):
        assert any(sr.model_case_row(sh, 0, r, pname, "n not clamped to L")[4] for r in range(sh.NBv)), (name, pname)
    with capsys.disabled():
        print(f"\nshape {name}: mutant -> classes aimed at: rows changed (exempt by rule where 0)")
        for mut, aimed in sr.MUTANTS.items():
            cells = [f"{n}: {h if h else ('exempt' if rule else 'MISSED')}" for n, m, _, h, rule in table if m == mut]
            print(f"  {mut} -> {aimed}: " + ", ".join(cells))
        for rule in sorted({t[4] for t in table if t[4] and not t[3]}):
            print(f"  exempt: {rule}")
    assert not missed, missed
