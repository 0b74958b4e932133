"""tests/comp_ref.py on the CPU, so that nothing in tests/test_gpu_comp.py rests on the construction: the budget and the lo share of
every exact case, the numpy models of both K4 forms against the exact classes (equal) and the bound class (inside the derived
bounds) under three accumulation orders each, and the mutant table per shape with its exemptions."""
import numpy as np
import pytest

import comp_ref as cr

SHAPES = {sh.name: sh for sh in cr.SHAPES}
CASES = [(n, D) for n in SHAPES for D in cr.DS]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _heads(sh):
    return 2 if sh.dense else 1


def _tiles(sh):
    """The float32 orders walk every tile of a dense shape, and the first and last tile of a long one (the fp64 evaluator, which an
    exact class makes the only answer, always walks all)."""
    return None if sh.dense else sorted({0, (sh.NBv - 1) // 32})


def _same(got, ref, kinds):
    """Equal by bit pattern; the all-zero rows by value (+0 or -0)."""
    zero = np.array([[k == "zero" for k in kh] for kh in kinds[:got.shape[0]]])
    eq = _bits(got) == _bits(ref)
    eq[zero] = (got[zero] == 0)
    return eq


@pytest.mark.parametrize("cls", ["X1", "X2"])
@pytest.mark.parametrize("name,D", CASES)
def test_exact_case_budget_lo_share_and_kinds(name, D, cls):
    sh = SHAPES[name]
    c = cr.exact_case(sh, D, cls)                     # (the builder asserts the budget per element, hi + lo = x, lo . lo = 0)
    print(f"{name} D={D} {cls}: bits {c.info['bits']}, largest sum {c.info['budget']:.3f} of 2^24 quanta, "
          f"lo != 0 on {c.info['lo_share']:.1%} of {c.info['nonzero']} non-zero operands of the split side")
    assert c.info["budget"] < 1.0 and c.info["lo_share"] >= 0.25
    want = {cr.kind_of(sh, i) for i in range(min(32, sh.NBv))} if sh.NBv < 32 else \
        {k for k in cr.KINDS if not (k == "text" and not sh.n_txt) and not (k.startswith("hot:") and not 0 <= cr._col(sh, k) < sh.L)}
    for h in range(cr.HEADS):
        assert sorted(cr.head_perm(sh, h).tolist()) == list(range(sh.NBv))
        for t0 in range(0, sh.NBv - 31 if sh.NBv >= 32 else 1, 32):
            miss = want - set(c.kinds[h][t0:t0 + 32])       # (a tile whose rotation starts on pair_b has no pair_a in front of it)
            assert not miss - ({"pair_b"} if 7 * (t0 // 32) % 32 == 4 else set()), (h, t0, miss)
        for i, k in enumerate(c.kinds[h]):
            nz = np.nonzero(c.w[h, i])[0]
            if k == "zero":
                assert nz.size == 0 and not c.ref[h, i].any()
            elif k.startswith("hot:"):              # comp[i] = vbar[j] 2^-e, to the bit
                j = cr._col(sh, k)
                assert nz.tolist() == [j] and np.array_equal(c.ref[h, i], c.vbar[h, j] * c.w[h, i, j])
                assert np.log2(c.w[h, i, j]) % 1 == 0
            elif k == "text":
                assert nz.tolist() == [sh.NBv]
            elif k == "pair_b":
                if h == 0:
                    assert c.kinds[0][i - 1] == "pair_a" and np.nonzero(c.w[0, i] != c.w[0, i - 1])[0].tolist() == [sh.L - 1]
            else:
                assert nz.size == sh.nnz
    if sh.NB_total > sh.L:
        assert (np.abs(c.vbar[:, sh.L:]) >= 2.0 ** 16 * np.abs(c.vbar[:, :sh.L]).max(1, keepdims=True)).all() and np.isfinite(c.vbar).all()
    assert sh.NBv <= 2 or len({c.w[h].tobytes() for h in range(cr.HEADS)}) == cr.HEADS


@pytest.mark.parametrize("cls", ["X1", "X2"])
@pytest.mark.parametrize("name,D", CASES)
def test_models_reproduce_the_exact_classes(name, D, cls):
    sh = SHAPES[name]
    c = cr.exact_case(sh, D, cls)
    H = _heads(sh)
    for form in ("chain", "split"):
        got = cr.model(c, H, form, "exact")
        assert _same(got, c.ref[:H], c.kinds).all(), (name, D, cls, form, "fp64")
        for order in cr.ORDERS[form]:
            got = cr.model(c, H, form, order, tiles=_tiles(sh))
            done = ~np.isnan(got)
            assert done.any() and (_same(got, c.ref[:H], c.kinds) | ~done).all(), (name, D, cls, form, order)


@pytest.mark.parametrize("name,D", CASES)
def test_models_stay_inside_the_bounds(name, D):
    sh = SHAPES[name]
    c = cr.bound_case(sh, D)
    H = _heads(sh)
    b = cr.bounds(c.w[:H], c.vbar[:H], sh.L)
    assert np.array_equal(b["ref"], c.ref[:H]) and (b["S"] > 0).any()
    for form in ("chain", "split"):
        for order in cr.ORDERS[form]:
            got = cr.model(c, H, form, order, tiles=_tiles(sh)).astype(np.float64)
            done = ~np.isnan(got)
            err = np.where(done, np.abs(np.where(done, got, 0) - b["ref"]), 0)
            ratio = np.where(b[form] > 0, err / np.where(b[form] > 0, b[form], 1), np.where(err > 0, np.inf, 0))
            print(f"{name} D={D} {form:5s} {order:11s}: largest |model - ref| / bound {ratio.max():.3f}")
            assert (err <= b[form]).all(), (name, D, form, order, float(ratio.max()))


@pytest.mark.parametrize("name,D", CASES)
def test_mutant_table(name, D):
    """Every mutant changes the exact-class output of the model (X1 or X2; any difference counts, equality is what the device test
    asserts) on every shape that can hold it, and the split form's arithmetic mutants leave the bound class by 8 bounds and more.
    hi_trunc cannot: with hi truncated |x - hi| < 2^-7 |x| and |rest| <= 2^-16 |x|, so what is dropped is at most
    (2^-14 + 2^-15 + ...) < 3.1 * 2^-15 per product -- under 3.1 bounds by derivation, asserted as such and printed -- and the exact
    classes cannot see it at all (hi + lo = x under either rounding).  The split is pinned on the device by the exact classes
    (hi + lo = x with lo != 0) and by the bound itself, not by this mutant."""
    sh = SHAPES[name]
    H = 2
    exact = {cls: cr.exact_case(sh, D, cls) for cls in ("X1", "X2")}
    bc = cr.bound_case(sh, D)
    b = cr.bounds(bc.w[:H], bc.vbar[:H], sh.L)
    for form in ("chain", "split"):
        for mut in cr.MUTANTS:
            seen = []
            for cls, c in exact.items():
                got = cr.model(c, H, form, "exact", mut)
                if not _same(got, c.ref[:H], c.kinds).all():
                    seen.append(cls)
            rule = cr.exemption(sh, D, form, mut)
            line = f"{name} D={D} {form:5s} {mut:11s}: " + ("differs on " + " ".join(seen) if seen else f"EXEMPT ({rule})")
            if mut in cr.SPLIT_MUTANTS and form == "split":
                got = cr.model(bc, H, form, "exact", mut).astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = float(np.nanmax(np.where(b["split"] > 0, np.abs(got - b["ref"]) / b["split"], 0)))
                line += f"; bound class: {ratio:.1f} bounds"
                print(line)
                if mut == "hi_trunc":
                    assert 1.0 < ratio < 3.1, (name, D, mut, ratio)      # (it does leave the bound, on every shape)
                else:
                    assert ratio >= 8.0, (name, D, mut, ratio)
            else:
                print(line)
            assert seen or rule is not None, (name, D, form, mut, "no element differs and no rule exempts the shape")
