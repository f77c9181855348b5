"""CPU: the exact references of tests/exact_ref.py are what they claim.  The float64 references equal int64 evaluations;
float32 accumulation in any order equals them whenever `bound_ok` holds, and stops doing so one term past the bound;
every entry of `perturbations` changes the reference (which is what gives tests/test_gpu_exact.py its teeth); and for the
long reductions the relative size of those changes lies under the float32 tolerances of the tolerance-based parity tests:
a checked record that those tests could not see a single element counted wrongly."""
import numpy as np
import pytest

import exact_ref as X

F32 = np.float32


def _chain_goa(N, n_groups, size):
    """Column of each atom: `n_groups` groups of `size` consecutive atoms at the front, then single atoms."""
    goa = np.empty(N, dtype=np.int64)
    for a in range(N):
        goa[a] = a // size if a < n_groups * size else n_groups + a - n_groups * size
    return goa, N - n_groups * (size - 1)


def test_bound_and_ranges():
    assert X.bound_ok(4096, 64, 64, 24) and not X.bound_ok(4097, 64, 64, 24)
    assert X.mantissa("float64", np.float64) == 53 and X.mantissa(np.float64, "float32") == 24
    assert X.int_range(3 * 20003, ["float32"]) == 16                 # 60009 * 16 * 16 <= 2**24 < 60009 * 17 * 17
    assert X.int_range(3 * 20003, ["float64"]) == 100                # capped
    assert X.int_range(3 * 20011, ["float32"], 3, 3) == 5
    with pytest.raises(AssertionError):
        X.int_range(3 * 20011, ["float32"], 16, 16)                  # only 0 / +-1 data would fit: refused
    v = X.integers(np.random.default_rng(0), (1000,), 7)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).min() == 1 and np.abs(v).max() == 7 and set(np.sign(v)) == {-1.0, 1.0}
    d = X.powers_of_two(np.random.default_rng(0), (1000,), zeros=0.2)
    assert (d == 0).any() and set(np.unique(d[d > 0])) <= {1.0, 2.0, 4.0, 8.0}


def test_float64_references_equal_int64_evaluations():
    rng = np.random.default_rng(1)
    f = X.gram_frames(37, 11, ["float64"], group=3, seed=2)
    goa, n_red = _chain_goa(11, 2, 3)
    fi = f.astype(np.int64)
    Ci = np.zeros((11, n_red), dtype=np.int64)
    Ci[np.arange(11), goa] = 1
    Ri = np.einsum("tad,ar->tdr", fi, Ci).reshape(-1, n_red)
    assert np.array_equal(X.gram_ref(f, goa, n_red), (Ri.T @ Ri).astype(np.float64))
    assert np.array_equal(X.gram_ref(f), np.einsum("tid,tjd->ij", fi, fi).astype(np.float64))
    pts, mat = X.operand_pair(13, (9, 13, 3), (5, 13), ["float64"], seed=3)
    assert np.array_equal(X.apply_ref(pts, mat), np.einsum("cn,tnd->tcd", mat.astype(np.int64), pts.astype(np.int64)))
    a, b = X.operand_pair(3 * 9, (9, 4, 3), (9, 6, 3), ["float64"], seed=4)
    assert np.array_equal(X.cross_ref(a, b), np.einsum("tid,tjd->ij", a.astype(np.int64), b.astype(np.int64)))
    fac = X.integers(rng, (9, 5, 13), 50)
    assert np.array_equal(X.frames_ref(pts, fac), np.einsum("tcf,tfd->tcd", fac.astype(np.int64), pts.astype(np.int64)))
    g = X.integers(rng, (9, 5, 3), 50)
    assert np.array_equal(X.frames_t_ref(g, fac), np.einsum("tca,tcd->tad", fac.astype(np.int64), g.astype(np.int64)))
    assert np.array_equal(X.frames_outer_ref(g, pts), np.einsum("tcd,tad->tca", g.astype(np.int64), pts.astype(np.int64)))
    w = X.integers(rng, (9, 4, 13), 50)
    u = X.pair_disp(pts, X.integers(rng, (9, 4, 3), 50))
    A, B = X.pair_pull_ref(w, u)
    ui, wi = u.astype(np.int64), w.astype(np.int64)
    assert np.array_equal(A, np.einsum("tij,tijd->tjd", wi, ui)) and np.array_equal(B, -np.einsum("tij,tijd->tid", wi, ui))
    pairs = np.stack(np.nonzero(np.ones((4, 13))), axis=1)
    A2, B2 = X.list_pull_ref(w.reshape(9, -1), u.reshape(9, -1, 3), pairs, 4, 13)
    assert np.array_equal(A2, A) and np.array_equal(B2, B)
    ptr, atoms = np.array([0, 3, 4, 13]), np.arange(13)[::-1].copy()
    assert np.array_equal(X.group_sum_ref(pts, ptr, atoms)[:, 0], pts[:, [12, 11, 10]].sum(1))


def _float32_orders(R):
    """Gram of the rows of R accumulated in float32: forward, reversed, and pairwise over blocks of 8 rows."""
    R32 = R.astype(F32)
    n = R.shape[1]

    def run(order):
        acc = np.zeros((n, n), dtype=F32)
        for k in order:
            acc += np.outer(R32[k], R32[k])  # (float32 products of integers below 2**12: exact)
        return acc

    L = R.shape[0]
    blocks = [run(range(s, min(s + 8, L))) for s in range(0, L, 8)]
    while len(blocks) > 1:
        blocks = [blocks[i] + blocks[i + 1] if i + 1 < len(blocks) else blocks[i] for i in range(0, len(blocks), 2)]
    return run(range(L)), run(range(L - 1, -1, -1)), blocks[0]


@pytest.mark.parametrize("T,N,n_groups,size", [(333, 12, 0, 1), (1001, 9, 2, 3), (2731, 5, 1, 2)])
def test_float32_accumulation_in_any_order_is_exact_under_the_bound(T, N, n_groups, size):
    f = X.gram_frames(T, N, ["float32"], group=size, seed=T)
    goa, n_red = _chain_goa(N, n_groups, size)
    ref = X.gram_ref(f, goa, n_red)
    assert np.abs(ref).max() <= 2 ** 24
    assert np.abs(ref).max() > 2 ** 20  # the range the generator chose is not a timid one
    for got in _float32_orders(X.reduce_columns(f, goa, n_red)):
        assert got.dtype == F32 and np.array_equal(got.astype(np.float64), ref)


def test_one_term_past_the_bound_is_not_exact():
    """4096 terms of 64 * 64 sum to 2**24 exactly (the bound holds with equality); one more term of 1 * 1 leaves the
    bound, and 2**24 + 1 is no float32: the bound is the edge."""
    x = np.full((4096, 1), 64.0)
    assert X.bound_ok(len(x), 64, 64, 24)
    for got in _float32_orders(x):
        assert float(got[0, 0]) == 2.0 ** 24 == float((x.T @ x)[0, 0])
    y = np.concatenate([x, [[1.0]]])
    assert not X.bound_ok(len(y), 64, 64, 24)
    exact = float((y.T @ y)[0, 0])
    assert exact == 2.0 ** 24 + 1
    for got in _float32_orders(y):
        assert float(got[0, 0]) != exact
    assert X.bound_ok(len(y), 64, 64, 53)  # (float64 holds it)


def _gram_case(T, N, n_groups=0, size=1, seed=5):
    f = X.gram_frames(T, N, ["float32"], group=size, seed=seed)
    goa, n_red = _chain_goa(N, n_groups, size)
    return f, (lambda g: X.gram_ref(g, goa, n_red)), (1 if n_groups else None)


def _families(T):
    """(name, the perturbed operand, reference as a function of it, a constraint-group member or None)"""
    rng = np.random.default_rng(T)
    out = [("gram",) + _gram_case(T, 24), ("gram with groups",) + _gram_case(T, 25, 3, 4)]
    pts, mat = X.operand_pair(20, (T, 20, 3), (4, 20), ["float32"], seed=6)
    out.append(("apply", pts, lambda p: X.apply_ref(p, mat), None))
    a, b = X.operand_pair(3 * T, (T, 7, 3), (T, 11, 3), ["float32"], seed=7)
    out.append(("cross", a, lambda q: X.cross_ref(q, b), None))
    x, c = X.integers(rng, (T, 9, 3), 20), X.integers(rng, (T, 5, 3), 20)
    w = X.integers(rng, (T, 5, 9), 20)
    out.append(("pull weights", w, lambda v: np.concatenate(X.pair_pull_ref(v, X.pair_disp(x, c)), axis=1), None))
    out.append(("pull sites", x, lambda v: np.concatenate(X.pair_pull_ref(w, X.pair_disp(v, c)), axis=1), None))
    return out


@pytest.mark.parametrize("T", [1, 2, 333])
def test_every_perturbation_changes_the_reference(T):
    for name, arr, ref_of, member in _families(T):
        ref = ref_of(arr)
        perts = X.perturbations(arr.shape, member)
        assert len(perts) >= (3 if T > 2 else 1)
        for what, idx in perts:
            changed = X.perturb(arr, idx)
            assert np.abs(changed - arr).sum() == 1 and np.abs(changed[idx]) == np.abs(arr[idx]) - 1
            assert not np.array_equal(ref_of(changed), ref), (name, what, idx)


OLD_TOLERANCES = (2e-5, 3e-5, 5e-5)  # test_gpu_parity / _autograd / _distances; _dispatch_classes; _layouts


def test_the_old_tolerances_cannot_see_one_element_of_a_long_reduction():
    """T = 20003 (test_gram_edge_form_many_splits, the long K8a case): a single element changed by 1 moves the result
    by less than each float32 tolerance -- of the largest entry for the Gram matrix, of each entry's sum of |a||b| for
    K8a (the measure of tests/test_gpu_autograd.py) -- for EVERY place `perturbations` lists, as it happens."""
    T = 20003
    a, b = X.operand_pair(3 * T, (T, 7, 3), (T, 11, 3), ["float32"], seed=7)
    cases = [("gram",) + _gram_case(T, 200) + (None,), ("gram with groups",) + _gram_case(T, 130, 10, 3) + (None,),
             ("cross", a, lambda q: X.cross_ref(q, b), None, lambda q: X.cross_ref(np.abs(q), np.abs(b)))]
    for name, arr, ref_of, member, bound_of in cases:
        ref = ref_of(arr)
        scale = np.abs(ref).max() if bound_of is None else bound_of(arr)
        sizes = {}
        for what, idx in X.perturbations(arr.shape, member):
            diff = np.abs(ref_of(X.perturb(arr, idx)) - ref)
            assert diff.max() >= 1
            sizes[what] = (float(np.max(diff / scale)), int((diff > 0).sum()))
        print(name, {k: f"{v[0]:.2e} of the scale in {v[1]} entries" for k, v in sizes.items()})
        for tol in OLD_TOLERANCES:
            assert min(v[0] for v in sizes.values()) < tol, (name, tol, sizes)
        assert max(v[0] for v in sizes.values()) < min(OLD_TOLERANCES), (name, sizes)
