"""Whole molecules, host side (no GPU): ``MoleculeTree`` / ``from_bonds`` against brute force, the two forms of the
NumPy reference (tests/whole_ref.py) against each other, ``make_whole`` on CPU tensors and NumPy arrays against the
reference (image counts exact, coordinates within 1 ulp at max(|x|, |u|), and within 2 ulp of the independent
two-rounding form: ``whole_ref.assert_coords``), the keyword
``bonds=`` of project_forces refused without a box before any device work, and the C ABI's new entries."""
import inspect

import numpy as np
import pytest
import torch

import whole_ref as R
from aggforce_amd import MoleculeTree, _lib, make_whole, project_forces
from aggforce_amd.agg import project_forces_grid_cv
from aggforce_amd.jaxutil import PairList
from aggforce_amd.pbc import as_tree


def random_bonds(n, rng):
    """A random graph over n sites: a few molecules (random trees), ring-closing and repeated bonds, in random row and
    column order; and the component label of every site (its lowest index)."""
    par = R.random_tree(n, int(rng.integers(1 << 30)), n_roots=int(rng.integers(1, max(2, n // 4 + 1))))
    par[rng.random(n) < 0.15] = -1  # more singletons and fragments
    child = np.flatnonzero(par >= 0)
    bonds = np.stack([child, par[child]], axis=1)
    comp = np.arange(n)
    for i in R.topological(par):
        if par[i] >= 0:
            comp[i] = comp[par[i]]
    for c in np.unique(comp):  # (label = lowest index of the component)
        comp[comp == c] = np.flatnonzero(comp == c).min()
    extra = []
    for _ in range(int(rng.integers(0, n // 3 + 1))):  # ring closures inside a component, repeats of a bond
        i = int(rng.integers(n))
        same = np.flatnonzero(comp == comp[i])
        j = int(rng.choice(same))
        if i != j:
            extra.append((i, j))
    if len(bonds) and len(extra) % 2:
        extra.append(tuple(bonds[0][::-1]))
    bonds = np.concatenate([bonds, np.array(extra, dtype=np.int64).reshape(-1, 2)])
    flip = rng.random(len(bonds)) < 0.5
    bonds[flip] = bonds[flip][:, ::-1]
    return bonds[rng.permutation(len(bonds))], comp


def test_from_bonds_builds_a_spanning_forest_with_brute_force_jump_tables():
    rng = np.random.default_rng(20261018)
    for trial in range(60):
        n = int(rng.integers(1, 201))
        bonds, comp = random_bonds(n, rng)
        tree = MoleculeTree.from_bonds(n, bonds if trial % 2 else PairList(bonds, n))
        par = tree.parent
        assert par.shape == (n,) and tree.n_sites == n
        # a forest: every site reaches a root, the root is the lowest index of its component, every edge is a bond
        bonded = {frozenset(map(int, b)) for b in bonds}
        for i in range(n):
            a, steps = i, 0
            while par[a] >= 0:
                assert frozenset((int(a), int(par[a]))) in bonded
                a, steps = par[a], steps + 1
                assert steps <= n
            assert a == comp[i]
        assert (par >= 0).sum() == n - len(np.unique(comp))  # spanning: one edge less than sites per component
        # breadth first: no bond skips a level
        level = np.array([sum(1 for _ in iter_up(par, i)) for i in range(n)])
        assert all(abs(level[i] - level[j]) <= 1 for i, j in bonds)
        assert tree.depth == R.depth_of(par) == level.max()
        want = R.jump_tables(par)
        assert tree.n_rounds == want.shape[0] and tree.jumps.dtype == np.int32 and tree.jumps.shape == want.shape
        assert np.array_equal(tree.jumps, want)
        pairs = tree.pairs
        assert isinstance(pairs, PairList) and pairs.n_sites == n
        assert {(int(c), int(p)) for c, p in pairs.pairs} == {(i, int(par[i])) for i in range(n) if par[i] >= 0}


def iter_up(par, i):
    while par[i] >= 0:
        i = par[i]
        yield i


@pytest.mark.parametrize("depth,rounds", [(0, 0), (1, 0), (2, 1), (3, 2), (4, 2), (5, 3), (16, 4), (17, 5)])
def test_depth_and_rounds(depth, rounds):
    down = np.arange(-1, depth)                                            # atom i hangs on i - 1
    up = np.where(np.arange(depth + 1) < depth, np.arange(1, depth + 2), -1)  # on i + 1: parents after their children
    for par in (down, up):
        tree = MoleculeTree(par)
        assert (tree.depth, tree.n_rounds) == (depth, rounds)
        assert tree.jumps.shape == (rounds, depth + 1) and np.array_equal(tree.jumps, R.jump_tables(par))
    star = MoleculeTree(R.star(9))
    assert (star.depth, star.n_rounds) == (1, 0)


def test_rings_and_repeats_are_tolerated_bad_rows_are_named():
    ring = MoleculeTree.from_bonds(6, [[0, 1], [1, 2], [2, 0], [2, 1], [1, 0], [4, 5], [5, 4]])
    assert ring.parent.tolist() == [-1, 0, 0, -1, -1, 4]
    assert MoleculeTree.from_bonds(3, []).parent.tolist() == [-1, -1, -1]
    assert MoleculeTree.from_bonds(0, np.zeros((0, 2), dtype=np.int64)).n_sites == 0
    with pytest.raises(ValueError, match="row 2"):
        MoleculeTree.from_bonds(4, [[0, 1], [1, 2], [3, 3]])
    with pytest.raises(ValueError, match="row 1"):
        MoleculeTree.from_bonds(4, [[0, 1], [1, 4]])
    with pytest.raises(ValueError, match="row 0"):
        MoleculeTree.from_bonds(4, [[-1, 1], [1, 2]])
    with pytest.raises(ValueError, match="integers"):
        MoleculeTree.from_bonds(4, [[0.5, 1.0]])
    with pytest.raises(ValueError, match="shape"):
        MoleculeTree.from_bonds(4, [0, 1, 2])
    with pytest.raises(ValueError, match="4 sites"):
        MoleculeTree.from_bonds(4, PairList([[0, 1]], 5))


def test_the_constructor_validates_the_forest():
    with pytest.raises(ValueError, match="cycle"):
        MoleculeTree([1, 2, 0, -1])
    with pytest.raises(ValueError, match="cycle"):
        MoleculeTree([-1, 1])  # its own parent
    with pytest.raises(ValueError, match=r"parent\[2\]"):
        MoleculeTree([-1, 0, 3])
    with pytest.raises(ValueError, match=r"parent\[0\]"):
        MoleculeTree([-2, 0])
    with pytest.raises(ValueError, match="integers"):
        MoleculeTree(np.array([-1.0, 0.0]))
    with pytest.raises(ValueError, match="deep"):
        MoleculeTree(np.arange(-1, (1 << 16)))  # depth 2^16
    assert MoleculeTree(np.arange(-1, (1 << 16) - 1)).n_rounds == 16  # depth 2^16 - 1
    tree = MoleculeTree([-1, 0])
    with pytest.raises(ValueError):
        tree.parent[0] = 1  # a constant
    with pytest.raises(ValueError, match="3 sites"):
        as_tree(tree, 3)


CASES = [(tree, N, T) for tree in R.TREES for N, T in ((1, 1), (2, 3), (65, 9), (131, 3))]


def test_the_two_forms_of_the_reference_agree():
    """Pointer jumping over brute-force tables equals the sequential unwrap, one box and a box per frame."""
    deep = 0
    for tree, N, T in CASES:
        for per_frame in (False, True):
            w, x, box, par = R.molecules(tree, N, T, "float64", per_frame)
            k = R.counts_sequential(w, box, par)
            assert np.array_equal(k, R.counts_jumps(w, box, par)), (tree, N, T)
            assert np.abs(R.shift(w, box, k) - x).max() <= 4 * np.spacing(np.abs(x).max() + box.max())
            deep = max(deep, int(np.abs(k).max()))
    assert deep >= 2  # the molecules are longer than the cell


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
def test_make_whole_on_cpu_tensors_and_numpy_matches_the_reference(dtype, per_frame):
    for tree, N, T in CASES:
        w, _, box, par = R.molecules(tree, N, T, dtype, per_frame)
        u, k = R.reference(tree, N, T, dtype, per_frame)
        mt = MoleculeTree(par)
        got, images = make_whole(torch.from_numpy(w.copy()), box, mt, return_images=True)
        assert isinstance(got, torch.Tensor) and not got.is_cuda and images.dtype == torch.int32
        assert np.array_equal(images.numpy(), k), (tree, N, T)
        R.assert_coords(got.numpy(), u, w, f"cpu tensor {tree} N={N} T={T} {dtype}")
        # (the host body widens as ``whole_ref.shift`` does; the two-rounding form is the independent check)
        R.assert_coords(got.numpy(), R.shift_plain(w, box, k), w, f"cpu tensor, plain form {tree} N={N} T={T}", ulps=2)
        arr = w.copy()
        out = make_whole(arr, torch.from_numpy(box.copy()), mt)
        assert isinstance(out, np.ndarray) and out.dtype == w.dtype and np.array_equal(arr, w)  # (input untouched)
        assert np.array_equal(out, got.numpy())
        same = make_whole(arr, box, mt, inplace=True)
        assert same is arr and np.array_equal(arr, out)
        # consequences: a root never moves, the result is whole already and comes back bit for bit
        assert np.array_equal(out[:, par < 0], w[:, par < 0])
        again, zero = make_whole(out, box, mt, return_images=True)
        assert np.array_equal(again, out) and not zero.any()
    w, _, box, par = R.molecules("random", 65, 9, dtype, per_frame)
    assert np.array_equal(make_whole(w, box, MoleculeTree(R.TREES["none"](65))), w)
    bonds = np.stack([np.flatnonzero(par >= 0), par[par >= 0]], axis=1)
    assert np.array_equal(make_whole(w, box, bonds), make_whole(w, box, MoleculeTree.from_bonds(65, bonds)))


def test_edge_behaviour_of_the_host_body():
    w, _, box, par = R.molecules("chain5", 65, 9, "float64", True)
    good, kgood = make_whole(w, box, MoleculeTree(par), return_images=True)
    bad = torch.from_numpy(box.copy())
    bad[4, 1] = 0.0
    with pytest.raises(ValueError, match="positive and finite"):
        make_whole(w, bad, MoleculeTree(par))  # a box on the host is checked
    x = w.copy()
    x[2, 7, 0], x[3, 8, 2] = np.nan, np.inf
    got, k = make_whole(x, box, MoleculeTree(par), return_images=True)
    ref_u, ref_k = R.whole(x, box, par)
    assert np.array_equal(k, ref_k) and np.array_equal(got, ref_u, equal_nan=True)
    assert np.isnan(got[2, 7, 0]) and got[3, 8, 2] == np.inf
    touched = np.zeros(x.shape, dtype=bool)
    touched[2, 7:12, 0] = touched[3, 8:12, 2] = True  # the atom and what hangs below it in its chain of 6
    assert np.array_equal(got[~touched], good[~touched]) and np.array_equal(k[~touched], kgood[~touched])
    with pytest.raises(ValueError, match="shape"):
        make_whole(w[0], box, MoleculeTree(par))
    with pytest.raises(ValueError, match="64 sites"):
        make_whole(w, box, MoleculeTree(par[:64].clip(-1)))
    req = torch.from_numpy(w.copy()).requires_grad_()
    with pytest.raises(ValueError, match="inplace"):
        make_whole(req, box, MoleculeTree(par), inplace=True)
    out = make_whole(req, box, MoleculeTree(par))
    out.sum().backward()
    assert torch.equal(req.grad, torch.ones_like(req)) and np.array_equal(out.detach().numpy(), good)


def test_bonds_without_a_box_or_coordinates_raises_before_touching_a_device(monkeypatch):
    from aggforce_amd import _kernels as K

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(K, "as_device", no_device)
    monkeypatch.setattr(K, "lib", no_device)
    x = np.zeros((4, 3, 3))
    f = np.ones((4, 3, 3))
    bonds = [[0, 1], [1, 2]]
    with pytest.raises(ValueError, match="box"):
        project_forces(x, f, None, bonds=bonds)
    with pytest.raises(ValueError, match="coords"):
        project_forces(None, f, None, constrained_inds=set(), box=[3.0, 3.0, 3.0], bonds=bonds)
    with pytest.raises(ValueError, match="box"):
        project_forces_grid_cv({"l2_regularization": [1.0]}, x, f, n_folds=2, bonds=bonds)
    with pytest.raises(ValueError, match="row 1"):
        project_forces(x, f, None, box=[3.0, 3.0, 3.0], bonds=[[0, 1], [1, 3]])
    with pytest.raises(ValueError, match="shape"):
        project_forces(x, f, None, box=[3.0, 3.0], bonds=bonds)


def test_the_new_keywords_are_optional_and_named():
    for fn in (project_forces, project_forces_grid_cv):
        p = inspect.signature(fn).parameters
        assert p["bonds"].default is None and p["box"].default is None
        assert list(p).index("bonds") > list(p).index("box") and p["bonds"].kind == p["bonds"].POSITIONAL_OR_KEYWORD
    p = inspect.signature(make_whole).parameters
    assert [p[n].kind for n in ("inplace", "return_images")] == [inspect.Parameter.KEYWORD_ONLY] * 2


def test_the_c_abi_of_k11():
    lib = _lib.load()
    n_max = lib.aggf_make_whole_lds_max_sites()
    assert n_max == (160 * 1024 - 48) // 24  # 24 bytes of counts per atom and six lengths in the 160 KiB of a CU
    assert lib.aggf_make_whole_workspace_bytes(0, 5, 3, 0) == 0 == lib.aggf_make_whole_workspace_bytes(7, 0, 3, 1)
    assert lib.aggf_make_whole_workspace_bytes(7, 5, 0, 0) == 7 * 5 * 3 * 4
    assert lib.aggf_make_whole_workspace_bytes(7, 5, 3, 1) == 2 * 7 * 5 * 3 * 4
    assert lib.aggf_make_whole_workspace_bytes(1 << 62, 1 << 20, 3, 1) == 0  # does not fit
    buf = np.zeros(64)
    p = buf.ctypes.data
    call = lambda *a: lib.aggf_make_whole(*a)  # noqa: E731
    assert call(None, 0, 5, 0, None, None, 0, p, 0, None, None, None, 0, 0, None) == 0  # nothing to do
    assert call(p, 2, 0, 1, p, None, 0, p, 3, p, None, None, 0, 0, None) == 0
    for args in [(p, 2, 5, 0, p, None, 0, None, 0, p, None, None, 0, 0, None),          # no box
                 (p, 2, 5, 0, p, None, 0, p, 1, p, None, None, 0, 0, None),             # stride
                 (p, 2, 5, 2, p, None, 0, p, 0, p, None, None, 0, 0, None),             # dtype
                 (p, -1, 5, 0, p, None, 0, p, 0, p, None, None, 0, 0, None),
                 (p, 2, 5, 0, None, None, 0, p, 0, p, None, None, 0, 0, None),          # no parent
                 (p, 2, 5, 0, p, None, 2, p, 0, p, None, None, 0, 0, None),             # rounds without tables
                 (p, 2, 5, 0, p, p, 17, p, 0, p, None, None, 0, 0, None),               # deeper than 2^16
                 (p, 2, 5, 0, p, None, 0, p, 0, p, None, None, 0, 3, None),             # form
                 (p, 2, n_max + 1, 0, p, None, 0, p, 0, p, None, None, 0, 1, None)]:    # beyond the LDS form
        assert call(*args) == -1, args  # AGGF_ERR_ARG
    assert call(p, 2, 5, 0, p, p, 2, p, 0, p, None, p, 2 * 2 * 15 * 4 - 1, 2, None) == -3  # AGGF_ERR_WORKSPACE: short
    assert call(p, 2, 5, 0, p, p, 2, p, 0, p, None, None, 1 << 20, 2, None) == -3
