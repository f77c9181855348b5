"""Map validation under periodic boundaries (jaxmapval box=, aggforce_amd.pbc): the restatement the GPU tests compare
with, the call surface, the random stream and the argument checks.  CPU only."""
import inspect
import types

import numpy as np
import pytest
import torch

import cell_ref
import mapval_pbc_ref as pref
import mapval_ref as ref
from aggforce_amd import jaxmapval, mapval, pbc

BOX = np.array([4.1, 5.3, 6.7])
KW = dict(inner=1.0, outer=2.0, width=0.5)


def _sites(T, n, H, seed):
    """Sites uniform over the cell H ((3, 3) or (T, 3, 3))."""
    s = np.random.default_rng(seed).random((T, n, 3))
    return np.einsum("tnk,tkj->tnj", s, np.broadcast_to(H, (T, 3, 3)))


@pytest.mark.parametrize("kind", ["box", "frames_box"] + cell_ref.KINDS)
def test_restated_forces_equal_central_differences_of_the_restated_energy(kind):
    T, n, offset, width = 2, 5, 2.5, 1.7
    if kind == "box":
        H, box = np.diag(BOX), BOX
    elif kind == "frames_box":
        L = BOX * np.array([[1.0, 1.0, 1.0], [1.02, 0.97, 1.01]])
        H, box = np.stack([np.diag(r) for r in L]), L
    else:
        H = cell_ref.cell_of(kind, T)
        box = pref.Tri(H)
    h = 1e-5
    for seed in range(50):  # no pair within 1e-3 of the switch of its image: the energy is smooth over the stencil
        X = _sites(T, n, H, seed)
        if cell_ref.tie_distance(X[:, :, None, :] - X[:, None, :, :], H) > 1e-3:
            break
    else:
        raise AssertionError("no tie-free input found")
    assert pref.displacements(X, box)[2].mean() > 0.3  # images that differ from the raw displacement take part
    G = pref.forces(X, offset, width, box)
    num = np.empty_like(X)
    for idx in np.ndindex(*X.shape):
        Xp, Xm = X.copy(), X.copy()
        Xp[idx] += h
        Xm[idx] -= h
        num[idx] = -(pref.literal_energies(Xp, offset, width, box).sum()
                     - pref.literal_energies(Xm, offset, width, box).sum()) / (2 * h)
    np.testing.assert_allclose(G, num, rtol=1e-7, atol=1e-8 * np.abs(G).max())
    # the diagonal is d = 0: it adds n exp(-(o/w)^2) to every frame's energy
    E1 = pref.literal_energies(X[:, :1], offset, width, box)
    np.testing.assert_allclose(E1, np.exp(-((offset / width) ** 2)), rtol=1e-15)


@pytest.mark.parametrize("kind", cell_ref.KINDS)
def test_the_restated_image_is_the_brute_force_minimum_image_below_the_safe_radius(kind):
    T, n = 3, 40
    H = cell_ref.cell_of(kind, T)
    X = _sites(T, n, H, 11)
    d, x, moved = pref.displacements(X, pref.Tri(H))
    raw = X[:, :, None, :] - X[:, None, :, :]
    checked = 0
    for t in range(T):
        Ht = np.broadcast_to(H, (T, 3, 3))[t]
        best, length = cell_ref.brute_min(raw[t].reshape(-1, 3), Ht)
        short = length < cell_ref.safe_radius(Ht)
        np.testing.assert_allclose(d[t].reshape(-1, 3)[short], best[short], rtol=0, atol=1e-12)
        assert np.all(np.sqrt(x[t].reshape(-1)) >= length - 1e-12)  # beyond: an image, never shorter than the minimum
        checked += int((short & moved[t].reshape(-1)).sum())
    assert checked > 50  # short pairs whose image is not the raw displacement


def test_the_box_form_of_the_restatement_is_its_cell_form_without_off_diagonals():
    X = _sites(4, 6, np.diag(BOX), 3)
    F = np.random.default_rng(4).standard_normal(X.shape)
    a = pref.shift_terms(X, F, 2.0, 1.3, BOX)
    b = pref.shift_terms(X, F, 2.0, 1.3, pref.Tri(np.diag(BOX)))
    np.testing.assert_allclose(a, b, rtol=1e-13)
    far = pref.shift_terms(X, F, 2.0, 1.3, 1e6 * BOX)  # a box far larger than the molecule: the open restatement
    np.testing.assert_allclose(far, ref.shift_terms(X, F, 2.0, 1.3), rtol=1e-13)


# ------------------------------------------------------------------ the call surface
def _no_device():
    def refuse(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    return types.SimpleNamespace(as_device=refuse, gauss_proj=refuse, gauss_shift=refuse, gauss_pair_forces=refuse,
                                 like_input=refuse, lib=refuse)


def test_the_new_names_are_in_pbc_and_the_pinned_surface_is_unchanged():
    E = inspect.Parameter.empty
    want = {"sq_gaussian_energies": [("positions", E), ("offset", E), ("width", E), ("box", E)],
            "sq_gaussian_forces": [("positions", E), ("offset", E), ("width", E), ("box", E)],
            "rsqpg_forces": [("positions", E), ("inner", E), ("outer", E), ("width", E), ("randg", None),
                             ("sq_args", True), ("box", None)]}
    for name, params in want.items():
        got = [(p.name, p.default) for p in inspect.signature(getattr(pbc, name)).parameters.values()]
        assert got == params, name
        assert getattr(pbc, name) is not getattr(jaxmapval, name)
    assert sorted(jaxmapval.__all__) == sorted(["random_uniform_forces", "rsqpg_forces", "random_residual_shift",
                                                "random_force_proj", "mscg_ip", "sq_gaussian_energies",
                                                "sq_gaussian_forces"])
    assert "box" not in inspect.signature(jaxmapval.rsqpg_forces).parameters


CELL = [[8.0, 0, 0], [2.0, 8.0, 0], [-4.0, 2.0, 16.0]]


def test_argument_errors_are_raised_before_any_device_work(monkeypatch):
    monkeypatch.setattr(mapval, "K", _no_device())
    monkeypatch.setattr(pbc, "K", _no_device())
    X = np.zeros((4, 3, 3))
    fused = [lambda **kw: jaxmapval.random_force_proj(X, X, 3, **kw),
             lambda **kw: jaxmapval.random_residual_shift(X, X, 3, **kw),
             lambda **kw: jaxmapval.random_force_proj(X, X, 3, method=pbc.rsqpg_forces, **kw),
             lambda **kw: pbc.rsqpg_forces(X, **kw)]
    for call in fused:
        for bad in ([8.0, 9.0], np.ones((3, 3)), np.ones((4, 9)), np.ones((5, 3)), [[8.0, 9.0, 10.0]]):
            with pytest.raises(ValueError, match="shape"):
                call(box=bad, **KW)
        for bad in ([8.0, 0.0, 9.0], [8.0, np.inf, 9.0], [8.0, np.nan, 9.0], [8.0, -1.0, 9.0]):
            with pytest.raises(ValueError, match="positive and finite"):
                call(box=bad, **KW)
        with pytest.raises(ValueError, match="gradient"):
            call(box=torch.tensor([8.0, 9.0, 10.0], requires_grad=True), **KW)
        with pytest.raises(ValueError, match="gradient"):
            pbc.Cell(torch.tensor(CELL, requires_grad=True))
        # outer beyond half the smallest length; sq_args=False: outer is a squared distance
        with pytest.raises(ValueError, match="half the smallest"):
            call(box=[8.0, 9.0, 10.0], inner=1.0, outer=4.01, width=0.5)
        with pytest.raises(ValueError, match="half the smallest"):
            call(box=[8.0, 9.0, 10.0], inner=1.0, outer=16.1, width=0.5, sq_args=False)
        with pytest.raises(ValueError, match="half the smallest"):
            call(box=np.array([[9.0, 9.0, 10.0]] * 3 + [[9.0, 7.9, 10.0]]), inner=1.0, outer=4.0, width=0.5)
        with pytest.raises(ValueError, match="half the smallest"):  # a cell: safe_radius = min(ax, by, cz) / 2
            call(box=pbc.Cell(CELL), inner=1.0, outer=4.01, width=0.5)
        with pytest.raises(ValueError, match="width"):
            call(box=[8.0, 9.0, 10.0], inner=1.0, outer=2.0, width=0.0)
        # at the bound itself the arguments pass, and the device is what is asked next
        for ok in (dict(box=[8.0, 9.0, 10.0], inner=1.0, outer=4.0, width=0.5),
                   dict(box=[8.0, 9.0, 10.0], inner=1.0, outer=16.0, width=0.5, sq_args=False),
                   dict(box=pbc.Cell(CELL), inner=1.0, outer=4.0, width=0.5)):
            with pytest.raises(AssertionError, match="device work"):
                call(**ok)
    for fn in (pbc.sq_gaussian_forces, pbc.sq_gaussian_energies):
        with pytest.raises(ValueError, match="shape"):
            fn(np.zeros((4, 3)), 1.0, 1.0, [8.0, 9.0, 10.0])
        with pytest.raises(ValueError, match="shape"):
            fn(X, 1.0, 1.0, np.ones((4, 9)))
        with pytest.raises(ValueError, match="positive and finite"):
            fn(X, 1.0, 1.0, [8.0, 0.0, 10.0])
        with pytest.raises(ValueError, match="width"):
            fn(X, 1.0, 0.0, [8.0, 9.0, 10.0])
        with pytest.raises(ValueError, match="gradient"):
            fn(X, 1.0, 1.0, torch.tensor([8.0, 9.0, 10.0], requires_grad=True))
        with pytest.raises(ValueError, match="per-frame Cell"):
            fn(X, 1.0, 1.0, pbc.Cell(np.tile(np.array(CELL), (5, 1, 1))))


def _fake_kernels(record):
    """Stand-in for aggforce_amd._kernels: records what the fused path asks for, box included."""

    def gauss_proj(X, F, o, width, box=None):
        record.update(offsets=o.numpy().copy(), width=width, kind="proj", box=box)
        return torch.zeros(o.numel(), dtype=torch.float64)

    def gauss_shift(X, F, o, width, box=None):
        record.update(offsets=o.numpy().copy(), width=width, kind="shift", box=box)
        z = torch.zeros(o.numel(), dtype=torch.float64)
        return z, z

    return types.SimpleNamespace(as_device=lambda x: torch.as_tensor(x), gauss_proj=gauss_proj, gauss_shift=gauss_shift)


@pytest.mark.parametrize("method", ["default", "pbc"])
@pytest.mark.parametrize("fn", ["random_force_proj", "random_residual_shift"])
def test_the_periodic_call_is_fused_with_the_offsets_and_generator_state_of_the_open_call(monkeypatch, fn, method):
    record = {}
    monkeypatch.setattr(mapval, "K", _fake_kernels(record))
    X = np.zeros((4, 3, 3), dtype=np.float32)
    extra = {} if method == "default" else {"method": pbc.rsqpg_forces}
    boxes = {"lengths": (np.array([8.0, 9.0, 10.0]), (3,)), "frames": (np.full((4, 3), 9.0), (4, 3)),
             "cell": (pbc.Cell(CELL), (4, 9)), "none": (None, None)}
    for S in (1, 37, 1001):
        for name, (box, shape) in boxes.items():
            record.clear()
            kw = dict(KW) if box is None else dict(KW, box=box)
            if box is None and method == "default":
                continue  # the open call of the default method: tests/test_mapval_host.py
            rg = np.random.default_rng(7)
            vals = getattr(jaxmapval, fn)(X, X, n_samples=S, randg=rg, average=False, **kw, **extra)
            assert len(vals) == S and record["kind"] == ("proj" if fn == "random_force_proj" else "shift")
            want, w = ref.offsets(7, S, **KW)
            np.testing.assert_array_equal(record["offsets"], want)
            assert record["width"] == w
            tail = np.random.default_rng(7)
            for _ in range(S):
                tail.random()
            assert rg.random() == tail.random()
            if box is None:
                assert record["box"] is None
            else:  # the normalised box in the coordinates' dtype, contiguous
                b = record["box"]
                assert tuple(b.shape) == shape and b.dtype == torch.float32 and b.is_contiguous()
                if name == "cell":
                    np.testing.assert_array_equal(b[2].numpy(), np.array(CELL, dtype=np.float32).reshape(9))


def test_any_other_method_is_handed_the_box_like_every_other_keyword(monkeypatch):
    monkeypatch.setattr(mapval, "K", _fake_kernels({}))
    X = np.zeros((4, 3, 3))
    seen = []

    def method(coords, randg=None, **kw):
        seen.append(kw)
        raise KeyError("reached")

    with pytest.raises(KeyError):
        jaxmapval.random_force_proj(X, X, 2, method=method, box=[8.0, 9.0, 10.0], scale=2.0)
    assert seen == [{"box": [8.0, 9.0, 10.0], "scale": 2.0}]
