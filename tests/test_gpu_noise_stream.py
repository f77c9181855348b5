"""GPU: every random number the library draws on the device, value by value against tests/noise_ref.py
(Philox4x32-10 + Box-Muller from the published algorithm; itself pinned by tests/test_noise_ref_host.py).

The three consumers of ``normal_quad`` -- ``synth_normal_kernel`` (stream word 0), ``noise_sites_kernel`` and
``augment_kernel`` (stream word 1) -- and the Python bookkeeping above them (per-call seed, frame offset, dtype).

Tolerance (u = 2^-53), derived, not tuned: everything up to the uniforms is integer arithmetic and exact, the angle
is the same double on both sides; what remains is the device's ``log`` (1 ulp) under a ``sqrt``, ``sincos`` (2 ulp)
and two roundings, about 4 ulp = 8 u relative, doubled:

    float64 output                         |z_dev - z_ref| <= 16 u |z_ref|
    float32 output                         ... + 1/2 ulp32(ref)
    synth_normal with mean / sigma         16 u sigma |z_ref| + 2 u |ref|   (+ 1/2 ulp32(ref))

An error in the integer part is O(1).  The worst ratios measured are printed when the module finishes (run with -s)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import noise_ref as R  # noqa: E402
from aggforce_amd import LinearMap, Trajectory  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.trajectory import AugmentedTrajectory, CondNormal, JCondNormal, SimpleCondNormal  # noqa: E402
from oracle import aggforce_oracle as orc  # noqa: E402

U = R.U
KBT = 0.6955215
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {np.float32: torch.float32, np.float64: torch.float64}
SEEDS = [0, 1, 42100, 2**32, 2**32 + 1, 2**64 - 1]
MEASURED = {}  # (kernel, output dtype) -> worst |dev - ref| / (u |ref|) (float64) or / bound (float32)


@pytest.fixture(scope="module", autouse=True)
def report_measured():
    yield
    for (kernel, dt), worst in sorted(MEASURED.items()):
        unit = "u |z_ref| (bound 16)" if dt == "float64" else "of the float32 bound"
        print(f"\nnoise stream, {kernel} {dt}: worst deviation {worst:.3f} {unit}")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def excess(dev, ref, z=None, sigma=1.0):
    """Worst |dev - ref| / bound over the array (inf where dev is not a number): <= 1 passes.  ``ref``: the float64
    reference; ``z``: the float64 standard normals behind it when it is mean + sigma z (else ref is z itself)."""
    dev = np.asarray(dev)
    ref = np.asarray(ref, dtype=np.float64)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    bound = 16 * U * np.abs(ref) if z is None else 16 * U * np.abs(sigma * z) + 2 * U * np.abs(ref)
    if dev.dtype == np.float32:
        bound = bound + 0.5 * ulp32(ref)
    else:
        assert dev.dtype == np.float64
    err = np.abs(dev.astype(np.float64) - ref)
    ratio = np.where(np.isfinite(err), err / bound, np.inf)
    return float(ratio.max())


def measure(kernel, dev, ref):
    dev = np.asarray(dev)
    if dev.dtype == np.float64:
        worst = float(np.max(np.abs(dev - ref) / (U * np.abs(ref))))
    else:
        worst = excess(dev, ref)
    key = (kernel, dev.dtype.name)
    MEASURED[key] = max(MEASURED.get(key, 0.0), worst)


@functools.lru_cache(maxsize=None)
def site_ref(T, n_cg, seed, frame_offset, mutation=None):
    out = R.site_noise_ref(T, n_cg, np.float64, seed, frame_offset, mutation=mutation)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synth_ref(T, N, seed, frame_offset, mean=0.0, sigma=1.0, lattice=0.0, mutation=None):
    out, z = R.synth_normal_ref(T, N, np.float64, seed, frame_offset, mean, sigma, lattice, mutation=mutation, with_z=True)
    out.setflags(write=False)
    z.setflags(write=False)
    return out, z


def grid_cap(source, function):
    """The cap on the number of 256-thread workgroups that ``function`` of csrc/``source`` launches (`if (g > CAP)`)."""
    text = open(os.path.join(ROOT, "aggforce_amd", "csrc", source)).read()
    m = re.search(re.escape(function) + r".*?if \(g > (\d+)\) g = (\d+);", text, re.S)
    assert m and m.group(1) == m.group(2), f"no grid cap found in {function}"
    return int(m.group(1))


# ---------------------------------------------------------------------------------------------- synth_normal
SYNTH_SHAPES = [(1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 1, 3), (7, 5, 3), (33, 9, 1_000_001), (4, 50, 0), (2, 50, 2**33)]


def synth_dev(T, N, dt, seed, frame_offset, **kw):
    return K.synth_normal(T, N, TDT[dt], seed, frame_offset, **kw).cpu().numpy()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_synth_normal_values(dt):
    """Shards that start at every lane of a quad, rows that are not whole quads, a quad index beyond 2^32 (frame
    offset 2^33), seeds whose high word matters."""
    for T, N, off in SYNTH_SHAPES:
        for seed in SEEDS:
            dev = synth_dev(T, N, dt, seed, off)
            ref, _ = synth_ref(T, N, seed, off)
            assert dev.dtype == dt and excess(dev, ref) <= 1, (T, N, off, seed, excess(dev, ref))
            measure("synth_normal", dev, ref)
    assert (2**33 * 150) >> 2 > 2**32


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_synth_normal_mean_sigma_and_lattice(dt):
    for T, N, off, lattice in [(7, 5, 3, 0.0), (4, 50, 0, 0.0), (3, 1, 1, 1.5), (3, 8, 1, 1.5), (3, 9, 1, 1.5),
                               (3, 27, 1, 1.5), (3, 28, 1, 1.5), (2, 28, 5, -0.75)]:
        dev = synth_dev(T, N, dt, 42100, off, mean=1.0, sigma=3.0, lattice=lattice)
        ref, z = synth_ref(T, N, 42100, off, 1.0, 3.0, lattice)
        assert excess(dev, ref, z, 3.0) <= 1, (T, N, off, lattice, excess(dev, ref, z, 3.0))
    # the lattice alone (sigma = 0): exact
    dev = synth_dev(2, 28, dt, 5, 0, mean=0.25, sigma=0.0, lattice=1.5)
    assert np.array_equal(dev, np.broadcast_to(0.25 + 1.5 * R.lattice_coord(28), (2, 28, 3)).astype(dt))


def test_synth_normal_past_the_grid_stride_cap():
    """More quads than the capped launch has threads: the grid-stride loop takes a second pass (odd row length)."""
    T, N = 1400, 2001
    cap = grid_cap("aggf_util.hip", "static dim3 stream_grid")
    assert cap * 256 < T * N * 3 // 4 < 2 * cap * 256
    dev = synth_dev(T, N, np.float64, 42100, 0)
    ref, _ = synth_ref(T, N, 42100, 0)
    assert np.isfinite(dev).all() and np.max(np.abs(dev)) <= R.Z_MAX
    assert excess(dev, ref) <= 1, excess(dev, ref)
    measure("synth_normal", dev, ref)
    synth_ref.cache_clear()  # (67 MB; the small cases are recomputed in no time)


# ------------------------------------------------------------------ the generated sites with mean 0, var 1: y = eps
SITE_CASES = [(T, n_cg, off) for n_cg in (1, 3, 5, 16) for T in (5, 257) for off in (0, 3, 1_000_001)]


def sites_dev(T, n_cg, aug_dt, out_dt, seed, frame_offset, kbt=2.0):
    mean = torch.zeros((T, n_cg, 3), dtype=TDT[aug_dt], device="cuda")
    y, fa = K.condnormal_sites(mean, 1.0, kbt, None, seed, frame_offset, TDT[out_dt])
    return y.cpu().numpy(), fa.cpu().numpy()


def augment_dev(T, n_cg, traj_dt, aug_dt, seed, frame_offset, kbt=2.0):
    """Two real atoms: atom 0 belongs to site 0, atom 1 (weight 1/2) to the last site.  kbt and the weights are powers
    of two, so every product below is exact."""
    rng = np.random.default_rng(T * 1000 + n_cg)
    coords = rng.random((T, 2, 3)).astype(traj_dt)
    forces = rng.standard_normal((T, 2, 3)).astype(traj_dt)
    M = np.zeros((n_cg, 2))
    M[0, 0], M[n_cg - 1, 1] = 1.0, 0.5
    cols = K.premap_columns(M, TDT[aug_dt], "cuda")
    mean = torch.zeros((T, n_cg, 3), dtype=TDT[aug_dt], device="cuda")
    oc, of = K.condnormal_augment(torch.from_numpy(coords).cuda(), torch.from_numpy(forces).cuda(), cols, n_cg, mean,
                                  1.0, kbt, None, seed, frame_offset)
    oc, of = oc.cpu().numpy(), of.cpu().numpy()
    out_dt = np.promote_types(traj_dt, aug_dt)
    assert oc.dtype == of.dtype == out_dt and np.array_equal(oc[:, :2], coords.astype(out_dt))
    y = oc[:, 2:]
    # F + kbt M' r with r = eps: one rounding, in the output type
    want = forces.astype(out_dt) + (kbt * np.stack([y[:, 0], 0.5 * y[:, n_cg - 1]], axis=1)).astype(out_dt)
    assert np.array_equal(of[:, :2], want)
    return y, of[:, 2:]


def as_rounded(y, aug_dt):
    """A float32 augmenter rounds eps to float32 whatever the output type: judge the values as float32."""
    return y.astype(np.float32) if aug_dt == np.float32 else y


@pytest.mark.parametrize("aug_dt,out_dt", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float64)])
def test_condnormal_sites_draw_the_reference_stream(aug_dt, out_dt):
    for T, n_cg, off in SITE_CASES + [(3, 16, 2**33)]:
        for seed in (42100, 2**64 - 1):
            y, fa = sites_dev(T, n_cg, aug_dt, out_dt, seed, off)
            ref = site_ref(T, n_cg, seed, off)
            assert y.dtype == out_dt and np.array_equal(fa, -2.0 * y)
            if aug_dt == np.float32:
                assert np.array_equal(y, y.astype(np.float32).astype(out_dt))
            y = as_rounded(y, aug_dt)
            assert excess(y, ref) <= 1, (T, n_cg, off, seed, excess(y, ref))
            measure("condnormal_sites", y, ref)


@pytest.mark.parametrize("traj_dt,aug_dt", [(np.float32, np.float32), (np.float64, np.float64), (np.float64, np.float32),
                                            (np.float32, np.float64)])
def test_condnormal_augment_draws_the_reference_stream(traj_dt, aug_dt):
    """T % 4 != 0: the last frame block of augment_kernel is short."""
    for T, n_cg, off in SITE_CASES:
        y, fa = augment_dev(T, n_cg, traj_dt, aug_dt, 42100, off)
        ref = site_ref(T, n_cg, 42100, off)
        assert np.array_equal(fa, -2.0 * y)
        y = as_rounded(y, aug_dt)
        assert excess(y, ref) <= 1, (T, n_cg, off, excess(y, ref))
        measure("condnormal_augment", y, ref)


@pytest.mark.parametrize("n_cg", [700, 1300])
def test_condnormal_augment_with_two_and_one_frames_per_block(n_cg):
    """float64 sites: 4 frames of 700 sites (67 200 bytes) do not fit the LDS budget of 60 000 bytes -> 2 frames per
    workgroup; 2 frames of 1300 sites (62 400 bytes) do not either -> 1."""
    y, _ = augment_dev(5, n_cg, np.float64, np.float64, 2**32 + 1, 3)
    ref = site_ref(5, n_cg, 2**32 + 1, 3)
    assert excess(y, ref) <= 1, excess(y, ref)
    measure("condnormal_augment", y, ref)


def test_condnormal_sites_past_the_grid_stride_cap():
    """More quads than the capped launch has threads, from a frame offset that is not quad-aligned."""
    T, n_cg, off = 2049, 2731, 3
    cap = grid_cap("aggf_augment.hip", 'extern "C" int aggf_condnormal_sites')
    assert cap * 256 < T * n_cg * 3 // 4 < 2 * cap * 256 and (off * n_cg * 3) % 4 != 0
    y, fa = sites_dev(T, n_cg, np.float32, np.float32, 42100, off)
    ref = R.site_noise_ref(T, n_cg, np.float64, 42100, off)
    assert np.isfinite(y).all() and np.max(np.abs(y)) <= R.Z_MAX * (1 + 2.0 ** -23) and np.array_equal(fa, -2.0 * y)
    assert excess(y, ref) <= 1, excess(y, ref)
    measure("condnormal_sites", y, ref)


# ------------------------------------------------------------------------- with a real premap, mean and variance
def system(T=300, N=24, n_cg=5, seed=5, dt=np.float32):
    rng = np.random.default_rng(seed)
    coords = (5 * rng.random((T, N, 3))).astype(dt)
    forces = (30 * rng.standard_normal((T, N, 3))).astype(dt)
    cmat = orc.list_mapping_matrix([[4 * i, 4 * i + 1] for i in range(n_cg)], N)
    return coords, forces, cmat


@pytest.mark.parametrize("dt,tol_c,tol_f", [(np.float32, 1e-6, 2e-5), (np.float64, 1e-9, 1e-9)])
def test_extended_arrays_with_drawn_noise_equal_the_oracle_on_reference_noise(dt, tol_c, tol_f):
    coords, forces, cmat = system(dt=dt)
    N, n_cg, var, seed = cmat.shape[1], cmat.shape[0], 0.01, 42100
    eps_ref = site_ref(len(coords), n_cg, seed, 0).astype(dt)
    oc, of = orc.augment(coords, forces, cmat, var, KBT, eps_ref, dtype=dt)
    a = CondNormal(cov=var, premap=LinearMap(cmat), seed=seed, dtype=dt)
    aug = AugmentedTrajectory.from_trajectory(t=Trajectory(coords=coords, forces=forces), augmenter=a, kbt=KBT)
    assert aug.coords.dtype == dt and rel(aug.coords, oc) < tol_c and rel(aug.forces, of) < tol_f
    y, fa, _ = CondNormal(cov=var, premap=LinearMap(cmat), seed=seed, dtype=dt).noise_sites(coords, KBT)
    assert rel(y.cpu().numpy(), oc[:, N:]) < tol_c and rel(fa.cpu().numpy(), of[:, N:]) < tol_f
    # the noise itself, recovered from the generated sites: O(1) off if a wrong element had been drawn
    got = (np.asarray(aug.coords[:, N:], np.float64) - orc.trjdot(coords.astype(np.float64), cmat)) / np.sqrt(var)
    assert np.max(np.abs(got - eps_ref)) < (1e-4 if dt == np.float32 else 1e-12)


# ------------------------------------------------------------------------------ the bookkeeping of gausstraj.py
def draws(make, n_calls, source):
    a = make()
    return [np.asarray(a.sample(source)) for _ in range(n_calls)]


@pytest.mark.parametrize("seed", [42100, 2**64 - 5])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_call_k_of_an_augmenter_draws_from_call_seed_k(seed, dt):
    """sample, augment_trajectory and noise_sites of a scalar covariance: stream word 1 under call_seed(seed, k), also
    where seed + k * increment wraps past 2^64; frame_offset shifts the flat index."""
    T, n, off = 6, 3, 7
    zeros = np.zeros((T, n, 3), dtype=dt)
    make = lambda: CondNormal(cov=1.0, seed=seed, dtype=dt, frame_offset=off)  # noqa: E731
    assert (seed + 2 * R.GOLDEN_GAMMA >= 2**64) or seed == 42100
    for k, y in enumerate(draws(make, 3, zeros)):
        ref = site_ref(T, n, R.call_seed(seed, k), off)
        assert y.dtype == dt and excess(y, ref) <= 1, (k, excess(y, ref))
    a, b = make(), make()
    for k in range(3):
        oc, _ = a.augment_trajectory(zeros, zeros, 2.0)
        y, fa, _ = b.noise_sites(zeros, 2.0)
        ref = site_ref(T, n, R.call_seed(seed, k), off)
        assert excess(np.asarray(oc)[:, n:], ref) <= 1 and excess(y.cpu().numpy(), ref) <= 1, k
    # without the offset: the first frames of the stream
    y0 = CondNormal(cov=1.0, seed=seed, dtype=dt).sample(zeros)
    assert excess(y0, site_ref(T, n, R.call_seed(seed, 0), 0)) <= 1
    assert not np.array_equal(y0, draws(make, 1, zeros)[0])


def test_astype_continues_the_call_count():
    T, n, seed = 6, 3, 42100
    a = CondNormal(cov=1.0, seed=seed)
    y0 = a.sample(np.zeros((T, n, 3), dtype=np.float32))
    b = a.astype(np.float64)
    y1 = b.sample(np.zeros((T, n, 3)))
    assert y0.dtype == np.float32 and excess(y0, site_ref(T, n, R.call_seed(seed, 0), 0)) <= 1
    assert y1.dtype == np.float64 and excess(y1, site_ref(T, n, R.call_seed(seed, 1), 0)) <= 1
    assert excess(np.asarray(b.sample(np.zeros((T, n, 3)))), site_ref(T, n, R.call_seed(seed, 2), 0)) <= 1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_simple_condnormal_draws_the_same_stream(dt):
    T, n, seed = 6, 4, 2**32 + 1
    s = SimpleCondNormal(var=1.0, seed=seed, dtype=dt)
    zeros = np.zeros((T, n, 3), dtype=dt)
    for k in range(2):
        y = np.asarray(s.sample(zeros))
        assert y.dtype == dt and excess(y, site_ref(T, n, R.call_seed(seed, k), 0)) <= 1, k


@pytest.mark.parametrize("off", [0, 11])
def test_full_covariance_draws_from_stream_zero_under_the_call_seed(off):
    """eps of the full-covariance form = synth_normal (stream word 0) under the same per-call seed."""
    coords, _, cmat = system(T=257, dt=np.float64)
    n, seed = cmat.shape[0], 2**64 - 5
    B = np.random.default_rng(3).standard_normal((3 * n, 3 * n))
    cov = 0.05 * (B @ B.T / (3 * n) + np.eye(3 * n))
    a = JCondNormal(cov=cov, premap=LinearMap(cmat).flat_call, seed=seed, frame_offset=off)
    assert a.dtype == np.float64
    for k in range(3):
        eps_ref, _ = synth_ref(257, n, R.call_seed(seed, k), off)
        oy = orc.condnormal_full_sample(coords, cmat, cov, eps_ref)
        assert rel(a.sample(coords), oy) < 1e-12, k
    # noise_sites and augment_trajectory of the full form go through the same draw
    eps_ref, _ = synth_ref(257, n, R.call_seed(seed, 3), off)
    y, _, _ = a.noise_sites(coords, KBT)
    assert rel(y.cpu().numpy(), orc.condnormal_full_sample(coords, cmat, cov, eps_ref)) < 1e-12


# ------------------------------------------------------------------------------------------------- sensitivity
@functools.lru_cache(maxsize=None)
def probe_outputs():
    """Device outputs of the probes, drawn once."""
    zeros = np.zeros((5, 3, 3))
    a = CondNormal(cov=1.0, seed=42100, dtype=np.float64)
    return {
        "synth_lanes": synth_dev(7, 5, np.float64, 42100, 3),
        "synth_high_counter": synth_dev(2, 50, np.float64, 1, 2**33),
        "synth_high_key": synth_dev(4, 50, np.float64, 2**32 + 1, 0),
        "synth_affine_f32": synth_dev(7, 5, np.float32, 42100, 3, mean=1.0, sigma=3.0, lattice=1.5),
        "sites": sites_dev(5, 5, np.float64, np.float64, 42100, 3)[0],
        "sites_high_counter": sites_dev(3, 16, np.float64, np.float64, 42100, 2**33)[0],
        "augment_f32": augment_dev(5, 5, np.float32, np.float32, 42100, 3)[0],
        "calls": np.stack([np.asarray(a.sample(zeros)) for _ in range(3)]),
    }


def probe_excess(name, dev, m):
    """The comparison of the tests above, against a reference with mutation ``m`` (None: the true one)."""
    if name == "synth_lanes":
        return excess(dev, R.synth_normal_ref(7, 5, np.float64, 42100, 3, mutation=m))
    if name == "synth_high_counter":
        return excess(dev, R.synth_normal_ref(2, 50, np.float64, 1, 2**33, mutation=m))
    if name == "synth_high_key":
        return excess(dev, R.synth_normal_ref(4, 50, np.float64, 2**32 + 1, 0, mutation=m))
    if name == "synth_affine_f32":
        ref, z = R.synth_normal_ref(7, 5, np.float64, 42100, 3, 1.0, 3.0, 1.5, mutation=m, with_z=True)
        return excess(dev, ref, z, 3.0)
    if name == "sites":
        return excess(dev, R.site_noise_ref(5, 5, np.float64, 42100, 3, mutation=m))
    if name == "sites_high_counter":
        return excess(dev, R.site_noise_ref(3, 16, np.float64, 42100, 2**33, mutation=m))
    if name == "augment_f32":
        return excess(dev, R.site_noise_ref(5, 5, np.float64, 42100, 3, mutation=m))
    if name == "calls":
        ref = np.stack([R.site_noise_ref(5, 3, np.float64, R.call_seed(42100, k, m), 0, mutation=m) for k in range(3)])
        return excess(dev, ref)
    raise KeyError(name)


# the probes that MUST notice (the others may: a mutation of the rounds is seen everywhere)
MUST_CATCH = {
    "stream_ignored": {"sites", "sites_high_counter", "augment_f32", "calls"},
    "counter_high_dropped": {"synth_high_counter", "sites_high_counter"},
    "key_high_dropped": {"synth_high_key"},
    "call_seed_not_advanced": {"calls"},
}


def test_probes_pass_against_the_true_reference():
    for name, dev in probe_outputs().items():
        assert probe_excess(name, dev, None) <= 1, name


@pytest.mark.parametrize("m", R.MUTATIONS)
def test_a_mutated_reference_fails_the_same_comparison(m):
    """One mistake in the reference at a time: the comparison that passes against the true reference must FAIL.  (A
    mistake in the kernel is the same disagreement seen from the other side.)"""
    caught = {name for name, dev in probe_outputs().items() if not probe_excess(name, dev, m) <= 1}
    print(m, "caught by", sorted(caught))
    want = MUST_CATCH.get(m, {"synth_lanes", "sites", "calls"})
    assert want <= caught, f"{m}: not noticed by {sorted(want - caught)}"
