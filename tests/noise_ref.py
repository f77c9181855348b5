"""Host reference for the device noise stream, for tests/test_noise_ref_host.py and tests/test_gpu_noise_stream.py.
NumPy only; nothing under aggforce_amd/ imports it and it imports nothing from there.

Written from the published algorithm (Salmon, Moraes, Dror & Shaw, "Parallel random numbers: as easy as 1, 2, 3",
SC'11: Philox4x32-10) and from the contract of the library, not from its kernels:

    element g of a stream          flat index g = (frame_offset + t) * row + 3 * site + dim  (row = 3 * sites)
    quad q = g >> 2, lane g & 3    counter = (q lo, q hi, stream lo, stream hi), key = (seed lo, seed hi)
    words (0, 1) -> lanes 0, 1     words (2, 3) -> lanes 2, 3
    u = (word + 0.5) / 2^32        rad = sqrt(-2 ln u1), angle = fl64(6.283185307179586476925 * u2)
    even lane = rad cos(angle)     odd lane = rad sin(angle)
    stream word 0: synth_normal    stream word 1: the sites of the conditional normal (noise=None)
    call k of one augmenter        seed_k = (seed + k * 0x9E3779B97F4A7C15) mod 2^64

Everything up to the uniforms is integer arithmetic and exact; the angle is the float64 product (as on the device);
ln, sqrt, sin and cos are evaluated in numpy.longdouble (64-bit mantissa on x86-64) and the result is rounded to
float64 once.  ``extended=False`` evaluates them in float64 instead (the statistical tests of the stream do not need
more and draw 1e7 values several times).

``mutation`` replaces ONE step by a plausible mistake (MUTATIONS); the sensitivity test of the GPU module uses it to
show that the comparison would notice each of them.
"""
import numpy as np

U = 2.0 ** -53
M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers of words 0 and 2
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl increments of the two key words
GOLDEN_GAMMA = 0x9E3779B97F4A7C15        # per-call seed increment
TWO_PI = 6.283185307179586476925         # (rounds to the float64 nearest 2 pi)
STREAM_SYNTH, STREAM_SITES = 0, 1
Z_MAX = float(np.sqrt(66.0 * np.log(2.0)))  # u1 >= 2^-33: |z| <= sqrt(-2 ln 2^-33)

MUTATIONS = ("rounds9", "multipliers_swapped", "key_not_bumped", "stream_ignored", "counter_high_dropped",
             "key_high_dropped", "sincos_swapped", "lanes_reversed", "half_omitted", "call_seed_not_advanced")

_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is not an extended type on this machine"


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10, m0=M0, m1=M1, bump=True):
    """Philox4x32 on uint64 arrays holding 32-bit words (broadcast against each other): the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK32 for v in (c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(m0), np.uint64(m1)
    for _ in range(rounds):
        p0 = m0 * c0      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK32
        if bump:
            k0 = (k0 + np.uint64(W0)) & _MASK32
            k1 = (k1 + np.uint64(W1)) & _MASK32
    return c0, c1, c2, c3


def words(seed, stream, q, mutation=None):
    """The four 32-bit words of quad(s) ``q`` of stream word ``stream`` under ``seed`` (Python ints of any size are
    taken mod 2^64)."""
    seed, stream = int(seed) % 2**64, int(stream) % 2**64
    q = np.asarray(q, dtype=np.uint64)
    kw = {}
    if mutation == "rounds9":
        kw["rounds"] = 9
    elif mutation == "multipliers_swapped":
        kw["m0"], kw["m1"] = M1, M0
    elif mutation == "key_not_bumped":
        kw["bump"] = False
    elif mutation == "stream_ignored":
        stream = 0
    q_hi = q >> _S32
    if mutation == "counter_high_dropped":
        q_hi = np.zeros_like(q)
    k_hi = 0 if mutation == "key_high_dropped" else seed >> 32
    return philox4x32_10(q & _MASK32, q_hi, stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, k_hi, **kw)


def _uniform(word, mutation):
    half = 0.0 if mutation == "half_omitted" else 0.5
    return (word.astype(np.float64) + half) / 4294967296.0  # exact: 33 bits


def _box_muller(u1, u2, extended):
    """(rad cos, rad sin) rounded to float64 once."""
    wide = np.longdouble if extended else np.float64
    angle = (TWO_PI * u2).astype(wide)  # the float64 product, as on the device
    with np.errstate(divide="ignore", invalid="ignore"):  # (only a mutated reference can take ln 0)
        rad = np.sqrt(wide(-2) * np.log(u1.astype(wide)))
        return (rad * np.cos(angle)).astype(np.float64), (rad * np.sin(angle)).astype(np.float64)


def normal(seed, stream, g, mutation=None, extended=True):
    """Standard normals at the flat indices ``g`` (any integer array, any order) of one stream: float64."""
    g = np.asarray(g, dtype=np.uint64)
    w = words(seed, stream, g >> np.uint64(2), mutation)
    lane = (g & np.uint64(3)).astype(np.int64)
    if mutation == "lanes_reversed":
        lane = 3 - lane
    upper = lane >= 2
    u1 = _uniform(np.where(upper, w[2], w[0]), mutation)
    u2 = _uniform(np.where(upper, w[3], w[1]), mutation)
    c, s = _box_muller(u1, u2, extended)
    if mutation == "sincos_swapped":
        c, s = s, c
    return np.where(lane % 2 == 0, c, s)


def normal_range(seed, stream, g0, n, mutation=None, extended=True):
    """normal(seed, stream, arange(g0, g0 + n)) with every quad computed once."""
    g0, n = int(g0), int(n)
    q0, q1 = g0 >> 2, (g0 + n - 1) >> 2
    q = np.uint64(q0) + np.arange(q1 - q0 + 1, dtype=np.uint64)
    w = words(seed, stream, q, mutation)
    z = np.empty((q.size, 4))
    for h in (0, 1):
        c, s = _box_muller(_uniform(w[2 * h], mutation), _uniform(w[2 * h + 1], mutation), extended)
        if mutation == "sincos_swapped":
            c, s = s, c
        z[:, 2 * h], z[:, 2 * h + 1] = c, s
    if mutation == "lanes_reversed":
        z = z[:, ::-1]
    lo = g0 - 4 * q0
    return z.reshape(-1)[lo:lo + n].copy()


def lattice_coord(N):
    """(N, 3) integer lattice position of site a: a % side, (a // side) % side, a // side^2, with ``side`` the smallest
    integer whose cube holds N sites."""
    side = 1
    while side ** 3 < N:
        side += 1
    a = np.arange(N)
    return np.stack([a % side, (a // side) % side, a // (side * side)], axis=1).astype(np.float64)


def synth_normal_ref(T, N, dtype, seed, frame_offset=0, mean=0.0, sigma=1.0, lattice=0.0, mutation=None,
                     with_z=False):
    """K.synth_normal: mean + lattice * coord(site, dim) + sigma * z over stream word 0, (T, N, 3), computed in float64
    and cast to ``dtype``; ``with_z`` also returns the float64 z (the tolerance is stated in terms of it)."""
    row = 3 * N
    z = normal_range(seed, STREAM_SYNTH, int(frame_offset) * row, T * row, mutation).reshape(T, N, 3)
    mu = np.full((N, 3), float(mean))
    if lattice != 0.0:
        mu = mu + float(lattice) * lattice_coord(N)
    out = (mu[None] + float(sigma) * z).astype(dtype)
    return (out, z) if with_z else out


def site_noise_ref(T, n_cg, dtype, seed, frame_offset=0, mutation=None):
    """The standard normals of the generated sites (noise=None): stream word 1, row 3 n_cg, (T, n_cg, 3)."""
    row = 3 * n_cg
    z = normal_range(seed, STREAM_SITES, int(frame_offset) * row, T * row, mutation)
    return z.reshape(T, n_cg, 3).astype(dtype)


def call_seed(seed, k, mutation=None):
    """Seed of call ``k`` (0, 1, ...) of an augmenter created with ``seed``."""
    if mutation == "call_seed_not_advanced":
        k = 0
    return (int(seed) + int(k) * GOLDEN_GAMMA) % 2**64
