"""NumPy reference of ``make_whole`` (K11), shared by tests/test_whole_host.py and tests/test_gpu_whole.py, written from
the operation's definition and independent of aggforce_amd/pbc.py:

    n_i = 0 for a root, else (int) rint((x_i - x_parent(i)) * invL)   invL = 1 / L, in the coordinates' dtype
    k_i = n_i + the n of every ancestor of i
    u_i = x_i - k_i L                                                  rounded ONCE (the kernel's fma)

in two forms: ``counts_sequential`` walks every atom's root path parents first (a topological order found by following
parents), ``counts_jumps`` is the pointer-jumping form over tables built here by brute force.  Both give integers, so
they must agree exactly with each other (checked on the host) and with the kernels.  NumPy rounds every float32 /
float64 operation correctly and fuses nothing, which is the arithmetic the kernels write out for n_i.

Two forms of the shift.  ``shift`` forms x - k L in a wider type (float64 for float32, the 64-bit-mantissa long double
of x86-64 for float64) and narrows: within 2^-11 ulp of the correctly rounded value, i.e. of what one fma returns.  It
is the coordinate reference of the tests, held to 1 ulp at the magnitude max(|x|, |u|) (``ulp_bound``) -- the bound
stated for a reference that rounds twice; this one is tighter and is held to the same bound.  (Where long double is
no wider than double the float64 reference rounds twice and ``shift_plain``'s bound applies.)
``shift_plain`` is the two-rounding form in the coordinates' dtype, a multiply and a subtract, written independently
of the library's host body.  Its product is off by at most 1/2 ulp(k L), and k L = x - u is below 2 max(|x|, |u|):
at most 1 ulp at that magnitude; its subtraction and the other side's single rounding add 1/2 ulp each: two results
that both descend from the exact x - k L differ by at most 2 ulp at the magnitude max(|x|, |u|, |u'|)
(``assert_coords(..., ulps=2)``).

Also here: forests (``TREES``), random-walk molecules longer than the cell with every bond component below 0.44 L,
wrapped into [0, L) (``molecules``), boxes (``BOX``, ``frame_boxes``)."""
import functools

import numpy as np

BOX = np.array([4.1, 5.3, 6.7])
MAX_EDGE = 1 << 15
BOND = 0.44  # the largest bond component, in box lengths


def frame_boxes(T, seed):
    """(T, 3): BOX varying by a few percent per frame."""
    return BOX * (1 + 0.03 * np.random.default_rng(seed).uniform(-1, 1, (T, 3)))


# ---------------------------------------------------------------------------------------------------- forests
def chain(n, depth):
    """Chains of ``depth`` bonds laid end to end over n atoms (the last one may be shorter): atom i hangs on i - 1."""
    par = np.arange(-1, n - 1)
    par[:: depth + 1] = -1
    return par


def star(n):
    par = np.zeros(n, dtype=np.int64)
    par[:1] = -1
    return par


def random_tree(n, seed, n_roots=1):
    """A random forest whose labels are shuffled, so that parents come after their children as often as before."""
    rng = np.random.default_rng(seed)
    par = np.full(n, -1, dtype=np.int64)
    for i in range(n_roots, n):
        par[i] = rng.integers(0, i)
    perm = rng.permutation(n)  # old label -> new label
    out = np.full(n, -1, dtype=np.int64)
    out[perm] = np.where(par >= 0, perm[np.maximum(par, 0)], -1)
    return out


def mixed(n, seed):
    """Several molecules and singletons: a random forest on the first two thirds, the rest without bonds."""
    m = max(1, 2 * n // 3)
    par = np.full(n, -1, dtype=np.int64)
    par[:m] = random_tree(m, seed, n_roots=min(m, 3))
    return par


CHAIN_DEPTHS = (1, 2, 3, 4, 5, 16, 17, 130)
TREES = {"none": lambda n: np.full(n, -1, dtype=np.int64), "star": star, "random": lambda n: random_tree(n, 40 + n),
         "mixed": lambda n: mixed(n, 50 + n)}
TREES.update({f"chain{d}": functools.partial(chain, depth=d) for d in CHAIN_DEPTHS})


def depth_of(par):
    """Bonds on the longest root path, by walking every atom up (brute force)."""
    best = 0
    for i in range(len(par)):
        d, a = 0, par[i]
        while a >= 0:
            d, a = d + 1, par[a]
            assert d <= len(par), "cycle"
        best = max(best, d)
    return best


def ancestor(par, i, steps):
    for _ in range(steps):
        if i < 0:
            return -1
        i = par[i]
    return int(i)


def jump_tables(par):
    """(R, n) int64, R the smallest integer with 2^R >= depth: [r][i] the 2^r-th ancestor of i or -1, each found by
    walking up 2^r parents."""
    depth = depth_of(par)
    R = 0
    while (1 << R) < depth:
        R += 1
    return np.array([[ancestor(par, i, 1 << r) for i in range(len(par))] for r in range(R)], dtype=np.int64).reshape(R, len(par))


_ORDERS = {}


def topological(par):
    """The atoms ordered so that every parent comes before its children (kept per forest)."""
    key = np.asarray(par, dtype=np.int64).tobytes()
    if key not in _ORDERS:
        _ORDERS[key] = _topological(par)
    return _ORDERS[key]


def _topological(par):
    level = np.zeros(len(par), dtype=np.int64)
    for i in range(len(par)):
        a = par[i]
        while a >= 0:
            level[i] += 1
            a = par[a]
    return np.argsort(level, kind="stable")


# ---------------------------------------------------------------------------------------------------- the operation
def _lengths(x, box):
    """(L, invL) (T or 1, 1, 3) in x's dtype; a length that is not positive and finite is NaN."""
    L = np.asarray(box, dtype=x.dtype).reshape(-1, 1, 3)
    with np.errstate(all="ignore"):
        L = np.where((L > 0) & np.isfinite(L), L, x.dtype.type(np.nan))
        return L, x.dtype.type(1) / L


def edge_counts(x, box, par):
    """n (T, N, 3) int64."""
    _, invL = _lengths(x, box)
    with np.errstate(all="ignore"):
        q = (x - x[:, np.maximum(par, 0)]) * invL
        n = np.where(np.isfinite(q), np.clip(np.rint(q), -MAX_EDGE, MAX_EDGE), 0).astype(np.int64)
    n[:, par < 0] = 0
    return n


def counts_sequential(x, box, par):
    n = edge_counts(x, box, par)
    k = np.zeros_like(n)
    for i in topological(par):
        k[:, i] = n[:, i] + (k[:, par[i]] if par[i] >= 0 else 0)
    return k


def counts_jumps(x, box, par, tables=None):
    k = edge_counts(x, box, par)
    for jr in (jump_tables(par) if tables is None else tables):
        k = k + np.where((jr >= 0)[None, :, None], k[:, np.maximum(jr, 0)], 0)
    return k


def shift(x, box, k):
    L, _ = _lengths(x, box)
    wide = np.float64 if x.dtype == np.float32 else np.longdouble
    with np.errstate(all="ignore"):
        return (x.astype(wide) - k.astype(x.dtype).astype(wide) * L.astype(wide)).astype(x.dtype)


def shift_plain(x, box, k):
    L, _ = _lengths(x, box)
    with np.errstate(all="ignore"):
        return x - k.astype(x.dtype) * L


def whole(x, box, par):
    """(u, k) of x (T, N, 3) float32 / float64 as stored."""
    k = counts_sequential(x, box, par)
    return shift(x, box, k), k


def ulp_bound(x, u, *more):
    """1 ulp at the magnitude max(|x|, |u|, ...), elementwise (the spacing of the dtype there)."""
    m = np.maximum(np.abs(x), np.abs(u))
    for v in more:
        m = np.maximum(m, np.abs(v))
    return np.spacing(m.astype(x.dtype))


def assert_coords(got, ref, x, what="", ulps=1):
    """|got - ref| <= ulps ulp at max(|x|, |ref|) (ulps = 2, against ``shift_plain``: at max(|x|, |ref|, |got|))."""
    got = np.asarray(got)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin].astype(np.longdouble) - ref[fin])
    bound = (ulp_bound(x, ref) if ulps == 1 else ulps * ulp_bound(x, ref, np.where(fin, got, 0)))[fin]
    worst = float((err / bound).max()) * ulps if err.size else 0.0
    print(f"{what}: max |got - ref| = {worst:.3g} ulp (bound {ulps})")
    assert (err <= bound).all(), f"{what}: {worst:.3g} ulp"


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def molecules(tree, N, T, dtype_name, per_frame, seed=0):
    """(wrapped, open, box, parent) as stored in ``dtype_name``: every atom a random step of at most BOND box lengths
    per component from its parent, roots anywhere in the cell; ``open`` is that walk (roots in the cell), ``wrapped``
    the same wrapped into [0, L), both formed in float64 and cast.  Read-only, shared by the tests."""
    par = TREES[tree](N)
    rng = np.random.default_rng([seed, N, T, sorted(TREES).index(tree)])
    box = (frame_boxes(T, 7 + seed) if per_frame else BOX.copy()).astype(dtype_name)
    L = box.astype(np.float64).reshape(-1, 1, 3)
    step = BOND * L * rng.uniform(-1, 1, (T, N, 3))
    x = L * rng.random((T, N, 3))
    for i in topological(par):
        if par[i] >= 0:
            x[:, i] = x[:, par[i]] + step[:, i]
    w = (x - L * np.floor(x / L)).astype(dtype_name)
    x = x.astype(dtype_name)
    for a in (w, x, box, par):
        a.setflags(write=False)
    return w, x, box, par


@functools.lru_cache(maxsize=None)
def reference(tree, N, T, dtype_name, per_frame, seed=0):
    """(u, k) of ``molecules(...)``'s wrapped coordinates; k int32."""
    w, _, box, par = molecules(tree, N, T, dtype_name, per_frame, seed)
    u, k = whole(w, box, par)
    k = k.astype(np.int32)
    u.setflags(write=False)
    k.setflags(write=False)
    return u, k
