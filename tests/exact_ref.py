"""Exact references for the contraction kernels (tests/test_exact_ref_host.py, tests/test_gpu_exact.py).

If every input of a sum of products is a small integer and

    L * A * B <= 2**p        (L: reduction length; A, B: bounds of the two operands' magnitudes AFTER any group sum;
                              p = 24 where float32 appears anywhere in the chain, 53 otherwise)

then every partial sum, in any order, is an integer of magnitude <= 2**p and therefore exactly representable: the result
does not depend on the summation order (split-K, slab layout, FMA contraction, MFMA accumulation order) and must equal
the exact integer result in every bit, in float32 and in float64.  The generators below derive the widest integer range
(up to +-100, zero excluded so that every element's contribution is visible) the bound admits for the shape and dtypes
they are given and assert the bound, so a changed shape cannot leave the exact regime silently.  The references are
float64 BLAS / einsum on the integer-valued arrays -- exact under the p = 53 bound, which each reference asserts for
itself -- and return float64 arrays that hold integers.  Host only: NumPy, no device."""
import math

import numpy as np

MANTISSA = {"float32": 24, "float64": 53}
CAP = 100


def bound_ok(L, A, B, p):
    """Every partial sum of L products of integers bounded by A and B is exactly representable with p mantissa bits."""
    return int(L) * int(A) * int(B) <= 2 ** int(p)


def _name(dt):
    s = str(dt)
    return s[len("torch."):] if s.startswith("torch.") else np.dtype(dt).name


def mantissa(*dtypes):
    """p of a chain through `dtypes` (NumPy or torch dtypes, or their names)."""
    return min(MANTISSA[_name(d)] for d in dtypes)


def int_range(L, dtypes, group_a=1, group_b=1, cap=CAP):
    """Largest r <= cap with L * (group_a r) * (group_b r) <= 2**p: operands drawn from [-r, r] keep a reduction of
    length L exact.  group_a / group_b: the factor by which an operand's magnitude can grow before the product -- the
    members of a constraint group summed, 2 for a difference of two elements or a scale of 2, 2**k for a division by
    powers of two up to 2**k (scale everything by 2**k: integers again)."""
    p = mantissa(*dtypes)
    r = min(int(cap), math.isqrt(2 ** p // (int(L) * int(group_a) * int(group_b))))
    assert r >= 2, f"no integer range beyond 0/+-1 keeps L={L}, groups {group_a}x{group_b} exact with p={p}"
    assert bound_ok(L, group_a * r, group_b * r, p) and not (r < cap and bound_ok(L, group_a * (r + 1), group_b * (r + 1), p))
    return r


def integers(rng, shape, r):
    """float64 array of integers uniform on [-r, r] without zero."""
    r = int(r)
    assert 1 <= r <= 16000
    v = rng.integers(-r, r, size=shape, dtype=np.int16)  # -r .. r - 1; the non-negative half moves up by one
    v += v >= 0
    return v.astype(np.float64)


def gram_frames(T, N, dtypes, group=1, seed=0):
    """(T, N, 3) frames for a Gram matrix over 3T rows whose reduced columns sum at most `group` atoms."""
    r = int_range(3 * T, dtypes, group, group)
    return integers(np.random.default_rng(seed), (T, N, 3), r)


def operand_pair(L, shape_a, shape_b, dtypes, group_a=1, group_b=1, seed=0, cap=CAP):
    """Two integer arrays for a contraction of length L of one with the other."""
    r = int_range(L, dtypes, group_a, group_b, cap)
    rng = np.random.default_rng(seed)
    return integers(rng, shape_a, r), integers(rng, shape_b, r)


def powers_of_two(rng, shape, zeros=0.0, kmax=3):
    """float64 array of 2**k, k in 0..kmax, a fraction `zeros` of them 0: exact divisors."""
    v = 2.0 ** rng.integers(0, kmax + 1, size=shape)
    return np.where(rng.random(shape) < zeros, 0.0, v)


def _exact(L, a, b):
    """The float64 reference itself is exact: assert the p = 53 bound for the operands as they are."""
    A, B = int(np.max(np.abs(a), initial=0)), int(np.max(np.abs(b), initial=0))
    assert bound_ok(L, max(A, 1), max(B, 1), 53), (L, A, B)


def _integral(x):
    assert np.array_equal(x, np.rint(x))
    return x


# ------------------------------------------------------------------ references (float64 holding integers)
def reduce_columns(f, goa, n_red):
    """(3T, n_red): rows (frame, xyz) of f (T, N, 3), columns summed over constraint groups (goa: column of atom)."""
    T, N, _ = f.shape
    F2 = np.ascontiguousarray(np.transpose(f, (0, 2, 1))).reshape(3 * T, N)
    if goa is None:
        return F2
    C = np.zeros((N, n_red))
    C[np.arange(N), np.asarray(goa)] = 1.0
    return F2 @ C


def gram_ref(f, goa=None, n_red=None):
    R = reduce_columns(np.asarray(f, np.float64), goa, n_red)
    _exact(R.shape[0], R, R)
    return _integral(R.T @ R)


def gram_pair_ref(a, b):
    return gram_ref(np.concatenate([a, b], axis=1))


def apply_ref(points, matrix):
    """out[t,c,d] = sum_n matrix[c,n] points[t,n,d]"""
    _exact(points.shape[1], points, matrix)
    return _integral(np.einsum("cn,tnd->tcd", np.asarray(matrix, np.float64), np.asarray(points, np.float64), optimize=True))


def frames_ref(points, factor, trans=None):
    """out[t,c,d] = sum_f factor[t,c,f] points[t,f,d] (+ trans)"""
    _exact(points.shape[1], points, factor)
    out = np.matmul(np.asarray(factor, np.float64), np.asarray(points, np.float64))
    return _integral(out if trans is None else out + trans)


def cross_ref(a, b):
    """out[i,j] = sum_{t,d} a[t,i,d] b[t,j,d]"""
    T = a.shape[0]
    _exact(3 * T, a, b)
    A2 = np.transpose(a, (0, 2, 1)).reshape(3 * T, -1)
    B2 = np.transpose(b, (0, 2, 1)).reshape(3 * T, -1)
    return _integral(A2.T @ B2)


def frames_t_ref(g, f):
    """out[t,a,d] = sum_c f[t,c,a] g[t,c,d]"""
    _exact(f.shape[1], f, g)
    return _integral(np.matmul(np.transpose(f, (0, 2, 1)), g))


def frames_outer_ref(g, p):
    """out[t,c,a] = sum_d g[t,c,d] p[t,a,d]"""
    _exact(3, g, p)
    return _integral(np.matmul(g, np.transpose(p, (0, 2, 1))))


def group_sum_ref(x, grp_ptr, grp_atoms):
    """(T, n_groups, 3) sums of x (T, N, 3) over CSR groups"""
    n = len(grp_ptr) - 1
    out = np.zeros((x.shape[0], n, 3))
    for g in range(n):
        out[:, g] = x[:, grp_atoms[grp_ptr[g]:grp_ptr[g + 1]]].sum(axis=1)
    return _integral(out)


def pair_disp(x, c):
    """u[t,i,j] = x[t,j] - c[t,i]"""
    return x[:, None, :, :] - c[:, :, None, :]


def pair_pull_ref(w, u):
    """A[t,j] = sum_i w_ij u_ij, B[t,i] = -sum_j w_ij u_ij for u (T, m, n, 3)"""
    q = w[..., None] * u
    return q.sum(axis=1), -q.sum(axis=2)


def list_pull_ref(w, u, pairs, m, n):
    """The same sums over a pair list: u (T, P, 3), pairs (P, 2) rows (i, j)"""
    T = u.shape[0]
    q = w[..., None] * u
    A, B = np.zeros((T, n, 3)), np.zeros((T, m, 3))
    for t in range(T):
        np.add.at(A[t], pairs[:, 1], q[t])
        np.add.at(B[t], pairs[:, 0], -q[t])
    return A, B


# ------------------------------------------------------------------ perturbations
def perturbations(shape, group_member=None):
    """Single-element +-1 changes at the places kernels forget, as (name, index) for an array of `shape` = (frames,
    atoms or rows, ..., fastest axis): the first and the last frame, the last atom, the last component of the fastest
    axis (xyz), the two elements on either side of a row's end (one of them lies in the 16-byte piece that straddles
    it whenever the rows are not whole pieces), a member of a constraint group (`group_member`: its atom index) and the
    array's last element.  `perturb` applies one of them, moving the element one step TOWARDS zero, so the bound the
    array was generated under still holds."""
    shape = tuple(int(s) for s in shape)
    T, mid = shape[0], tuple(s // 2 for s in shape)
    last = tuple(s - 1 for s in shape)
    out = [("first frame", (0,) + mid[1:]),
           ("last frame", (T - 1,) + tuple(s // 3 for s in shape[1:])),
           ("last atom", (mid[0], last[1]) + mid[2:]),
           ("last component", mid[:-1] + (last[-1],)),
           ("before a row end", (mid[0],) + last[1:]),
           ("after a row end", (min(mid[0] + 1, T - 1),) + (0,) * (len(shape) - 1)),
           ("last element", last)]
    if group_member is not None:
        out.append(("group member", (T // 3, int(group_member)) + mid[2:]))
    seen, uniq = set(), []
    for name, idx in out:
        if idx not in seen:
            seen.add(idx)
            uniq.append((name, idx))
    return uniq


def perturb(arr, index):
    out = np.array(arr, dtype=np.float64, copy=True)
    assert out[index] != 0
    out[index] -= np.sign(out[index])
    return out
