"""GPU: every kernel runs on the caller's stream and no wrapper waits for it (tests/stream_gate.py has the method).

CASES lists, per kernel family, a builder of true inputs at the smallest shape that reaches the family (shapes from
tests/test_gpu_layouts.py, tests/test_gpu_dispatch_classes.py and the family's own test file), the call, the C entries
the call drives and the kernels it must launch.  Each group of cases runs behind one gate on a non-default stream
with its floating-point inputs poisoned until a copy behind the gate fills them.  The last test compares the kernel
families launched behind a gate with the library's own inventory; tests/test_streams_host.py compares the entries with
aggforce_amd/_lib.py:PROTOTYPES on a machine without a GPU (this module imports without one: builders run lazily)."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_gate as SG  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402

F32, F64 = torch.float32, torch.float64
KBT = 0.6955215


class Case:
    def __init__(self, name, group, entries, families, build, synchronises=None, env=None, cleanup=None):
        self.name, self.group, self.entries, self.families = name, group, tuple(entries), tuple(families)
        self.build, self.synchronises, self.env, self.cleanup = build, synchronises, env, cleanup


class Flags:
    """Pooled flags (K.take_flag) of the cases that use one: a call returns a CLONE of its flag (a copy on its stream)
    and the flag itself goes back to the pool through K.read_flag -- which synchronises -- once the gated run is over."""
    taken = []

    @classmethod
    def take(cls, device="cuda"):
        flag = K.take_flag(torch.device(device, torch.cuda.current_device()))
        cls.taken.append(flag)
        return flag

    @classmethod
    def keep(cls, flag):
        cls.taken.append(flag)
        return flag

    @classmethod
    def give_back(cls):
        while cls.taken:
            K.read_flag(cls.taken.pop())


def dv(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # (a copy: shared inputs are read-only arrays)
    return (t if dtype is None else t.to(dtype)).cuda()


def rng_of(seed):
    return np.random.default_rng(seed)


def frames(T, N, seed, scale=1.0, dtype=F64):
    return dv(scale * rng_of(seed).standard_normal((T, N, 3)), dtype)


def finite_other(x, seed):
    """An explicit poison: fresh values of x's scale (for inputs whose default poison would not be a valid input)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = float(torch.nan_to_num(x).abs().max()) or 1.0
    return (torch.randn(x.shape, generator=g, dtype=torch.float64) * 0.5 * s).to(x.dtype).cuda()


# ------------------------------------------------------------------ K1
def pair_groups(N):
    from aggforce_amd.constraints import group_layout, groups_csr

    cons = {frozenset([3 * i, 3 * i + 1]) for i in range(N // 3)}
    goa, n_red = group_layout(N, cons)
    p, a = groups_csr(goa, n_red)
    return dv(p), dv(a), n_red


def b_gram(T, N, dtype, cdt, groups=False, first_col=0, accumulate=False):
    def build():
        f = frames(T, N, 100 + N, 3.0, dtype)
        gp = ga = None
        n_red = N
        if groups:
            gp, ga, n_red = pair_groups(N)
        if accumulate:
            base = dv(rng_of(N).standard_normal((n_red, n_red)))
            return [f, base], lambda x, g0: K.gram(x, gp, ga, n_red, cdt, out=g0.clone(), accumulate=True)
        if first_col:
            def call(x):
                part = torch.full((N, N), -7.0, dtype=F64, device="cuda")
                return K.gram(x, None, None, N, cdt, out=part, first_col=first_col)
            return [f], call
        return [f], lambda x: K.gram(x, gp, ga, n_red, cdt)
    return build


def b_gram_pair():
    a, b = frames(64, 128, 1, 1.0), frames(64, 128, 2, 1.0)
    return [a, b], K.gram_pair


def b_augmented_gram():
    rng = rng_of(5)
    n, n2 = 200, 56
    X = rng.standard_normal((n + n2, n + n2))
    C = np.where(rng.random((n2, n)) < 0.03, rng.standard_normal((n2, n)), 0.0)
    cols = K.premap_columns(C, F64, "cuda")  # (the premap's structure and values: built before the gate, as indices are)
    return [dv(X @ X.T)], lambda g: K.augmented_gram(g, n, cols)


def b_sym_group_reduce():
    from aggforce_amd.constraints import group_layout, groups_csr

    n = 256
    X = rng_of(6).standard_normal((n, n))
    goa, n_red = group_layout(n, {frozenset([0, 5]), frozenset([5, 9]), frozenset([20, 21, 22]), frozenset([100, 255])})
    gp, ga = (dv(x) for x in groups_csr(goa, n_red))
    return [dv(X @ X.T)], lambda g: K.sym_group_reduce(g, gp, ga, n_red)


def b_gram_quadform():
    rng = rng_of(2)
    B = rng.normal(size=(130, 130))
    return [dv(B @ B.T), dv(rng.normal(size=(7, 130)))], K.gram_quadform


def b_sym_pack():
    g = rng_of(3).standard_normal((3, 37, 37))
    g = g + np.swapaxes(g, 1, 2)

    def call(x):
        p = K.sym_pack_upper(x)
        return p, K.sym_unpack_upper(p, torch.empty_like(x))
    return [dv(g)], call


# ------------------------------------------------------------------ K2
def qp_problem(n, m, nrhs, seed, p=None):
    rng = rng_of(seed)
    shape = () if p is None else (p,)
    R = rng.standard_normal(shape + (3 * n + 5, n))
    G = np.swapaxes(R, -1, -2) @ R
    A = rng.standard_normal(shape + (m, n))
    B = A @ rng.standard_normal(shape + (n, nrhs))
    G = dv(G)
    # the poison of G is positive definite too
    return (G, 1.5 * G + torch.eye(n, dtype=F64, device="cuda")), dv(A), dv(B)


def b_solve(n, m, nrhs, schur_reg, n_refine):
    def build():
        G, A, B = qp_problem(n, m, nrhs, n + m)
        return [G, A, B], lambda g, a, b: K.eq_qp_solve(g, 1e-3, None, a, b, schur_reg=schur_reg, n_refine=n_refine)
    return build


def b_solve_pinned():
    G, _, _ = qp_problem(200, 3, 1, 7)
    pins = torch.arange(0, 200, 16, dtype=torch.int32)[:12].cuda()
    return [G], lambda g: K.eq_qp_solve_pinned(g, 1e-3, None, pins)


def b_solve_batched(shift):
    def build():
        p, n, m = 3, 70, 9
        G, A, B = qp_problem(n, m, 1, 11, p=p)
        if not shift:
            return [G, A, B], lambda g, a, b: K.eq_qp_solve_batched(g, 0.5, None, a, b)
        perm = torch.arange(n, dtype=torch.int32).repeat(p, 1).contiguous().cuda()

        def call(g, a, b):
            ata = (a.transpose(1, 2) @ a).contiguous()  # (torch, on the current stream)
            return K.eq_qp_solve_batched(g, 0.5, None, a, b, AtA=ata, perm=perm)
        return [G, A, B], call
    return build


def b_expand_map():
    X = dv(rng_of(4).standard_normal((5, 9)))
    goa = dv(rng_of(5).integers(0, 9, size=40).astype(np.int32))
    return [X], lambda x: K.expand_map(x, goa, 40)


# ------------------------------------------------------------------ K3
def b_apply(n_cg, N, T, replace=False):
    def build():
        rng = rng_of(n_cg + N)
        pts = 50 * rng.standard_normal((T, N, 3))
        mat = dv(rng.standard_normal((n_cg, N)))
        if not replace:
            return [dv(pts), mat], lambda p, m: K.linearmap_apply(p, m)
        clean = dv(pts)
        pts[rng.integers(0, T, 7), rng.integers(0, N, 7), rng.integers(0, 3, 7)] = np.nan
        pts[T - 1, N - 1, 2] = np.nan

        def call(p, m):
            probe = Flags.take()
            out, ss = K.linearmap_apply(p, m, nan_fill=-1.0, want_sumsq=True, nan_probe=probe)
            return out, ss, probe.clone()
        # the poison holds no NaN: the flag differs too
        return [(dv(pts), 0.7 * clean.roll(1, 0)), mat], call
    return build


def b_slice_gather():
    pts = frames(301, 175, 3, 20.0, F32)
    idx = dv(np.array([0, 1, 17, 98, 173, 174], dtype=np.int32))

    def call(p):
        probe = Flags.take()
        return K.slice_gather(p, idx, F64, nan_probe=probe), probe.clone()
    return [pts], call


# ------------------------------------------------------------------ K3c / K8 / K4b contractions
def contraction_inputs():
    rng = rng_of(21)
    T, N, n_cg = 137, 45, 13
    return (frames(T, N, 1), dv(rng.standard_normal((T, n_cg, N))), dv(rng.standard_normal((T, n_cg, 3))),
            dv(rng.standard_normal((T, n_cg, 3))))


def b_trjdot_frames(trans):
    def build():
        p, fac, tr, _ = contraction_inputs()
        return ([p, fac, tr], K.trjdot_frames) if trans else ([p, fac], K.trjdot_frames)
    return build


def b_trjdot_cross(accumulate):
    def build():
        p, _, _, g = contraction_inputs()
        if not accumulate:
            return [p, g], lambda a, b: K.trjdot_cross(a, b, F64)
        base = dv(rng_of(22).standard_normal((45, 13)))
        return [p, g, base], lambda a, b, o: K.trjdot_cross(a, b, F64, out=o.clone(), accumulate=True)
    return build


def b_trjdot_frames_t():
    _, fac, _, g = contraction_inputs()
    return [g, fac], lambda a, b: K.trjdot_frames_t(a, b, F64)


def b_trjdot_frames_outer():
    p, _, _, g = contraction_inputs()
    return [g, p], lambda a, b: K.trjdot_frames_outer(a, b, F64)


def feat_inputs():
    rng = rng_of(6)
    T, N, n_feat = 203, 11, 9
    return (dv(rng.standard_normal((T, N, 3))), dv(rng.standard_normal((T, N, n_feat))),
            dv(rng.standard_normal((T, n_feat, 3))))


def b_feat_contract():
    return list(feat_inputs()), lambda f, x, d: K.feat_contract(f, x, d, 0.6, 16)


def b_feat_constraint_rows():
    _, feat, _ = feat_inputs()
    M = dv(rng_of(7).random((4, 11)))
    idx = np.array([3, 77, 0, 41, 89])
    return [feat, M], lambda x, m: K.feat_constraint_rows(x, idx, m, 3)


def b_feat_weights():
    _, feat, _ = feat_inputs()
    coef = dv(rng_of(8).standard_normal(9))

    def call(x, c):
        w = torch.zeros((203, 4, 11), dtype=F64, device="cuda")
        K.feat_weights(x, c, w, 2)
        return w
    return [feat, coef], call


def gb_rows_inputs():
    rng = rng_of(31)
    n_cg, G, nb, S = 7, 150, 5, 45
    Mg = dv(rng.random((n_cg, G)) * (rng.random((n_cg, G)) < 0.3))
    gauss = dv(rng.random((S, G - 1, nb)))
    keep = dv(np.sort(rng.choice((G - 1) * nb, size=300, replace=False)).astype(np.int32))
    return Mg, gauss, keep, (S, G, G - 1, nb)


def b_gb_constraint_rows():
    Mg, gauss, keep, (S, G, n_ch, nb) = gb_rows_inputs()
    return [Mg, gauss], lambda m, g: K.gb_constraint_rows(m, g, S, G, n_ch, nb, 2, cols=keep)


def b_gb_group_overlap():
    Mg = gb_rows_inputs()[0]
    return [Mg], K.gb_group_overlap


def b_gb_constraint_gram():
    Mg, gauss, keep, (S, G, n_ch, nb) = gb_rows_inputs()
    ld = G + 300 + 37

    def call(m, g):
        out = torch.zeros((ld, ld), dtype=F64, device="cuda")
        return K.gb_constraint_gram(K.gb_group_overlap(m), g, S, G, n_ch, nb, out, cols=keep)
    return [Mg, gauss], call


# ------------------------------------------------------------------ K4
BOX = np.array([4.1, 5.3, 6.7])


def k4_inputs():
    rng = rng_of(9)
    T, G, n_cg, nb = 7, 20, 3, 4
    n_ch = G - 1
    sizes = np.ones(G, dtype=np.float32)
    sizes[[1, 4, G - 2]] = 2.0
    coef = rng.standard_normal((n_cg, G + n_ch * nb)) * (rng.random((n_cg, G + n_ch * nb)) < 0.5)
    from aggforce_amd.qp.gbfeat import gb_centers

    return dict(T=T, G=G, n_cg=n_cg, nb=nb, n_ch=n_ch, sizes=dv(sizes), coef=dv(coef),
                compact=K.gb_compact_coefficients(coef, G, "cuda"),
                cols=dv(np.flatnonzero(rng.random(n_ch * nb) < 0.6).astype(np.int32)),
                centers=dv(gb_centers(6.0, 0.0, nb, 0.5, np.float64)),
                Pg=dv(BOX * rng.random((T, G, 3))), cg=dv(BOX * rng.random((T, n_cg, 3))),
                Fg=dv(20 * rng.standard_normal((T, G, 3))), box=dv(BOX))


def b_k4(which, boxed):
    def build():
        from aggforce_amd.qp.gbfeat import CLIP

        o = k4_inputs()
        G, n_ch, cen, sizes = o["G"], o["n_ch"], o["centers"], o["sizes"]
        floats = [o["Fg"], o["Pg"], o["cg"]] + ([o["box"]] if boxed else [])

        def call(Fg, Pg, cg, box=None):
            if which == "channels":
                return K.gb_channels(Pg, cg, 1, sizes, n_ch, cen, 1.0, CLIP, box=box)
            if which == "regmat":
                R = torch.zeros((o["T"], 128, 3), dtype=F64, device="cuda")
                return K.gb_regmat(Fg, Pg, cg, 1, sizes, G, n_ch, cen, 1.0, CLIP, KBT, R)
            if which == "regmat_cols":
                R = torch.zeros((o["T"], 128, 3), dtype=F64, device="cuda")
                return K.gb_regmat_cols(Fg, Pg, cg, 1, sizes, G, o["cols"], cen, 1.0, CLIP, KBT, R, box=box)
            if which == "apply":
                return K.gb_apply(Fg, Pg, cg, sizes, G, n_ch, cen, 1.0, CLIP, o["coef"], box=box)
            if which == "apply_cols":
                return K.gb_apply_cols(Fg, Pg, cg, sizes, G, cen, 1.0, CLIP, o["compact"], box=box)
            if which == "range":
                return K.gb_distance_range(Pg.float(), cg.float(), n_ch, box=None if box is None else box.float())
            raise KeyError(which)
        return floats, call
    return build


def b_group_reduce():
    gp, ga, n_red = pair_groups(61)
    return [frames(301, 61, 4)], lambda x: K.group_reduce(x, gp, ga, n_red, True, F64)


# ------------------------------------------------------------------ K5
def k5_inputs():
    from oracle import aggforce_oracle as orc

    rng = rng_of(8)
    T, N, n_cg = 517, 12, 3
    M = orc.list_mapping_matrix([[0, 1], [4], [7, 8, 9]], N)
    return (dv(5 * rng.random((T, N, 3))), dv(30 * rng.standard_normal((T, N, 3))), M,
            dv(rng.standard_normal((T, n_cg, 3))), n_cg)


def b_condnormal_augment():
    c, f, M, noise, n_cg = k5_inputs()
    cols = K.premap_columns(M, F64, "cuda")
    Md = dv(M)

    def call(c_, f_, z):
        mean = K.linearmap_apply(c_, Md)
        return K.condnormal_augment(c_, f_, cols, n_cg, mean, 0.05, KBT, z, 1, 0)
    return [c, f, noise], call


def b_condnormal_sites(philox):
    def build():
        _, _, _, noise, n_cg = k5_inputs()
        mean = dv(rng_of(9).standard_normal(tuple(noise.shape)))
        if philox:
            return [mean], lambda m: K.condnormal_sites(m, 0.05, KBT, None, 17, 5, F64)
        return [mean, noise], lambda m, z: K.condnormal_sites(m, 0.05, KBT, z, 1, 0, F64)
    return build


def b_residual_over_var():
    rng = rng_of(3)
    return ([dv(5 * rng.standard_normal((1237, 7, 3))), dv(5 * rng.standard_normal((1237, 7, 3)))],
            lambda g, m: K.residual_over_var(g, m, 0.37, F64))


def b_frames_matmul():
    rng = rng_of(10)
    T, Kd, J = 333, 36, 9
    x, sub, b, add = (dv(rng.standard_normal(s)) for s in ((T, Kd), (T, Kd), (J, Kd), (T, J)))
    return [x, b, sub, add], lambda x_, b_, s_, a_: K.frames_matmul(x_, b_, s_, a_, 0.5)


def b_augment_concat():
    rng = rng_of(4)
    T, N, n = 333, 9, 4
    arrs = [dv(rng.standard_normal(s)) for s in ((T, N, 3), (T, N, 3), (T, n, 3), (T, N, 3), (T, n, 3))]
    return arrs, lambda x, F, y, corr, lg: K.augment_concat(x, F, y, corr, lg, 0.7)


def b_synth_normal():
    # The generator has NO input, so the poison cannot see where its kernel ran: a misrouted synth_normal_kernel writes
    # the same values early.  For this kernel only the other half of the contract is checked -- the call returns at
    # once, and its output is complete when work ordered behind it on the stream (the axpby with a poisoned operand,
    # which gives the case its input) reads it.
    y = frames(257, 33, 12)
    return [y], lambda y_: K.axpby(1.0, K.synth_normal(257, 33, F64, 9, sigma=30.0, lattice=1.5), 2.0, y_)


# ------------------------------------------------------------------ K6
def b_pair_var(moments, boxed):
    def build():
        import guess_box_data as D

        x, L = D.wrapped(False, "float64")
        floats = [dv(x)] + ([dv(L)] if boxed else [])
        fn = K.pair_dist_moments if moments else K.pair_dist_var
        return floats, (lambda x_, b=None: fn(x_, box=b))
    return build


def b_pair_pool_term():
    rng = rng_of(13)
    v, mr, m = (dv(rng.random((31, 31))) for _ in range(3))
    return [v, mr, m], lambda v_, mr_, m_: K.pair_pool_term(v_.clone(), mr_, m_, 0.3)


# ------------------------------------------------------------------ K7
def k7_inputs():
    rng = rng_of(31)
    return dv(10.0 * rng.random((53, 67, 3))), dv(rng.standard_normal((53, 67, 3))), dv(np.array([45.0, 60.0, 80.0]))


def b_gauss_pair_forces():
    x, _, _ = k7_inputs()
    return [x], lambda x_: K.gauss_pair_forces(x_, 45.0, 30.0, want_forces=True, want_energies=True)


def b_gauss(which):
    def build():
        x, f, offs = k7_inputs()
        fn = K.gauss_proj if which == "proj" else K.gauss_shift
        return [x, f, offs], lambda x_, f_, o_: fn(x_, f_, o_, 30.0)
    return build


def b_dot():
    x, f, _ = k7_inputs()
    return [x, f], K.dot


# ------------------------------------------------------------------ K9 / K10 / K11
def b_pair_dist(mode):
    def build():
        from pairlist_ref import lattice_sites

        x, c = dv(lattice_sites(7, 70, 51)), dv(lattice_sites(7, 13, 52) + 0.4)
        if mode == K.PAIR_DOT:
            v, y = frames(7, 70, 53), frames(7, 13, 54)
            return [x, c, v, y], lambda x_, c_, v_, y_: K.pair_dist(x_, c_, K.PAIR_DOT, v_, y_)
        return [x, c], lambda x_, c_: K.pair_dist(x_, c_, mode)
    return build


def b_pair_pull():
    from pairlist_ref import lattice_sites

    T, m, n = 5, 7, 300  # more than one 128-column panel: the float64 partials and their reduction
    x, c = dv(lattice_sites(T, n, 55)), dv(lattice_sites(T, m, 56) + 0.4)
    w = dv(rng_of(57).standard_normal((T, m, n)))
    return [w, x, c], lambda w_, x_, c_: K.pair_pull(w_, x_, c_)


def b_pair_list(pull, boxed):
    def build():
        from aggforce_amd.jaxutil import PairList
        from pairlist_ref import lattice_sites, random_list

        T, m, n, P = 9, 6, 11, 70
        tab = PairList(random_list(P, m, n, 300, self_form=False), n, m).on("cuda")
        x, c = dv(lattice_sites(T, n, 58)), dv(lattice_sites(T, m, 59) + 0.4)
        floats = [x, c] + ([dv(rng_of(60).standard_normal((T, P)))] if pull else []) + ([dv(BOX)] if boxed else [])

        def call(x_, c_, *rest):
            rest = list(rest)
            box = rest.pop() if boxed else None
            if pull:
                return K.pair_list_pull(rest[0], x_, c_, tab, box=box)
            return K.pair_list_dist(x_, c_, tab, box=box)
        return floats, call
    return build


def b_pair_min(T, m, n, boxed):
    def build():
        from pairlist_ref import lattice_sites

        x, c = dv(lattice_sites(T, n, 51)), dv(lattice_sites(T, m, 52) + 0.4)
        floats = [x, c] + ([dv(BOX)] if boxed else [])
        return floats, lambda x_, c_, b=None: K.pair_min(x_, c_, box=b)
    return build


def b_gbasis(which):
    def build():
        rng = rng_of(70)
        shape, nb, n_slots = (3, 5, 67), 10, 4
        d = dv(0.5 + 7.0 * rng.random(shape))
        s = dv(rng.standard_normal(shape))
        cen = dv(np.linspace(0.5, 8.0, nb))
        channels = [(-1 if i % 5 == 0 else (i % n_slots if i % n_slots != 1 else 2)) for i in range(shape[-1])]
        spec = K.BasisSpec(cen, 1.3, 1e-3, channels, n_slots)
        if which == "expand":
            return [d, s], lambda d_, s_: K.gbasis_expand(d_, spec, 1, s_)
        if which == "contract":
            h = dv(rng.standard_normal(shape + (n_slots * nb,)))
            return [h, d], lambda h_, d_: K.gbasis_contract(h_, d_, spec, 1, K.GB_H_ROW)
        return [d, s], lambda d_, s_: K.gbasis_sum(d_, spec, 0, s_)
    return build


def b_make_whole(form):
    def build():
        import whole_ref as R
        from aggforce_amd import MoleculeTree

        w, _, box, par = R.molecules("random", 131, 9, "float64", False)
        tab = MoleculeTree(par).on("cuda")

        def call(x, b):
            images = torch.zeros(tuple(x.shape), dtype=torch.int32, device="cuda")
            return K.make_whole(x, b, tab, images=images, _form=form), images
        return [dv(np.array(w)), dv(np.array(box))], call
    return build


# ------------------------------------------------------------------ small kernels
def b_nan_flag():
    x = frames(211, 37, 41)
    x.view(-1)[1234] = float("nan")

    def call(x_):
        return Flags.keep(K.nan_flag(x_)).clone()  # (the pooled flag is handed back after the gated run)
    return [(x, finite_other(x, 1))], call


def b_small(which):
    def build():
        a, b = frames(211, 37, 41, 3.0), frames(211, 5, 42, 3.0)
        if which == "sumsq":
            return [a], K.sumsq
        if which == "axpby":
            return [a, a.flip(0).contiguous()], lambda x, y: K.axpby(2.0, x, -0.5, y)
        if which == "scale":
            return [a], lambda x: K.scale(x, -2.5)
        if which == "take_frames":
            idx = np.array([0, 210, 5, 5, 100, 209])
            return [a], lambda x: K.take_frames(x, idx)
        if which == "concat_sites":
            return [a, b], K.concat_sites
        raise KeyError(which)
    return build


def b_host_value(which):
    def build():
        a = frames(211, 37, 41, 3.0)
        if which == "has_nan":
            bad = a.clone()
            bad.view(-1)[77] = float("nan")
            return [(bad, finite_other(a, 2))], lambda x: torch.as_tensor([K.has_nan(x)])
        if which == "read_flag":
            bad = a.clone()
            bad.view(-1)[78] = float("nan")
            return [(bad, finite_other(a, 4))], lambda x: torch.as_tensor([K.read_flag(K.nan_flag(x))])
        if which == "allclose":
            return [a, (a.clone(), finite_other(a, 3))], lambda x, y: torch.as_tensor([K.allclose(x, y)])
        if which == "take_frames_device_index":
            idx = dv(np.array([0, 210, 5, 5, 100, 209]))
            return [a], lambda x: K.take_frames(x, idx)
        raise KeyError(which)
    return build


SYNCHRONISES = {
    "has_nan": "returns a Python bool: read_flag copies the flag to the host",
    "allclose": "returns a Python bool: read_flag copies the flag to the host",
    "read_flag": "returns a Python bool: the flag is copied to the host (the NaN policy of LinearMap / JLinearMap reads "
                 "one flag per call this way)",
    "take_frames_device_index": "an index tensor on the device is range-checked on the host (one .tolist())",
}

GRAM_OVERLAP = {"AGGF_GRAM_PACK": "overlap", "AGGF_GRAM_PACK_MIN_FRAMES": "256"}

CASES = [
    # K1
    Case("gram_streaming", "k1", ["aggf_gram"], ["gram_small_kernel", "gram_reduce_small_kernel"], b_gram(1201, 61, F64, F64)),
    Case("gram_tile_in_place", "k1", ["aggf_gram"], ["gram_tile_dma_kernel<", "build_tile_table_kernel", "gram_reduce_kernel"],
         b_gram(1201, 601, F64, F64)),
    Case("gram_pack_groups", "k1", ["aggf_gram"], ["pack_groups_kernel", "gram_tile_dma_kernel<"],
         b_gram(515, 800, F32, F64, groups=True)),
    Case("gram_first_col", "k1", ["aggf_gram_from_column"], ["gram_tile_dma_kernel<"], b_gram(1001, 601, F64, F64, first_col=128)),
    Case("gram_accumulate", "k1", ["aggf_gram"], ["gram_small_kernel"], b_gram(1201, 61, F64, F64, accumulate=True)),
    Case("gram_macro_tiles", "k1", ["aggf_gram"], ["gram_tile_dma_kernel_x2", "build_macro_table_kernel"],
         b_gram(333, 1152, F64, F64)),
    Case("gram_overlapped_pack", "k1_overlap", ["aggf_gram"], ["pack_groups_kernel<float, double, true>", "gram_tile_dma_kernel<"],
         b_gram(2051, 800, F32, F64, groups=True), env=GRAM_OVERLAP),
    Case("gram_pair", "k1b", ["aggf_gram_pair"], ["gram_"], b_gram_pair),
    Case("augmented_gram", "k1b", ["aggf_augmented_gram"], ["auggram_h_kernel", "auggram_kernel"], b_augmented_gram),
    Case("sym_group_reduce", "k1b", ["aggf_sym_group_reduce"], ["sym_group_reduce_kernel"], b_sym_group_reduce),
    Case("gram_quadform", "k1b", ["aggf_gram_quadform"], ["rowdot_kernel"], b_gram_quadform),
    Case("sym_pack_unpack", "k1b", ["aggf_sym_pack_upper", "aggf_sym_unpack_upper"], ["sym_pack_kernel", "sym_unpack_kernel"],
         b_sym_pack),
    # K2
    Case("eq_qp_solve", "k2", ["aggf_eq_qp_solve"], ["chol_step_kernel", "crop_transpose_kernel"], b_solve(200, 17, 17, 1e-12, 3)),
    Case("eq_qp_solve_three_launch_steps", "k2", ["aggf_eq_qp_solve"], ["potrf_diag_mfma_kernel", "gemm_tile_kernel"],
         b_solve(640, 5, 2, 0.0, 1), env={"AGGF_SOLVE_WGS": "1"}),
    Case("eq_qp_solve_pinned", "k2", ["aggf_eq_qp_solve_pinned"], ["pinned_build_kernel", "pinned_scatter_kernel"], b_solve_pinned),
    Case("eq_qp_solve_batched", "k2", ["aggf_eq_qp_solve_batched"], ["chol_step_kernel"], b_solve_batched(False)),
    Case("eq_qp_solve_batched_shift", "k2", ["aggf_eq_qp_solve_batched_shift"], ["chol_step_kernel"], b_solve_batched(True)),
    Case("expand_map", "k2", ["aggf_expand_map"], ["expand_map_kernel"], b_expand_map),
    # K3
    Case("apply_tile", "k3", ["aggf_linearmap_apply"], ["aggf::apply_kernel<"], b_apply(20, 24, 333)),
    Case("apply_small", "k3", ["aggf_linearmap_apply"], ["apply_small_kernel"], b_apply(10, 175, 1003)),
    Case("apply_dma", "k3", ["aggf_linearmap_apply"], ["apply_dma_kernel"], b_apply(40, 200, 257)),
    Case("apply_nan_replace", "k3", ["aggf_linearmap_apply"], ["aggf::apply_kernel<", "sum_partials_kernel"],
         b_apply(20, 77, 333, replace=True), cleanup=Flags.give_back),
    Case("slice_gather", "k3", ["aggf_slice_gather"], ["slice_gather_kernel"], b_slice_gather, cleanup=Flags.give_back),
    # K3c / K8 / K4b
    Case("trjdot_frames", "k8", ["aggf_trjdot_frames"], ["trjdot_frames_kernel"], b_trjdot_frames(False)),
    Case("trjdot_frames_trans", "k8", ["aggf_trjdot_frames"], ["trjdot_frames_kernel"], b_trjdot_frames(True)),
    Case("trjdot_cross", "k8", ["aggf_trjdot_cross"], ["trjdot_cross_kernel", "trjdot_cross_reduce"], b_trjdot_cross(False)),
    Case("trjdot_cross_accumulate", "k8", ["aggf_trjdot_cross"], ["trjdot_cross_kernel"], b_trjdot_cross(True)),
    Case("trjdot_frames_t", "k8", ["aggf_trjdot_frames_t"], ["trjdot_frames_t_kernel"], b_trjdot_frames_t),
    Case("trjdot_frames_outer", "k8", ["aggf_trjdot_frames_outer"], ["trjdot_frames_outer_kernel"], b_trjdot_frames_outer),
    Case("feat_contract", "k8", ["aggf_feat_contract"], ["feat_contract_kernel"], b_feat_contract),
    Case("feat_constraint_rows", "k8", ["aggf_feat_constraint_rows"], ["feat_rows_kernel"], b_feat_constraint_rows),
    Case("feat_weights", "k8", ["aggf_feat_weights"], ["feat_weights_kernel"], b_feat_weights),
    Case("gb_constraint_rows", "k8", ["aggf_gb_constraint_rows"], ["gb_rows_kernel"], b_gb_constraint_rows),
    Case("gb_group_overlap", "k8", ["aggf_gb_group_overlap"], ["gb_overlap_kernel"], b_gb_group_overlap),
    Case("gb_constraint_gram", "k8", ["aggf_gb_constraint_gram"], ["gb_ata_kernel"], b_gb_constraint_gram),
    # K4
    Case("group_reduce", "k4", ["aggf_group_reduce"], ["group_reduce_kernel"], b_group_reduce),
    Case("gb_regmat", "k4", ["aggf_gb_regmat"], ["gb_regmat_kernel"], b_k4("regmat", False)),
    Case("gb_channels", "k4", ["aggf_gb_channels"], ["gb_channels_kernel"], b_k4("channels", False)),
    Case("gb_channels_box", "k4", ["aggf_gb_channels_pbc"], ["gb_channels_pbc_kernel"], b_k4("channels", True)),
    Case("gb_regmat_cols", "k4", ["aggf_gb_regmat_cols"], ["gb_regmat_cols_kernel"], b_k4("regmat_cols", False)),
    Case("gb_regmat_cols_box", "k4", ["aggf_gb_regmat_cols_pbc"], ["gb_regmat_cols_pbc_kernel"], b_k4("regmat_cols", True)),
    Case("gb_apply", "k4", ["aggf_gb_apply"], ["gb_apply_kernel"], b_k4("apply", False)),
    Case("gb_apply_box", "k4", ["aggf_gb_apply_pbc"], ["gb_apply_pbc_kernel"], b_k4("apply", True)),
    Case("gb_apply_cols", "k4", ["aggf_gb_apply_cols"], ["gb_apply_cols_kernel"], b_k4("apply_cols", False)),
    Case("gb_apply_cols_box", "k4", ["aggf_gb_apply_cols_pbc"], ["gb_apply_cols_pbc_kernel"], b_k4("apply_cols", True)),
    Case("gb_distance_range", "k4", ["aggf_gb_distance_range"], ["gb_range_kernel"], b_k4("range", False)),
    Case("gb_distance_range_box", "k4", ["aggf_gb_distance_range_pbc"], ["gb_range_pbc_kernel"], b_k4("range", True)),
    # K5
    Case("condnormal_augment", "k5", ["aggf_condnormal_augment"], ["augment_kernel"], b_condnormal_augment),
    Case("condnormal_sites", "k5", ["aggf_condnormal_sites"], ["noise_sites_kernel"], b_condnormal_sites(False)),
    Case("condnormal_sites_philox", "k5", ["aggf_condnormal_sites"], ["noise_sites_kernel"], b_condnormal_sites(True)),
    Case("residual_over_var", "k5", ["aggf_residual_over_var"], ["residual_over_var_kernel"], b_residual_over_var),
    Case("frames_matmul", "k5", ["aggf_frames_matmul"], ["frames_matmul_kernel"], b_frames_matmul),
    Case("augment_concat", "k5", ["aggf_augment_concat"], ["augment_concat_kernel"], b_augment_concat),
    Case("synth_normal", "k5", ["aggf_synth_normal"], ["synth_normal_kernel"], b_synth_normal),
    # K6
    Case("pair_dist_var", "k6", ["aggf_pair_dist_var"], ["pair_stats_kernel", "pair_var_kernel"], b_pair_var(False, False)),
    Case("pair_dist_var_box", "k6", ["aggf_pair_dist_var_pbc"], ["pair_stats_pbc_kernel", "pair_var_pbc_kernel"],
         b_pair_var(False, True)),
    Case("pair_dist_moments", "k6", ["aggf_pair_dist_moments"], ["pair_stats_kernel"], b_pair_var(True, False)),
    Case("pair_dist_moments_box", "k6", ["aggf_pair_dist_moments_pbc"], ["pair_stats_pbc_kernel"], b_pair_var(True, True)),
    Case("pair_pool_term", "k6", ["aggf_pair_pool_term"], ["pair_pool_kernel"], b_pair_pool_term),
    # K7
    Case("gauss_pair_forces", "k7", ["aggf_gauss_pair_forces"], ["gauss_site_forces_kernel", "gauss_energy_finish_kernel"],
         b_gauss_pair_forces),
    Case("gauss_proj", "k7", ["aggf_gauss_proj"], ["gauss_proj_kernel", "mapval_slab_reduce_kernel"], b_gauss("proj")),
    Case("gauss_shift", "k7", ["aggf_gauss_shift"], ["gauss_shift_kernel"], b_gauss("shift")),
    Case("dot", "k7", ["aggf_dot"], ["dot_kernel", "dot_finish_kernel"], b_dot),
    # K9 / K10 / K11
    Case("pair_dist", "k9", ["aggf_pair_dist"], ["pairdist_kernel"], b_pair_dist(0)),
    Case("pair_dist_dot", "k9", ["aggf_pair_dist"], ["pairdist_kernel"], b_pair_dist(2)),
    Case("pair_pull", "k9", ["aggf_pair_pull"], ["pairpull_kernel", "pairpull_reduce_kernel"], b_pair_pull),
    Case("pair_list_dist", "k9", ["aggf_pair_list_dist"], ["pairlist_kernel"], b_pair_list(False, False)),
    Case("pair_list_dist_box", "k9", ["aggf_pair_list_dist_pbc"], ["pairlist_pbc_kernel"], b_pair_list(False, True)),
    Case("pair_list_pull", "k9", ["aggf_pair_list_pull"], ["pairlist_pull_kernel"], b_pair_list(True, False)),
    Case("pair_list_pull_box", "k9", ["aggf_pair_list_pull_pbc"], ["pairlist_pull_pbc_kernel"], b_pair_list(True, True)),
    Case("pair_min_one_split", "k9", ["aggf_pair_min"], ["pairmin_kernel"], b_pair_min(5, 3, 7, False)),
    Case("pair_min_several_splits", "k9", ["aggf_pair_min"], ["pairmin_kernel", "pairmin_reduce_kernel"],
         b_pair_min(67, 70, 257, True)),
    Case("gbasis_expand", "k10", ["aggf_gbasis_expand"], ["gb_expand_kernel"], b_gbasis("expand")),
    Case("gbasis_contract", "k10", ["aggf_gbasis_contract"], ["gb_contract_kernel"], b_gbasis("contract")),
    Case("gbasis_sum", "k10", ["aggf_gbasis_sum"], ["gb_chansum_kernel", "gb_chansum_reduce_kernel"], b_gbasis("sum")),
    Case("make_whole_lds", "k10", ["aggf_make_whole"], ["whole_lds_kernel"], b_make_whole(1)),
    Case("make_whole_global", "k10", ["aggf_make_whole"], ["whole_edge_kernel", "whole_jump_kernel", "whole_shift_kernel"],
         b_make_whole(2)),
    # small kernels
    Case("nan_flag", "small", ["aggf_has_nan"], ["has_nan_kernel"], b_nan_flag, cleanup=Flags.give_back),
    Case("sumsq", "small", ["aggf_sumsq"], ["sumsq_kernel", "sum_fixed_kernel"], b_small("sumsq")),
    Case("axpby", "small", ["aggf_daxpby"], ["axpby_kernel"], b_small("axpby")),
    Case("scale", "small", ["aggf_scale"], ["scale_kernel"], b_small("scale")),
    Case("take_frames", "small", ["aggf_take_frames"], ["take_frames_kernel"], b_small("take_frames")),
    Case("concat_sites", "small", ["aggf_concat_sites"], ["concat_sites_kernel"], b_small("concat_sites")),
    # wrappers that return a host value: one gate each
    Case("has_nan", "sync_has_nan", ["aggf_has_nan"], ["has_nan_kernel"], b_host_value("has_nan"),
         synchronises=SYNCHRONISES["has_nan"]),
    Case("read_flag", "sync_read_flag", ["aggf_has_nan"], ["has_nan_kernel"], b_host_value("read_flag"),
         synchronises=SYNCHRONISES["read_flag"]),
    Case("allclose", "sync_allclose", ["aggf_not_close"], ["not_close_kernel"], b_host_value("allclose"),
         synchronises=SYNCHRONISES["allclose"]),
    Case("take_frames_device_index", "sync_take_frames", ["aggf_take_frames"], ["take_frames_kernel"],
         b_host_value("take_frames_device_index"), synchronises=SYNCHRONISES["take_frames_device_index"]),
]

# kernel families no gated case launches, and C entries with a stream that no case names, with the reason
EXEMPT = {
    "aggf_allreduce_sum": "the RCCL path of aggf_comm.hip needs two ranks (tests/test_gpu_comm.py runs it in child "
                          "processes); it launches no kernel of the library",
}
MAX_EXEMPT = 5

GROUPS = sorted({c.group for c in CASES}, key=[c.group for c in CASES].index)


# ------------------------------------------------------------------ 1. the canary
DEFAULT_STREAM_SERIALISES = (
    "observed on the MI355X: late in a long session a launch on the default (null) stream was held back behind the gated "
    "non-blocking stream (the gate held, the null stream's synchronise returned, yet the kernel ran after the copy and "
    "read true data); alone and early in a session the same launch reads the poison.  The null stream is no reliable "
    "'wrong stream' on this runtime: the second-stream canary is the one that must see the poison")


@pytest.mark.parametrize("wrong_name", ["second_stream",
                                        pytest.param("default_stream", marks=pytest.mark.xfail(
                                            strict=False, reason=DEFAULT_STREAM_SERIALISES))])
def test_canary_a_call_on_the_wrong_stream_reads_the_poison(wrong_name):
    """The method sees a misrouted launch: inputs filled behind the gate on `s`, the call made on another stream -- a
    second torch stream; the default stream -- gives a result that differs from the reference.  This is the only race
    of the module: the misrouted kernel reads valid memory that `s` overwrites later."""
    s = SG.stream()
    SG.calibrate()
    wrong = SG.other_stream() if wrong_name == "second_stream" else torch.cuda.default_stream()
    x = frames(211, 37, 41, 3.0)
    ref = K.scale(x, -2.5)
    torch.cuda.synchronize()
    with torch.cuda.stream(wrong):  # warm-up on the wrong stream
        K.scale(x, -2.5)
    torch.cuda.synchronize()
    buf = SG.default_poison(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        e0, e1 = SG.gate(0.1, s)
        buf.copy_(x, non_blocking=True)
    with torch.cuda.stream(wrong):
        out = K.scale(buf, -2.5)
        wrong.synchronize()  # the misrouted kernel is done ...
    held = not s.query()     # ... while the gate still holds the copy back
    torch.cuda.synchronize()
    seen = {"gate_held": held, "saw_poison": not torch.equal(SG.bits(out), SG.bits(ref)),
            "gate_s": e0.elapsed_time(e1) * 1e-3}
    SG._state["canary"][wrong_name] = seen
    SG.write_report()
    assert seen["gate_held"] and seen["saw_poison"], seen


# ------------------------------------------------------------------ 2. the wrappers, one gate per group
@pytest.mark.parametrize("group", GROUPS)
def test_every_call_of_the_group_runs_on_the_callers_stream_and_returns_at_once(group, monkeypatch):
    SG.run_behind_gate([c for c in CASES if c.group == group], monkeypatch)


# ------------------------------------------------------------------ 3. paths with internal streams, under a caller's stream
def _on_stream_equals_default(build, name, monkeypatch=None):
    """Host-returning paths: the result with GPU inputs filled behind the gate on `s` equals the default-stream result
    bit for bit (ordering only: these calls return host values, so they wait for the stream by contract)."""
    SG.run_behind_gate(Case(name, name, [], [], build, synchronises="returns host values"), monkeypatch)


def _as_tensors(res, keys=("mapped_coords", "mapped_forces")):
    out = [torch.as_tensor(np.asarray(K.as_device(res[k]).cpu())) for k in keys]
    return out + [torch.as_tensor([float(res["residual"])], dtype=F64)]


def test_linearmap_and_jlinearmap_under_a_callers_stream():
    from aggforce_amd import LinearMap
    from aggforce_amd.map import JLinearMap

    rng = rng_of(51)
    T, N, n_cg = 501, 175, 10
    dense = np.zeros((n_cg, N))
    for i in range(n_cg):
        dense[i, i * 17:(i + 1) * 17] = rng.random(17)
    sel = [[i * 17] for i in range(n_cg)]
    maps = {"linear_dense": LinearMap(dense), "linear_slice": LinearMap(sel, n_fg_sites=N),
            "j_dense": JLinearMap(dense), "j_slice": JLinearMap(LinearMap(sel, n_fg_sites=N).standard_matrix)}
    for name, lm in maps.items():
        _on_stream_equals_default(lambda lm=lm: ([frames(T, N, 52, 20.0)], lambda p: lm(p)), "map_" + name)
    # the pending-map path on K.side_stream
    slice_map = maps["linear_slice"]

    def pending(p):
        h = slice_map.map_async(p)
        assert h is not None
        return h.result()
    _on_stream_equals_default(lambda: ([frames(T, N, 52, 20.0)], pending), "map_async_side_stream")


@pytest.mark.parametrize("n_streams", ["3", "1"])
def test_project_forces_with_the_fused_gb_feat_fit_under_a_callers_stream(n_streams, monkeypatch):
    from aggforce_amd import LinearMap, project_forces
    from aggforce_amd.qp import Multifeaturize, gb_feat, id_feat, qp_feat_linear_map
    from aggforce_amd.util import Curry
    from test_gpu_feat import system

    monkeypatch.setenv("AGGF_FEAT_STREAMS", n_streams)
    coords, forces, cons, cmat = system(T=60, dtype=np.float32)
    cmap = LinearMap(cmat)
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=8.0, inner=0.0, n_basis=4, width=1.0)])
    picks = [rng_of(3 + i).choice(60, size=6, replace=False) for i in range(4)]

    def build():
        def call(c, f):
            return _as_tensors(project_forces(c, f, cmap, constrained_inds=cons, method=qp_feat_linear_map, featurizer=feat,
                                              kbt=KBT, frame_indices=picks, l2_regularization=10.0))
        return [dv(coords), dv(forces)], call
    _on_stream_equals_default(build, f"project_forces_gb_feat_{n_streams}_streams")


def test_project_forces_linear_with_guessed_constraints_under_a_box_and_a_callers_stream():
    import guess_box_data as D
    from aggforce_amd import LinearMap, project_forces

    x, L = D.wrapped(False, "float64")
    cmap = LinearMap([[0], [5], [40], [129]], n_fg_sites=D.N)

    def build():
        f = frames(D.T, D.N, 61, 30.0)
        box = dv(L)
        return [dv(x), f], lambda c, f_: _as_tensors(project_forces(c, f_, cmap, constrained_inds="auto", box=box,
                                                                    l2_regularization=1e-3))
    _on_stream_equals_default(build, "project_forces_linear_auto_box")


def test_noised_fit_under_a_callers_stream():
    from aggforce_amd import LinearMap, Trajectory, joptgauss_map
    from test_gpu_noised_fused import KBT as KBT_N, VAR, case

    coords, forces, cmat, cons, l2, eps, _ = case("slice_f32")
    cmap = LinearMap(cmat)

    def build():
        def call(c, f):
            traj = Trajectory(coords=c, forces=f)
            tm = joptgauss_map(traj, cmap, var=VAR, kbt=KBT_N, constraints=cons, noise=list(eps), l2_regularization=l2)
            mapped = tm(traj)
            return [torch.as_tensor(np.array(tm.tmap.force_map.standard_matrix)), K.as_device(mapped.forces).cpu(),
                    K.as_device(mapped.coords).cpu()]
        return [dv(coords), dv(forces)], call
    _on_stream_equals_default(build, "noised_fit_slice_f32")


def test_streamed_project_forces_entered_from_a_callers_stream(tmp_path):
    """Host inputs, so no poison: entered from a non-default current stream the streamed fit equals the in-memory one
    as tests/test_gpu_staged.py::test_streamed_project_forces_matches_in_memory requires."""
    from aggforce_amd import project_forces
    from aggforce_amd.stream import load_trajectory, project_forces_streamed
    from test_gpu_staged import rel, system

    coords, forces, cmap, cons, _ = system(T=1000, seed=21)
    np.save(tmp_path / "run_coords.npy", coords)
    np.save(tmp_path / "run_forces.npy", forces)
    mc, mf = load_trajectory(str(tmp_path / "run"))
    ref = project_forces(coords, forces, cmap, cons, l2_regularization=1e-3, gram_dtype=np.float64)
    s = SG.stream()
    with torch.cuda.stream(s):
        SG.gate(0.05, s)
        out = project_forces_streamed(mc, mf, cmap, cons, l2_regularization=1e-3, chunk_frames=128, gram_dtype=np.float64)
    s.synchronize()
    assert rel(out["tmap"].force_map.standard_matrix, ref["tmap"].force_map.standard_matrix) < 1e-9
    assert rel(out["mapped_forces"], ref["mapped_forces"]) < 1e-9
    assert rel(out["mapped_coords"], ref["mapped_coords"]) < 1e-6
    assert abs(out["residual"] - ref["residual"]) < 1e-9 * ref["residual"]


def test_autograd_forward_and_backward_under_a_callers_stream():
    """jaxutil.distances and jaxutil.trjdot, forward and backward inside the stream context, inputs filled behind the
    gate: values and gradients equal the default-stream ones bit for bit, and nothing waits for the stream."""
    from aggforce_amd import jaxutil
    from pairlist_ref import lattice_sites

    def build():
        x = dv(lattice_sites(7, 40, 71))
        fac = dv(rng_of(72).standard_normal((7, 5, 40)))
        w = dv(rng_of(73).standard_normal((7, 40, 40)))

        def call(x_, fac_, w_):
            xl, fl = x_.detach().clone().requires_grad_(), fac_.detach().clone().requires_grad_()
            d = jaxutil.distances(xl)
            m = jaxutil.trjdot(xl, fl)
            ((d * w_).sum() + (m * m).sum()).backward()
            return d.detach(), m.detach(), xl.grad, fl.grad
        return [x, fac, w], call
    SG.run_behind_gate(Case("autograd_distances_trjdot", "autograd", [], ["pairdist_kernel", "pairpull_kernel"], build))


# ------------------------------------------------------------------ 4. two host threads
def test_two_host_threads_on_their_own_streams():
    """aggf_last_error, the pack pipeline's side stream and the per-device attribute flags are thread_local, the launch
    counters atomics: two Python threads, each on its own stream with its own inputs, run gram -> solve -> apply twenty
    times at once (ctypes releases the GIL inside the calls); every result equals the serial one bit for bit, and a bad
    call in one thread sets that thread's error string only."""
    def inputs(seed):
        f = frames(301, 61, seed, 3.0)
        A = dv(rng_of(seed).standard_normal((4, 61)))
        return f, A

    def chain(f, A):
        G = K.gram(f, None, None, 61, F64)
        X, st = K.eq_qp_solve(G, 1e-3, None, A)
        return G, X, st, K.linearmap_apply(f, X)

    data = [inputs(81), inputs(82)]
    serial = [[SG.bits(t) for t in chain(*d)] for d in data]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results, errors, last = [None, None], [None, None], [None, None]
    start, bad_call_made = threading.Barrier(2), threading.Event()

    def work(i):
        try:
            lib = _lib.load()
            with torch.cuda.stream(streams[i]):
                start.wait(timeout=30)
                outs = []
                for it in range(20):
                    outs.append(chain(*data[i]))
                    if i == 0 and it == 10:  # a bad argument: NULL pointers
                        rc = lib.aggf_has_nan(None, 5, _lib.F64, None, K.stream_ptr())
                        msg = lib.aggf_last_error()
                        bad_call_made.set()
                        assert rc != 0 and msg and b"aggf_has_nan" in msg, (rc, msg)
                streams[i].synchronize()
                results[i] = [[SG.bits(t) for t in o] for o in outs]
                # (the other thread reads its string only AFTER the bad call: a process-wide string would show it)
                assert bad_call_made.wait(timeout=60), "thread 0 never made its bad call"
                msg = lib.aggf_last_error()
                last[i] = msg.decode() if msg else ""
        except BaseException as exc:  # noqa: BLE001 -- reported by the main thread
            errors[i] = exc
            bad_call_made.set()  # (nobody waits for a thread that has failed)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish"
    assert errors == [None, None], errors
    for i in range(2):
        for it, out in enumerate(results[i]):
            assert all(torch.equal(a, b) for a, b in zip(out, serial[i])), (i, it)
    assert "aggf_has_nan" in last[0], last      # not cleared by the successful calls that followed
    assert "aggf_has_nan" not in last[1], last  # the other thread's error string is its own


# ------------------------------------------------------------------ 5. completeness, judged by the library
def test_every_kernel_family_ran_behind_a_gate(request):
    import kernel_inventory as inv

    ran = {it.name.split("[")[0] for it in request.session.items if "test_gpu_streams" in it.nodeid}
    own = {n for n, v in globals().items() if n.startswith("test_") and callable(v)}
    n_groups = sum(1 for it in request.session.items
                   if "test_every_call_of_the_group_runs_on_the_callers_stream" in it.nodeid)
    if request.config.option.keyword or not own <= ran or n_groups != len(GROUPS):
        pytest.skip("completeness is judged on a full run of this module only")
    compiled = inv.compiled_kernels(_lib.LIB_PATH)
    pretty = inv.demangle(sorted(compiled))
    families = {SG.family_of(p) for p in pretty.values()}
    assert len(families) > 90, "kernel inventory looks wrong"
    gated = set(SG.gated_families())
    assert len(EXEMPT) <= MAX_EXEMPT
    missing = sorted(f for f in families - gated if not any(e in f for e in EXEMPT))
    assert not missing, f"{len(missing)} kernel families were launched behind no gate: {missing}"
