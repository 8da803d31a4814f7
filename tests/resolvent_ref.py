"""High-precision restatement of the resolvent sums (helper of test_resolvent_ref_cpu.py / test_gpu_resolvent_edges.py, not
a conftest).

G_k(z) = inv(z I - H(k)), z = omega + i eta, and the rule values the library returns for it: the mean over the nodes of G
(F_GLOC), of tr G (F_TRGLOC) and of -Im tr G / pi (F_DOS).  numpy.linalg.inv in complex128 carries an error of eps cond(A)
itself, so it cannot judge a kernel where conditioning matters; here every inverse is refined in 80-bit long double
(Newton-Schulz, quadratically convergent from LAPACK's start) until its residual is below 1e-15, and the sums are kept in
long double.

What a kernel may lose is measured against the AMPLIFICATION of the case, not against the value: H(k) reaches any
implementation with a relative error of eps (the Fourier sum), and dG = G dH G, so no route can promise better than
eps * sum_k |w_k| ||G_k||_F^2 (||H_k||_F + |z|) on tr G or on an entry of the summed G.  `amplification` is that number
without the eps.
"""
import numpy as np

import abz_oracle as orc

EPS = 2.0 ** -52
KINDS = ("gloc", "trgloc", "dos")

# Largest err(numpy complex128 route) / (EPS * amplification) over every case of edge_cases(), every swept value and the
# three kinds; produced by
#     python -m pytest tests/test_resolvent_ref_cpu.py -k r_lapack -s
# (the test prints the value per case and fails if one exceeds this constant).
R_LAPACK = 1.1  # (1.0636 measured: 1 band, 129 points, eta / rho = 1e-2; rounded up, another LAPACK build may round otherwise)
# the slack of a device route over eps * amplification: 64 is what the suite already grants (1e-11 at eta = 0.02 on
# |H| ~ 1 is about 36 eps / eta^2, rounded up to a power of two); the second term keeps the bound above LAPACK's own error
K_BOUND = max(64.0, 8.0 * R_LAPACK)


def _need_long_double():
    if np.finfo(np.longdouble).eps > 1e-18:
        raise RuntimeError("resolvent_ref needs an 80-bit long double (numpy.longdouble is no wider than float64 here)")


def fourier_nodes(c, first, npt, d):
    """H(k) on the full grid of npt^d nodes, i1 fastest -> [npt^d, n, n] complex128."""
    c = np.asarray(c)
    n = c.shape[-1]
    so = orc.FourierSeries(c, period=1.0, first=first, ndim=d)
    ref = orc.fourier_ptr(so, npt)  # [i1..id, n, n]
    return np.ascontiguousarray(np.transpose(ref, tuple(range(d - 1, -1, -1)) + (d, d + 1)).reshape(-1, n, n))


def refined_inverse(A, tol=1e-15):
    """inv(A) of one matrix or of a stack [..., n, n]: numpy.linalg.inv in complex128, then three Newton-Schulz steps
    X <- X + X (I - A X) in numpy.clongdouble.  Returns (X, max |I - A X|); raises if that exceeds `tol`.

    The relative error of X is the residual (||X - inv(A)|| <= ||X|| res / (1 - res)).  The residual itself is a sum of
    products of size |A| |X| ~ cond(A) rounded to 2^-64, so it cannot fall below about 1e-19 cond(A): 1e-15 is reachable
    up to cond ~ 1e4 and is the default; the cases with a pole at 1e-6 of the spectral radius (cond 2e6, residuals up to
    3e-14 measured) pass a larger `tol` and are covered by Case.ref_err, which the tests hold against their bound."""
    _need_long_double()
    A = np.asarray(A, dtype=np.complex128)
    X = np.linalg.inv(A).astype(np.clongdouble)
    Al = A.astype(np.clongdouble)
    I = np.eye(A.shape[-1], dtype=np.clongdouble)
    for _ in range(3):
        X = X + X @ (I - Al @ X)
    res = float(np.abs(I - Al @ X).max())
    if not res <= tol:
        raise ArithmeticError(f"refined_inverse: residual {res:.2e} > {tol:.0e} after three steps (cond too large for this helper)")
    return X, res


def _of_kind(G, kind):
    """G [..., n, n] (long double) -> the kind's components: G itself, tr G, or -Im tr G / pi."""
    if kind == "gloc":
        return G
    tr = np.trace(G, axis1=-2, axis2=-1)
    if kind == "trgloc":
        return tr
    if kind == "dos":
        return -tr.imag / np.longdouble(np.pi)
    raise ValueError(kind)


def _resolvent_matrix(Hk, z):
    Hk = np.asarray(Hk, dtype=np.complex128)
    return complex(z) * np.eye(Hk.shape[-1]) - Hk


def summed_g(Hk, w, z, tol=1e-15):
    """sum_k w_k G_k(z) / sum_k w_k in long double [n, n], the largest residual `res` of the inverses, and the bound
    res sum_k |w_k| ||G_k||_F / sum_k w_k on the error of any entry of that mean (or of its trace / sqrt(n))."""
    w = np.asarray(w, dtype=np.longdouble)
    X, res = refined_inverse(_resolvent_matrix(Hk, z), tol)
    gn = np.sqrt((np.abs(X) ** 2).sum(axis=(-2, -1)))
    return np.tensordot(w.astype(np.clongdouble), X, axes=(0, 0)) / w.sum(), res, float(res * (np.abs(w) * gn).sum() / w.sum())


def rule_sum(Hk, w, z, kind):
    """The weighted mean over the nodes of G ("gloc", [n, n]), tr G ("trgloc") or -Im tr G / pi ("dos") at z, from
    refined_inverse, accumulated in long double."""
    return _of_kind(summed_g(Hk, w, z)[0], kind)


def amplification(Hk, w, z):
    """A = sum_k |w_k| ||G_k||_F^2 (||H_k||_F + |z|) / sum_k w_k: the first-order bound on what a perturbation eps |H| of
    the input does to tr G or to any entry of the summed G (|tr(G dH G)| <= ||G||_F^2 ||dH||_F).  For normal H this is
    sum_i (||H|| + |z|) / |z - lambda_i|^2."""
    Hk = np.asarray(Hk, dtype=np.complex128)
    w = np.asarray(w, dtype=np.float64)
    G = np.linalg.inv(_resolvent_matrix(Hk, z))  # (two digits of A are plenty)
    g2 = (np.abs(G) ** 2).sum(axis=(-2, -1))
    hn = np.sqrt((np.abs(Hk) ** 2).sum(axis=(-2, -1)))
    return float((np.abs(w) * g2 * (hn + abs(complex(z)))).sum() / w.sum())


def worst_cond(Hk, z):
    """Largest 2-norm condition number of z I - H(k) over the nodes."""
    return float(np.linalg.cond(_resolvent_matrix(Hk, z)).max())


def lapack_sum(Hk, w, z):
    """The same mean of G by the plain complex128 route (what r_lapack measures)."""
    w = np.asarray(w, dtype=np.float64)
    return np.tensordot(w.astype(np.complex128), np.linalg.inv(_resolvent_matrix(Hk, z)), axes=(0, 0)) / w.sum()


# ---------------------------------------------------------------------------------------------------------------- builders
def _hermitian_hopping(rng, dims, n):
    """Random coefficients with c[-R] = c[R]^dagger exactly (what the library detects as a Hermitian series)."""
    c = rng.standard_normal(dims + (n, n)) + 1j * rng.standard_normal(dims + (n, n))
    flip = c[tuple(slice(None, None, -1) for _ in dims)]
    return 0.5 * (c + np.conj(np.swapaxes(flip, -1, -2)))


def _centre(dims):
    return tuple(m // 2 for m in dims)


def gapped_hermitian(rng, dims, n, gap, delta=1.0):
    """A constant block diag(+delta ..., -delta ...) plus Hermitian hopping T(k) whose coefficients' 2-norms sum to
    0.9 (delta - gap / 2): ||T(k)||_2 < delta - gap / 2 at every k, so by Weyl's inequality no eigenvalue of H(k) lies in
    (-gap / 2, gap / 2).  `dims`: odd extents.  Returns (c, first)."""
    assert all(m % 2 == 1 for m in dims) and 0.0 < gap < 2.0 * delta
    c = _hermitian_hopping(rng, dims, n)
    total = sum(np.linalg.norm(c[idx], 2) for idx in np.ndindex(*dims))
    c *= 0.9 * (delta - 0.5 * gap) / total
    sign = np.where(np.arange(n) < (n + 1) // 2, 1.0, -1.0)
    c[_centre(dims)] += np.diag(delta * sign)
    return c, tuple(-(m // 2) for m in dims)


def dissipative(rng, dims, n, gamma):
    """A Hermitian series of norm about 1 plus -i Gamma, Gamma = gamma (I + P) constant with P Hermitian, 0 <= P <= I: so
    Gamma >= gamma I, and every leading minor of omega I - H(k) = (omega I - H_h(k)) + i Gamma has its field of values in
    the upper half plane at distance >= gamma from the real axis -- the unpivoted elimination's own precondition.  The
    Hermitian part does not depend on gamma (same rng state, same H_h).  Returns (c, first)."""
    assert all(m % 2 == 1 for m in dims) and gamma > 0.0
    c = _hermitian_hopping(rng, dims, n) / np.sqrt(n * np.prod(dims))
    B = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    P = B @ B.conj().T
    P = 0.5 * (P + P.conj().T)
    P /= np.linalg.eigvalsh(P)[-1]
    c[_centre(dims)] += -1j * gamma * (np.eye(n) + P)
    return c, tuple(-(m // 2) for m in dims)


def pole_sweep(Hk, node, eta):
    """Five swept values for the matrices Hk [nk, n, n]: [0] exactly on a float64 eigenvalue (its real part, where H is
    not Hermitian) of node `node`, so that this pole lies at the distance eta the case sets and no further; [1] midway
    between the two neighbouring eigenvalues of that node that lie furthest apart; [2] outside the spectrum of the whole
    grid; [3] on another eigenvalue of the node; [4] a quarter of the way from the first pole to the midway point.  (`eta`
    only keeps the value outside the spectrum at a distance that is not small against it.)"""
    Hk = np.asarray(Hk, dtype=np.complex128)
    hn = Hk[node]
    if np.abs(hn - hn.conj().T).max() <= 1e-14 * np.abs(hn).max():
        e = np.linalg.eigvalsh(hn)
    else:
        e = np.sort(np.linalg.eigvals(hn).real)
    rho = float(np.abs(np.linalg.eigvals(Hk)).max())
    n = len(e)
    j = n // 2
    if n >= 2:
        i = int(np.argmax(np.diff(e)))
        mid = 0.5 * (e[i] + e[i + 1])
        other = e[(j + 1 + n // 3) % n]
    else:
        mid = e[0] + 0.37 * rho
        other = e[0] - 0.21 * rho
    outside = 1.25 * rho + 10.0 * eta
    return np.array([e[j], mid, outside, other, e[j] + 0.25 * (mid - e[j])], dtype=np.float64)


def spectral_radius(Hk):
    """rho: the largest |eigenvalue| over the grid."""
    return float(np.abs(np.linalg.eigvals(np.asarray(Hk, dtype=np.complex128))).max())


# ------------------------------------------------------------------------------------------------------------------- cases
BANDS = (1, 2, 3, 4, 5, 8, 12, 16, 17, 24, 32, 33, 48, 64)
RATIOS = (1e-2, 1e-4, 1e-6)
GAP = 0.5
ORIGIN_SWEEP = np.array([-0.25, 0.0, 0.1, 0.25, 0.4]) * GAP  # [1] = 0.0 is the sweep of one value
ORIGIN_GAMMA = 0.1  # the dissipative cases at the origin: cond <= (||H_h|| + 2 gamma) / gamma, about 30


def grid_of(n):
    """(d, npt): the smallest grids that leave ragged slots: 25 nodes (odd against 8, 4 and 2 nodes per wave) up to 32
    bands, 13 nodes above."""
    return (2, 5) if n <= 32 else (1, 13)


# nodes_per_block of the register-resident inverse exceeds the nodes per wave and leaves a remainder: (bands, d, npt);
# 5 bands: 4913 nodes, 10 per block, 8 per wave; 12 bands: 2601, 6, 4; 20 bands: 1089, 3, 2
RAGGED = ((5, 3, 17), (12, 2, 51), (20, 2, 33))
RAGGED_RATIO = 1e-4  # the ragged grids in groups (b) and (c): one eta, the one of group (c)
# the closed-form store-free kernel of 1...4 bands serves grid lines of more than 128 points only
LONG_LINE = tuple((n, 1, 129) for n in (1, 2, 3, 4))


class Case:
    """One series on one grid with its swept values: the inputs of a GPU test and everything it is compared with
    (computed once per case: ref[kind] over the sweep, amp[i], cond, residual)."""

    def __init__(self, name, c, first, d, npt, eta, sweep, tol=1e-15, one=0):
        self.one = one  # which of the swept values makes the sweep of one value
        self.name, self.c, self.first, self.d, self.npt, self.eta, self.tol = name, c, first, d, npt, float(eta), tol
        self.n = c.shape[-1]
        self.sweep = np.asarray(sweep, dtype=np.float64)
        self.Hk = fourier_nodes(c, first, npt, d)
        self.w = np.ones(len(self.Hk))
        self._ref = None

    def _compute(self):
        if self._ref is None:
            G, res, amp, cond, rerr = [], 0.0, [], 0.0, []
            for om in self.sweep:
                z = complex(om, self.eta)
                g, r, e = summed_g(self.Hk, self.w, z, self.tol)
                G.append(g)
                res = max(res, r)
                rerr.append(e * np.sqrt(self.n))
                amp.append(amplification(self.Hk, self.w, z))
                cond = max(cond, worst_cond(self.Hk, z))
            self._ref = (np.stack(G), res, np.array(amp), cond, np.array(rerr))
        return self._ref

    def ref(self, kind):
        """[n_sweep, ncomp] long double, components of G in the library's order (row fastest)."""
        G = self._compute()[0]
        if kind == "gloc":
            return np.swapaxes(G, -1, -2).reshape(len(self.sweep), -1)
        return _of_kind(G, kind).reshape(len(self.sweep), 1)

    @property
    def amp(self):
        return self._compute()[2]

    @property
    def cond(self):
        return self._compute()[3]

    @property
    def residual(self):
        return self._compute()[1]

    @property
    def ref_err(self):
        """[n_sweep] bound on the reference's own error (any entry of the mean of G, or its trace)."""
        return self._compute()[4]

    def lapack(self, kind):
        G = np.stack([lapack_sum(self.Hk, self.w, complex(om, self.eta)) for om in self.sweep])
        if kind == "gloc":
            return np.swapaxes(G, -1, -2).reshape(len(self.sweep), -1)
        return np.asarray(_of_kind(G, kind)).reshape(len(self.sweep), 1)


def _dims(d, n):
    return (3,) * d if n <= 32 else (3,)


def _seed(n, d, npt, tag):
    return [20250, n, d, npt, tag]


def origin_case(n, herm, d=None, npt=None):
    """Group (a): eta = 0 at the origin and four more values inside the gap."""
    if d is None:
        d, npt = grid_of(n)
    rng = np.random.default_rng(_seed(n, d, npt, 1 if herm else 2))
    if herm:
        c, first = gapped_hermitian(rng, _dims(d, n), n, GAP)
    else:
        c, first = dissipative(rng, _dims(d, n), n, ORIGIN_GAMMA)
    return Case(f"origin n={n} d={d} npt={npt} {'herm' if herm else 'diss'}", c, first, d, npt, 0.0, ORIGIN_SWEEP, one=1)


def small_eta_case(n, herm, ratio, d=None, npt=None):
    """Group (b): a pole at distance ratio * rho.  Hermitian: eta = ratio * rho.  Dissipative: gamma = ratio * rho and
    eta = 0 (a series that carries its own broadening)."""
    if d is None:
        d, npt = grid_of(n)
    seed = _seed(n, d, npt, 3 if herm else 4)
    if herm:
        c = _hermitian_hopping(np.random.default_rng(seed), _dims(d, n), n) / np.sqrt(n * 3 ** d)
        first = tuple(-(m // 2) for m in c.shape[:d])
        Hk = fourier_nodes(c, first, npt, d)
        eta = ratio * spectral_radius(Hk)
        dist = eta
    else:
        # (the Hermitian part does not depend on gamma: rho from a first build)
        c0, first = dissipative(np.random.default_rng(seed), _dims(d, n), n, 1e-300)
        dist = ratio * spectral_radius(fourier_nodes(c0, first, npt, d))
        c, first = dissipative(np.random.default_rng(seed), _dims(d, n), n, dist)
        Hk = fourier_nodes(c, first, npt, d)
        eta = 0.0
    sweep = pole_sweep(Hk, len(Hk) // 2, dist)
    # (the residual of an inverse cannot fall below about 1e-19 cond: refined_inverse)
    return Case(f"eta/rho={ratio:g} n={n} d={d} npt={npt} {'herm' if herm else 'diss'}", c, first, d, npt, eta, sweep,
                tol=1e-15 if ratio >= 1e-4 else 1e-13)


def edge_cases():
    """Every case test_gpu_resolvent_edges.py runs, as (constructor, arguments): built lazily, one at a time."""
    out = []
    for herm in (True, False):
        for n in BANDS:
            out.append((origin_case, (n, herm)))
            for ratio in RATIOS:
                out.append((small_eta_case, (n, herm, ratio)))
        for n, d, npt in RAGGED:
            out.append((origin_case, (n, herm, d, npt)))
            out.append((small_eta_case, (n, herm, RAGGED_RATIO, d, npt)))
    for n, d, npt in LONG_LINE:
        out.append((origin_case, (n, True, d, npt)))
        for ratio in RATIOS:
            out.append((small_eta_case, (n, True, ratio, d, npt)))
    return out
