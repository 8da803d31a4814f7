"""Series whose resolvent needs row pivoting (helper of test_pivot_cpu.py / test_gpu_pivot.py, not a conftest).

Every family has a zero diagonal in EVERY coefficient, so the (0, 0) entry of z I - H(k) is z itself at every node: an
elimination without pivoting divides by omega at eta = 0 (NaN at omega = 0, about eps / omega lost at omega = 1e-9), while
the matrices are as well conditioned as a matrix gets (cond <= 4: the constant part is unitary, or a direct sum of sigma_x,
and |z| <= 1/4).  LAPACK's `inv`, which pivots by rows, returns them to a fraction of eps * amplification.

    shift        constant coefficient: the cyclic shift np.roll(eye(n), 1, axis=1) ([[0, 1], [2, 0]] for n = 2, where the
                 shift itself would be Hermitian) -- every pivot comes from another row;
    derangement  a seeded fixed-point-free permutation matrix with unit-modulus phases -- a general permutation to undo;
    paired       Hermitian, even n: kron(I_{n/2}, sigma_x) plus hopping with c(-R) = c(R)^dagger exactly.
Hopping: (N(0, 1) + i N(0, 1)) 0.1 / n on 3^d coefficients, first = -1.  eta = 0, swept values SWEEP; the sweep of one value
is omega = 0.  The reference is resolvent_ref.Case, unchanged.
"""
import numpy as np

import resolvent_ref as rr

ETA = 0.0
SWEEP = np.array([-0.25, 0.0, 1e-9, 0.1, 0.25])
ONE = 1  # SWEEP[ONE] = 0.0 is the sweep of one value
NONHERM_BANDS = (2, 3, 4, 5, 8, 12, 16, 17, 20, 24, 28, 32, 33, 40, 48, 56, 64)  # every (NQ, SUBS) of big_inverse_kernel
PAIRED_BANDS = (2, 4, 8, 16, 32, 64)
SMALL = (8, 1, 3)  # (bands, d, npt): fewer nodes than a wave has slots


def grid_of(n):
    """(d, npt): 25 nodes up to 16 bands, 7 above -- no multiple of the 2, 4 or 8 nodes a wave holds."""
    return (2, 5) if n <= 16 else (1, 7)


def _zero_diagonals(c):
    n = c.shape[-1]
    c[..., np.arange(n), np.arange(n)] = 0.0
    return c


def _hopping(rng, d, n):
    dims = (3,) * d
    c = (rng.standard_normal(dims + (n, n)) + 1j * rng.standard_normal(dims + (n, n))) * (0.1 / n)
    return _zero_diagonals(c)


def _seed(n, d, npt, tag):
    return [20251, n, d, npt, tag]


def _case(name, c, d, npt):
    return rr.Case(name, c, (-1,) * d, d, npt, ETA, SWEEP, one=ONE)


def shift_case(n, d=None, npt=None):
    if d is None:
        d, npt = grid_of(n)
    c = _hopping(np.random.default_rng(_seed(n, d, npt, 1)), d, n)
    c[(1,) * d] += np.array([[0.0, 1.0], [2.0, 0.0]]) if n == 2 else np.roll(np.eye(n), 1, axis=1)
    return _case(f"shift n={n} d={d} npt={npt}", c, d, npt)


def derangement(rng, n):
    """A permutation of 0 ... n - 1 without a fixed point (rejection sampling: about one draw in e passes)."""
    while True:
        p = rng.permutation(n)
        if not (p == np.arange(n)).any():
            return p


def derangement_case(n, d=None, npt=None):
    if d is None:
        d, npt = grid_of(n)
    rng = np.random.default_rng(_seed(n, d, npt, 2))
    c = _hopping(rng, d, n)
    P = np.zeros((n, n), dtype=np.complex128)
    P[np.arange(n), derangement(rng, n)] = np.exp(2j * np.pi * rng.random(n))
    c[(1,) * d] += P
    return _case(f"derangement n={n} d={d} npt={npt}", c, d, npt)


def paired_case(n, d=None, npt=None):
    assert n % 2 == 0
    if d is None:
        d, npt = grid_of(n)
    c = _hopping(np.random.default_rng(_seed(n, d, npt, 3)), d, n)
    flip = c[tuple(slice(None, None, -1) for _ in range(d))]
    c = _zero_diagonals(0.5 * (c + np.conj(np.swapaxes(flip, -1, -2))))  # c(-R) = c(R)^dagger exactly
    c[(1,) * d] += np.kron(np.eye(n // 2), np.array([[0.0, 1.0], [1.0, 0.0]]))
    return _case(f"paired n={n} d={d} npt={npt}", c, d, npt)


FAMILIES = {"shift": shift_case, "derangement": derangement_case, "paired": paired_case}


def all_cases():
    """(family, n, d, npt) of every case the tests run; d = npt = None: grid_of(n)."""
    out = [(fam, n, None, None) for fam in ("shift", "derangement") for n in NONHERM_BANDS]
    out += [("paired", n, None, None) for n in PAIRED_BANDS]
    out += [(fam, SMALL[0], SMALL[1], SMALL[2]) for fam in FAMILIES]
    return out


def case_id(p):
    fam, n, d, npt = p
    return f"{fam}-{n}" + (f"-{d}d{npt}" if d else "")


_CASES = {}


def get(p):
    """The case of one all_cases() entry, built once per process (its reference is computed on first use and kept)."""
    if p not in _CASES:
        fam, n, d, npt = p
        _CASES[p] = FAMILIES[fam](n) if d is None else FAMILIES[fam](n, d, npt)
    return _CASES[p]


def unpivoted_sum(Hk, w, z):
    """The mean of G over the nodes by Gauss-Jordan in place WITHOUT pivoting in complex128: the arithmetic of the device's
    default route (pivot c is entry (c, c), whatever it is), restated in numpy for all nodes at once."""
    Hk = np.asarray(Hk, dtype=np.complex128)
    n = Hk.shape[-1]
    A = complex(z) * np.eye(n) - Hk
    with np.errstate(all="ignore"):
        for c in range(n):
            ip = 1.0 / A[:, c, c]
            q = A[:, :, c] * ip[:, None]
            row = A[:, c, :].copy()
            A = A - q[:, :, None] * row[:, None, :]
            A[:, c, :] = ip[:, None] * row
            A[:, :, c] = -q
            A[:, c, c] = ip
        w = np.asarray(w, dtype=np.float64)
        return np.tensordot(w.astype(np.complex128), A, axes=(0, 0)) / w.sum()
