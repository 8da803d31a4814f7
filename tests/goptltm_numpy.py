"""numpy restatement of the Green's functions of the optimized tetrahedron method (helper of
test_ltm_green_optimized_cpu.py / test_gpu_ltm_green_optimized.py, not a conftest).

A composition that holds no table of its own: optltm_numpy.effective_corners gives the effective corner values e' (and A') of
every (permutation, cell) from the projection it derives in exact rationals; gltm_numpy.simplex_J_any (the trace) and
gwltm_numpy.simplex_weights_any (the corner weights) are the evaluation rule of the linear Green's functions, run on the sorted
e' with A' carried along.  Weight 1 / (6 npt^3) per simplex, an exactly rounded sum (fsum) per z.

`dtype`: the type in which the 20-point product is formed; the result is rounded to f64 before the closed forms, which are
f64 only.  np.longdouble against np.float64 shows what the rounding of e' does to the sums (the conditioning of a case).
"""
import math

import numpy as np

import gltm_numpy as gn
import gwltm_numpy as gwn
import optltm_numpy as on


def corners(eig, A=None, dtype=np.float64, optimized=True):
    """eig [npt]*3 + [n], A None, "energy" or [ncomp] + eig.shape -> (e' [S, 4] ascending, A' [S, 4, ncomp] or None) as f64, one row
    per (permutation, cell, band); optimized=False: the plain corner values."""
    eig = np.asarray(eig, dtype=dtype)
    ce = on.effective_corners(eig, dtype, optimized)                       # [6 ncell, 4, n]
    if A is None:
        cA = None
    elif isinstance(A, str):
        assert A == "energy"
        cA = ce[..., None]
    else:
        A = np.asarray(A, dtype=dtype)
        assert A.shape[1:] == eig.shape, (A.shape, eig.shape)
        cA = on.effective_corners(np.moveaxis(A, 0, -1), dtype, optimized)  # [6 ncell, 4, n, ncomp]
    ce = ce.transpose(0, 2, 1).reshape(-1, 4).astype(np.float64)
    o = np.argsort(ce, axis=1, kind="stable")
    ce = np.take_along_axis(ce, o, 1)
    if cA is not None:
        cA = cA.transpose(0, 2, 1, 3).reshape(len(ce), 4, -1).astype(np.float64)
        cA = np.take_along_axis(cA, o[:, :, None], 1)
    return ce, cA


def green(eig, A, zs, dtype=np.float64, optimized=True):
    """tr G(z) [nz] (A None) or G_A(z) [nz, ncomp] of the optimized rule, per unit cell and summed over bands, at the complex
    energies zs (Im z != 0); optimized=False: of the linear rule."""
    shape = np.shape(eig)
    ce, cA = corners(eig, A, dtype, optimized)
    w = 1.0 / (6.0 * shape[0] * shape[1] * shape[2])
    zs = np.atleast_1d(np.asarray(zs, dtype=np.complex128))
    if cA is None:
        out = np.empty(len(zs), dtype=np.complex128)
        for i, z in enumerate(zs):
            J = gn.simplex_J_any(ce, z)
            out[i] = complex(math.fsum(J.real), math.fsum(J.imag)) * w
        return out
    out = np.empty((len(zs), cA.shape[2]), dtype=np.complex128)
    for i, z in enumerate(zs):
        W = gwn.simplex_weights_any(ce, z)
        for c in range(cA.shape[2]):
            t = (cA[:, :, c] * W).ravel()
            out[i, c] = complex(math.fsum(t.real), math.fsum(t.imag)) * w
    return out


def z_lists(eig):
    """The z lists of the parity cases.  "generic": real parts inside and outside the bands with Im z in {0.5, 1e-2, 1e-4, -1e-3};
    "edges": eight effective corner values e' of the grid itself + 1e-8j (spread over the sorted e')."""
    lo, hi = float(np.min(eig)), float(np.max(eig))
    w = hi - lo
    re = np.array([lo - 0.3 * w, lo + 0.137 * w, lo + 0.52 * w, lo + 0.861 * w, hi + 0.3 * w])
    generic = np.array([x + 1j * y for y in (0.5, 1e-2, 1e-4, -1e-3) for x in re])
    e = np.unique(corners(eig)[0])
    edges = e[np.linspace(0, len(e) - 1, 10).astype(int)[1:-1]] + 1e-8j
    return {"generic": generic, "edges": edges}
