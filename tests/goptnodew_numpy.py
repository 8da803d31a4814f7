"""numpy restatement of the complex integration weights of the optimized tetrahedron method (helper of
test_ltm_green_node_weights_optimized_cpu.py / test_gpu_ltm_green_node_weights_optimized.py, not a conftest).

    W_b(k; z) = 1 / (6 npt^3) sum_t sum_{j = 1..20} sum_{m = 1..4} P[m][j] W'_m(T = (t, cell k - off_{t,j}); z),

with  G_A(z) = sum_k sum_b W_b(k; z) A_b(k)  the G_A of goptltm_numpy.green for any A.  The scatter form of optnodew_numpy.py with
the complex corner weights of gwltm_numpy.simplex_weights_any (W'_m = J[sort(e'), e'_m] / 4) in place of the real ones: for every
path and cell the band is taken at the 20 stencil points, e' = P e, the corners are sorted (stable), the corner weights are
brought back to path order, P^T W' is added at cell + off_j with np.roll, every index mod npt.  It holds no table of its own.

`dtype`: the type in which the 20-point product is formed; e' is rounded to f64 before the closed forms, which are f64 only
(as in goptltm_numpy).  Real and imaginary parts are scattered separately in the same order, so Im z < 0 gives the conjugate
of the weights at conj(z) to the bit.
"""
import itertools

import numpy as np

import gwltm_numpy as gwn
import optltm_numpy as on


def corner_weights(e, z):
    """Effective corner energies e [K, 4] (f64) in path order -> complex128 [K, 4]: the corner weights W'_m(z) in path order, unit =
    one simplex (they sum to J of the simplex)."""
    o = np.argsort(e, axis=1, kind="stable")
    es = np.take_along_axis(e, o, 1)
    ws = gwn.simplex_weights_any(es, z)
    out = np.empty_like(ws)
    np.put_along_axis(out, o, ws, 1)  # sorted corner s is corner o[s] of the path
    return out


def node_weights(eig, zs, dtype=np.float64):
    """eig [npt, npt, npt, n] ascending eigenvalues, complex zs (Im z != 0) -> W_b(k; z) as complex128 [nz, npt, npt, npt, n]."""
    eig = np.asarray(eig, dtype=dtype)
    npt = eig.shape[0]
    assert eig.shape[:3] == (npt, npt, npt)
    zs = np.atleast_1d(np.asarray(zs, dtype=np.complex128)).reshape(-1)
    P = on.projection_float(dtype)
    P64 = on.projection_float(np.float64)
    shape = (len(zs),) + eig.shape
    re, im = np.zeros(shape), np.zeros(shape)
    for perm in itertools.permutations(range(3)):
        x = on.stencil_values(eig, perm)                                            # [20, ncell, n]
        ep = np.tensordot(P, x, axes=(1, 0))                                        # [4, ncell, n]
        ep = np.ascontiguousarray(np.moveaxis(ep, 0, -1).reshape(-1, 4)).astype(np.float64)
        cw = np.stack([corner_weights(ep, z) for z in zs])                          # [nz, ncell n, 4]
        pr, pi = np.matmul(cw.real, P64), np.matmul(cw.imag, P64)                   # [nz, ncell n, 20]: P^T W'
        for j, off in enumerate(on.points(perm)):
            gr, gi = pr[..., j].reshape(shape), pi[..., j].reshape(shape)           # at the cell
            for ax in range(3):
                if off[ax]:
                    gr = np.roll(gr, int(off[ax]), axis=ax + 1)                     # to the point cell + off, wrapped
                    gi = np.roll(gi, int(off[ax]), axis=ax + 1)
            re += gr
            im += gi
    w = 1.0 / (6.0 * npt ** 3)
    return (re * w) + 1j * (im * w)
