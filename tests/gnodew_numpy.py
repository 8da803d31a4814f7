"""numpy restatement of the complex integration weights of the Green's function per grid point and band (helper of
test_ltm_green_node_weights_cpu.py / test_gpu_ltm_green_node_weights.py, not a conftest).

    W_b(k; z) = w sum_{T contains k} W^T_{i(k)}(z),      w = 1 / (d! npt^d),

with  G_A(z) = sum_k sum_b W_b(k; z) A_b(k)  for any A, on the mesh of ltm_numpy.py.  The scatter form of gwltm_numpy.py: the
sorted corners of every simplex and the flat (k, b) index of each are nodew_numpy.simplices, the d + 1 corner weights of a
simplex are gwltm_numpy.simplex_weights_any (W_i = J[x_0 .. x_m, x_i] / (m + 1), the evaluation rule of gltm_numpy.simplex_J),
and np.add.at scatters them onto the (k, b) they belong to: at most (d+1)! terms per entry.  Equal simplices (sorted energies)
are evaluated once.  Im z < 0: the conjugate of the weights at conj(z), to the bit (simplex_weights_any conjugates, the scatter
adds real and imaginary parts separately in the same order).
"""
import math

import numpy as np

import gwltm_numpy as gw
import nodew_numpy as nw

simplices = nw.simplices


def node_weights_from(simp, shape, zs):
    """The weights complex128 [nz] + shape from what simplices() returned (share it among lists of z)."""
    e, idx, d = simp
    nk = int(np.prod(shape[:d]))
    w = 1.0 / (math.factorial(d) * float(nk))
    rows, inv = np.unique(e, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    zs = np.atleast_1d(np.asarray(zs, dtype=np.complex128)).reshape(-1)
    W = np.zeros((len(zs), int(np.prod(shape))), dtype=np.complex128)
    flat = idx.reshape(-1)
    for i, z in enumerate(zs):
        share = gw.simplex_weights_any(rows, z)[inv].reshape(-1)
        re, im = np.zeros(W.shape[1]), np.zeros(W.shape[1])
        np.add.at(re, flat, share.real)
        np.add.at(im, flat, share.imag)
        W[i] = (re * w) + 1j * (im * w)
    return W.reshape((len(zs),) + tuple(shape))


def node_weights(eig, zs):
    """eig [npt]*d + [n] ascending eigenvalues, complex zs (Im z != 0) -> W_b(k; z) as complex128 [nz] + eig.shape."""
    eig = np.asarray(eig, dtype=np.float64)
    return node_weights_from(simplices(eig), eig.shape, zs)
