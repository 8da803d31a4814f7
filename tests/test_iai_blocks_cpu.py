"""IAI building blocks, CPU side: the numpy restatement (tests/iai_blocks_numpy.py) and its host-driven nested GK loop
against the oracle's own nested quadrature, so that the driver is proven before test_gpu_iai_blocks.py points it at the
device entry points abz_contract_nodes / abz_eval_line_nodes / abz_release_level."""
import numpy as np
import pytest

import abz_oracle as orc
import iai_blocks_numpy as ib
from test_gpu_fuzz import _herm_series

# (n, dims, eta, omega, abstol, seed): Hermitian random coefficients scaled by 1 / sqrt(n), the DOS integrand.  Measured:
# 1155 and 16155 evaluations; one GK panel per variable would be 15^2 = 225 and 15^3 = 3375, so both refine.
DRIVER_CASES = [(3, (3, 3), 0.3, 0.3, 1e-2, 9), (1, (3, 3, 3), 0.4, 0.3, 1e-2, 9)]


def driver_case(n, dims, seed):
    c, first = _herm_series(np.random.default_rng(seed), dims, n, 1.0 / np.sqrt(n))
    return c, first, orc.FourierSeries(c, period=1.0, first=first, ndim=len(dims))


@pytest.mark.parametrize("n,dims,eta,omega,abstol,seed", DRIVER_CASES)
def test_nested_gk_on_numpy_blocks_reproduces_nested_quad(n, dims, eta, omega, abstol, seed):
    """Same panels, same float operations: numevals equal and the value bit-identical when the oracle integrates the
    restatement's own integrand function; against the oracle's f_dos (a real scalar instead of a one-component complex
    vector) the counts are equal too and the values agree to rounding."""
    d = len(dims)
    _, _, so = driver_case(n, dims, seed)
    lims = orc.CubicLimits(np.zeros(d), np.ones(d))
    blocks = ib.NumpyBlocks(so)
    I, E, nev = ib.nested_gk(blocks, d, lims, ib.F_DOS, [eta], omega, abstol=abstol)
    f = lambda X, H: ib.integrand_ref(ib.F_DOS, n, d, [eta], omega, X, H)
    I0, E0, nev0 = orc.nested_quad(so, lims, f, abstol=abstol)
    print(f"n={n} dims={dims}: numevals {nev} (first panels alone: {15 ** d}), I = {I[0].real:.15g}")
    assert nev == nev0 and nev > 15 ** d
    assert I.shape == (1,) and np.array_equal(I, I0) and E == E0
    I1, E1, nev1 = orc.nested_quad(so, lims, orc.f_dos(eta, omega), abstol=abstol)
    assert nev1 == nev and abs(I[0] - I1) <= 1e-13 * abs(I1) and I[0].imag == 0.0
    assert all(len(blocks.sets[L]) == 0 for L in range(1, d))  # everything released at the end


def test_numpy_blocks_slot_numbering_and_release():
    rng = np.random.default_rng(3)
    c = rng.standard_normal((2, 3, 2, 2, 2)) + 1j * rng.standard_normal((2, 3, 2, 2, 2))
    so = orc.FourierSeries(c, period=(1.0, 2.0, 0.5), first=(-1, 0, -2), ndim=3)
    b = ib.NumpyBlocks(so)
    assert np.array_equal(b.contract_nodes(3, [0, 0, 0], [0.1, 0.2, 0.3]), [0, 1, 2])
    assert np.array_equal(b.contract_nodes(3, [0, 0], [0.4, 0.5]), [3, 4])  # appended per call
    assert np.array_equal(b.contract_nodes(2, [4, 0, 4], [0.7, -0.3, 1.9]), [0, 1, 2])
    assert np.array_equal(b.contract_nodes(2, [2], [0.6]), [3])
    x3, x2, x1 = 0.5, 1.9, 0.25
    v = b.eval_line_nodes([2, 3], [x1, x1], ib.F_GLOC, [0.5], 0.1)
    for row, (a3, a2) in zip(v, ((0.5, 1.9), (0.3, 0.6))):
        g = np.linalg.inv((0.1 + 0.5j) * np.eye(2) - orc.evaluate_direct(so, [x1, a2, a3]))
        assert np.abs(row.reshape(2, 2).T - g).max() <= 1e-13 * np.abs(g).max()  # column-major G, the right parents
    with pytest.raises(ValueError, match=r"parents\[1\] = 4 .*4 live"):
        b.eval_line_nodes([0, 4], [0.0, 0.0], ib.F_DOS, [0.5], 0.1)
    with pytest.raises(ValueError, match=r"parents\[0\] = -1"):
        b.contract_nodes(2, [-1], [0.0])
    with pytest.raises(ValueError, match=r"parents\[2\] = 1 .*1 live"):
        b.contract_nodes(3, [0, 0, 1], [0.0, 0.0, 0.0])  # level d holds the series alone
    assert len(b.sets[2]) == 5 and len(b.sets[1]) == 4  # a refused call appends nothing
    with pytest.raises(ValueError):
        b.contract_nodes(1, [0], [0.0])
    with pytest.raises(ValueError):
        b.contract_nodes(4, [0], [0.0])
    b.release_level(2)  # the levels below 2
    assert len(b.sets[1]) == 0 and len(b.sets[2]) == 5
    with pytest.raises(ValueError):  # a stale slot
        b.eval_line_nodes([0], [0.0], ib.F_DOS, [0.5], 0.1)
    assert np.array_equal(b.contract_nodes(2, [1], [0.2]), [0])
    b.release_level(3)
    assert len(b.sets[1]) == 0 and len(b.sets[2]) == 0 and b.sets[3] == [so]
    assert np.array_equal(b.contract_nodes(3, [0], [0.2]), [0])
    b.release_level(1)  # nothing lies below level 1
    assert len(b.sets[2]) == 1


def test_integrand_ref_menu():
    """Every integrand id of the menu at nodes, against formulas written out here."""
    rng = np.random.default_rng(5)
    n, d, N = 3, 2, 4
    X = rng.uniform(-1, 1, (N, d))
    H = rng.standard_normal((N, n, n)) + 1j * rng.standard_normal((N, n, n))
    eta, w = 0.45, 0.2
    G = np.stack([np.linalg.inv((w + 1j * eta) * np.eye(n) - h) for h in H])
    assert np.array_equal(ib.integrand_ref(ib.F_ONE, n, d, [], 0.0, X, H), np.ones((N, 1)))
    assert np.allclose(ib.integrand_ref(ib.F_GLOC, n, d, [eta], w, X, H).reshape(N, n, n), np.transpose(G, (0, 2, 1)), rtol=1e-14, atol=0)
    tr = np.trace(G, axis1=1, axis2=2)
    assert np.allclose(ib.integrand_ref(ib.F_TRGLOC, n, d, [eta], w, X, H)[:, 0], tr, rtol=1e-14, atol=0)
    assert np.allclose(ib.integrand_ref(ib.F_DOS, n, d, [eta], w, X, H)[:, 0], -tr.imag / np.pi, rtol=1e-14, atol=0)
    Hh = 0.5 * (H + np.conj(np.transpose(H, (0, 2, 1))))
    dos_h = ib.integrand_ref(ib.F_DOS, n, d, [eta], w, X, Hh)[:, 0]
    assert np.allclose(ib.integrand_ref(ib.F_DOS_EIG, n, d, [eta], w, X, Hh)[:, 0], dos_h, rtol=1e-12, atol=0)
    up = np.triu(H) + np.conj(np.transpose(np.triu(H, 1), (0, 2, 1)))  # Hermitian(H) reads the upper triangle
    up[:, range(n), range(n)] = H[:, range(n), range(n)].real
    assert np.allclose(ib.integrand_ref(ib.F_DOS_EIG, n, d, [eta], w, X, H)[:, 0], ib.integrand_ref(ib.F_DOS, n, d, [eta], w, X, up)[:, 0],
                       rtol=1e-12, atol=0)
    s = rng.standard_normal((N, 1, 1)) + 1j * rng.standard_normal((N, 1, 1))
    assert np.array_equal(ib.integrand_ref(ib.F_LINEAR, 1, d, [2.0, -0.5], 0.0, X, s)[:, 0], 2.0 * s[:, 0, 0] - 0.5)
    assert np.array_equal(ib.integrand_ref(ib.F_LINEAR_X, 1, d, [2.0, -0.5], 0.0, X, s), 2.0 * s[:, 0, 0][:, None] * X - 0.5)
    assert [ib.ncomp(f, n, d) for f in range(7)] == [1, 1, d, 1, 1, n * n, 1]
