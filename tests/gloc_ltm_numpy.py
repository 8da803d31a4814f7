"""numpy restatement of the local Green's function matrix of the tetrahedron method (helper of test_ltm_green_matrix_cpu.py /
test_gpu_ltm_green_matrix.py, not a conftest).

    G_pq(z) = sum_b int dk P^b_pq(k) / (z - e_b(k)),     P^b_pq(k) = U_pb(k) conj(U_qb(k)),

U(k) the eigenvector matrix of Hermitian(H(k)), bands ascending.  The projector does not change when column b of U is
multiplied by a phase, so LAPACK's and the device's agree wherever level b is not degenerate; inside a degenerate level only
the sum of the projectors over the level is defined.  Re P and Im P are real matrix elements of the tetrahedron method
(gwltm_numpy.green_weighted: linear inside a simplex like the energy), and

    G_pq(z) = G_{Re P}(z) + i G_{Im P}(z),     G_qp(z) = G_{Re P}(z) - i G_{Im P}(z)        (P^b_qp = conj(P^b_pq)).

Components: a pair (p, p) is one component, |U_pb|^2; a pair p != q is two, Re P^b_pq = ur_p ur_q + ui_p ui_q, then
Im P^b_pq = ui_p ur_q - ur_p ui_q -- the order abz_rule_ltm_projectors writes them in."""
import numpy as np

import gwltm_numpy as gw


def ncomponents(pairs):
    return sum(1 if p == q else 2 for p, q in pairs)


def eigenvectors(H):
    """H [..., n, n] Hermitian (the upper triangle is read) -> U [..., n, n], columns = bands ascending."""
    return np.linalg.eigh(np.asarray(H), UPLO="U")[1]


def projector_tensor(H):
    """H [..., n, n] -> P [n(p), n(q), ..., n(b)] complex, P[p, q, ..., b] = U_pb conj(U_qb)."""
    U = eigenvectors(H)
    return np.einsum("...pb,...qb->pq...b", U, U.conj())


def projectors(H, pairs):
    """H [nk, n, n] -> the components [ncomp, nk, n] of `pairs`, the layout of DeviceRule.ltm_elements_export after
    DeviceRule.ltm_projectors(pairs)."""
    P = projector_tensor(H)
    out = []
    for p, q in pairs:
        if p == q:
            out.append(P[p, p].real)
        else:
            out += [P[p, q].real, P[p, q].imag]
    return np.ascontiguousarray(np.stack(out))


def tensor_of_components(A, pairs, m, index=None):
    """Components A [ncomp, ...] of `pairs` -> P [m, m, ...] complex with P[q, p] = conj(P[p, q]); pairs that are not listed stay
    zero.  `index` maps an orbital of a pair to its position in the m x m block (default: itself)."""
    index = (lambda a: a) if index is None else index
    P = np.zeros((m, m) + A.shape[1:], dtype=np.complex128)
    c = 0
    for p, q in pairs:
        i, j = index(p), index(q)
        if p == q:
            P[i, i] = A[c]
            c += 1
        else:
            P[i, j] = A[c] + 1j * A[c + 1]
            P[j, i] = A[c] - 1j * A[c + 1]
            c += 2
    assert c == len(A)
    return P


def green_matrix(eig, HP, zs):
    """G [nz, m, m] of the eigenvalues eig [npt]*d + [n] and either H [npt]*d + [n, n] (m = n, the projectors come from
    numpy.linalg.eigh) or the projector tensor P [m, m] + [npt]*d + [n] itself (any m; only p <= q is read).  The upper
    triangle's Re P and Im P go through gwltm_numpy.green_weighted as real elements, all in one call, and the matrix is composed
    from the results."""
    eig = np.asarray(eig, dtype=np.float64)
    HP = np.asarray(HP)
    P = projector_tensor(HP) if HP.ndim == eig.ndim + 1 else HP
    assert P.shape[2:] == eig.shape and P.shape[0] == P.shape[1], (P.shape, eig.shape)
    m = P.shape[0]
    pairs = [(p, q) for p in range(m) for q in range(p, m)]
    A = []
    for p, q in pairs:
        A += [P[p, q].real] if p == q else [P[p, q].real, P[p, q].imag]
    g = gw.green_weighted(eig, np.stack(A), zs)
    G = np.empty((g.shape[0], m, m), dtype=np.complex128)
    c = 0
    for p, q in pairs:
        if p == q:
            G[:, p, p] = g[:, c]
            c += 1
        else:
            G[:, p, q] = g[:, c] + 1j * g[:, c + 1]
            G[:, q, p] = g[:, c] - 1j * g[:, c + 1]
            c += 2
    return G
