"""numpy restatement of the occupied pair scans (abz_rule_ltm_pairs_occupied; helper of test_ltm_pairs_occupied_cpu.py /
test_gpu_ltm_pairs_occupied.py, not a conftest).

For every Kuhn simplex of the grid and every pair (v, c) of the ranges, with e_v, e_c, Delta = e_c - e_v and the elements A all
linear inside the simplex,

    g = w sum int_R A delta(w - Delta) dk,     N = w sum int_R A theta(w - Delta) dk,     R = {e_v <= E_F} and {e_c > E_F}.

A GEOMETRIC restatement in the manner of wltm_numpy.py, and deliberately NOT the positive decomposition of the kernel: the region
is formed as a DIFFERENCE of sets, R = {e_v <= E_F} minus {e_c <= E_F} (the second lies inside the first: e_c >= e_v at every
corner, and the interpolants keep the order), and each of the two sets is filled by the barycentric vertex matrices B of
wltm_numpy._pieces -- with its complement "whole simplex minus tip" where that is what _pieces returns.  So a simplex
contributes a SIGNED sum over sub-simplices, each with the corner energies B Delta, the corner elements B A and the volume
fraction |det B|; on every sub-simplex g_A and N_A are evaluated as wltm_numpy does (volume x vertex mean below the energy, the
cone over the cut for the density).  A simplex without an occupied v-corner or without an empty c-corner is left out, so these
cases are exactly 0.  Tie convention: a corner is occupied iff e_v <= E_F and empty iff e_c > E_F.

Sums: blocks of 16 by numpy, the block sums through math.fsum (wltm_numpy.py).
"""
import math

import numpy as np

import wltm_numpy as wn


def _fs(x):
    """column sums of x [K, ncomp]"""
    x = np.asarray(x)
    if len(x) == 0:
        return [0.0] * x.shape[1]
    pad = (-len(x)) % 16
    if pad:
        x = np.concatenate([x, np.zeros((pad, x.shape[1]))])
    blocks = x.reshape(-1, 16, x.shape[1]).sum(axis=1)
    return [math.fsum(col) for col in blocks.T.tolist()]


def _region(f, F):
    """f [S, d+1] corner values -> [(rows, sign, B [K, d+1, d+1])]: signed sub-simplices filling {f <= F}, B in the corner order of f."""
    S, d1 = f.shape
    o = np.argsort(f, axis=1, kind="stable")
    fsorted = np.take_along_axis(f, o, 1)
    m = np.count_nonzero(fsorted <= F, axis=1)
    I = np.eye(d1)
    out = []
    full = np.flatnonzero(m == d1)
    if len(full):
        out.append((full, 1.0, np.broadcast_to(I, (len(full), d1, d1))))
    for mm in range(1, d1):
        sel = np.flatnonzero(m == mm)
        if not len(sel):
            continue
        below, complement, _ = wn._pieces(fsorted[sel], F)
        cols = np.broadcast_to(o[sel][:, None, :], (len(sel), d1, d1))
        for B in below:
            Bo = np.zeros((len(sel), d1, d1))
            np.put_along_axis(Bo, cols, np.asarray(B), axis=2)  # column j of B belongs to corner o[j]
            out.append((sel, -1.0 if complement else 1.0, Bo))
        if complement:
            out.append((sel, 1.0, np.broadcast_to(I, (len(sel), d1, d1))))
    return out


def _sums(e, a, wt, Es):
    """Sub-simplices with corner energies e [S, d+1], corner elements a [S, d+1, ncomp] and signed volumes wt [S] -> (g, N) [nE, ncomp]."""
    d1 = e.shape[1]
    d = d1 - 1
    ncomp = a.shape[2]
    o = np.argsort(e, axis=1, kind="stable")
    e = np.take_along_axis(e, o, 1)
    a = np.take_along_axis(a, o[:, :, None], 1)
    lo, hi = e[:, 0], e[:, -1]
    means = a.mean(axis=1) * wt[:, None]
    g = np.zeros((len(Es), ncomp))
    N = np.zeros((len(Es), ncomp))
    for i, E in enumerate(Es):
        Nc = [[x] for x in _fs(means[hi <= E])]
        gc = [[] for _ in range(ncomp)]
        inside = np.flatnonzero((lo <= E) & (E < hi))
        if len(inside):
            e_in, a_in, w_in = e[inside], a[inside], wt[inside]
            m_in = np.count_nonzero(e_in <= E, axis=1)
            for m in range(1, d1):
                sel = m_in == m
                if not sel.any():
                    continue
                es, as_, ws_ = e_in[sel], a_in[sel], w_in[sel]
                below, complement, cut = wn._pieces(es, E)
                vmean = lambda B: np.einsum("kv,kvc->kc", B.mean(axis=1), as_)
                part = sum(np.abs(np.linalg.det(B))[:, None] * vmean(B) for B in below)
                if complement:
                    part = as_.mean(axis=1) - part
                apex = np.where((E - es[:, 0]) >= (es[:, -1] - E), 0, d)
                e_apex = np.take_along_axis(es, apex[:, None], 1)[:, 0]
                tip = np.eye(d1)[apex][:, None, :]
                dens = sum((d * np.abs(np.linalg.det(np.concatenate([Cm, tip], axis=1))) / np.abs(e_apex - E))[:, None] * vmean(Cm)
                           for Cm in cut)
                for c, col in enumerate(_fs(part * ws_[:, None])):
                    Nc[c].append(col)
                for c, col in enumerate(_fs(dens * ws_[:, None])):
                    gc[c].append(col)
        for c in range(ncomp):
            N[i, c] = math.fsum(Nc[c])
            g[i, c] = math.fsum(gc[c])
    return g, N


def pairs_occ(eig, A, v0, nv, c0, nc, E_F, ws):
    """eig [npt]*d + [n] ascending eigenvalues; A None (A = 1, one component) or [ncomp] + [npt]*d + [nv nc] elements of the pair
    rule (pseudo-band (v - v0) nc + (c - c0)); transition energies ws
    -> (g [nw, ncomp], N [nw, ncomp], census): per unit cell and summed over pairs; census: the set of (occupied v-corners,
    empty c-corners) over all (simplex, pair)."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.ndim - 1
    d1 = d + 1
    ce = wn.corner_sets(eig, d)  # [ns, d+1, n]
    ns = len(ce)
    if A is None:
        cA = np.ones((ns, d1, nv * nc, 1))
    else:
        A = np.asarray(A, dtype=np.float64)
        assert A.shape[1:] == eig.shape[:d] + (nv * nc,), (A.shape, eig.shape)
        cA = wn.corner_sets(np.moveaxis(A, 0, -1), d)  # [ns, d+1, nb, ncomp]
    ncomp = cA.shape[-1]
    ev = np.concatenate([ce[:, :, v0 + p // nc] for p in range(nv * nc)])  # [ns nb, d+1]
    ec = np.concatenate([ce[:, :, c0 + p % nc] for p in range(nv * nc)])
    a = np.concatenate([cA[:, :, p, :] for p in range(nv * nc)])
    dl = ec - ev
    nocc = np.count_nonzero(ev <= E_F, axis=1)
    nemp = np.count_nonzero(ec > E_F, axis=1)
    census = set(zip(nocc.tolist(), nemp.tolist()))
    keep = np.flatnonzero((nocc > 0) & (nemp > 0))
    ev, ec, a, dl = ev[keep], ec[keep], a[keep], dl[keep]
    w = 1.0 / (math.factorial(d) * float(np.prod(eig.shape[:d])))
    ws = np.atleast_1d(np.asarray(ws, dtype=np.float64))
    es, As, wts = [], [], []
    for f, sign0 in ((ev, 1.0), (ec, -1.0)):
        for rows, sign, B in _region(f, E_F):
            es.append(np.einsum("kvj,kj->kv", B, dl[rows]))
            As.append(np.einsum("kvj,kjc->kvc", B, a[rows]))
            wts.append(sign0 * sign * np.abs(np.linalg.det(B)))
    if not es:
        z = np.zeros((len(ws), ncomp))
        return z, z.copy(), census
    g, N = _sums(np.concatenate(es), np.concatenate(As), np.concatenate(wts), ws)
    return g * w, N * w, census
