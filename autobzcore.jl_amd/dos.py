"""Density of states: DOSProblem + GGR + LTM.  ref: src/dos_interfaces.jl, src/dos_algorithms.jl, src/dos_ggr.jl."""
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _lib as L
from .bz import SymmetricBZ
from .series import FourierSeries, PairRule, density_matrix_orbitals, expectation_components, green_node_weight_zs, pair_components, pair_ranges
from .solver import NullParameters, checkkwargs


class DOSAlgorithm:
    pass


class GGR(DOSAlgorithm):
    """Generalized Gilat-Raubenheimer method.  ref: src/dos_algorithms.jl:7-26."""

    def __init__(self, npt=50):
        self.npt = int(npt)


def velocity_operators(h, basis=None):
    """The d operator series O_a = sum_j M[a, j] dH/dkappa_j of the Hamiltonian series `h`, M = `basis` [d, d] or the identity:
    kappa_j = x_j / t_j is the fractional coordinate of variable j (FourierSeries.derivative), so with the identity the band
    expectations <u_b|O_j|u_b> are the rule's velocity planes, v_j = <dH/dx_j> t_j.  The linear combinations are taken on the
    host coefficients; every O_a has the dims, `first` and period of `h` and is Hermitian when `h` is.
    Cartesian velocities: a zone from load_bz(bz, A) holds the reciprocal basis B = 2 pi inv(A)^T, columns b_j (bz.py), and a
    series of period 1 is a function of kappa with k = B kappa.  Then dH/dk_a = sum_j (d kappa_j / d k_a) dH/dkappa_j with
    d kappa_j / d k_a = inv(B)[j, a], so M = inv(B)^T = A / (2 pi) gives O_a = dH/dk_a, the velocity operator in the Cartesian
    direction a in units of (energy x length of A)."""
    if not isinstance(h, FourierSeries):
        raise ValueError("velocity_operators: h is not a FourierSeries")
    d = h.d
    M = np.eye(d) if basis is None else np.asarray(basis, dtype=np.float64)
    if M.shape != (d, d):
        raise ValueError(f"velocity_operators: basis of shape {M.shape}, expected [{d}, {d}]")
    dh = [h.derivative(j) for j in range(d)]
    out = []
    for a in range(d):
        c = sum(M[a, j] * dh[j].c for j in range(d))
        o = FourierSeries(c, period=h.t, first=h.first, ndim=d)
        o.scalar = h.scalar
        out.append(o)
    return out


class BandExpectation:
    """Band expectation values q_i = <u_b(k)| O_i(k) |u_b(k)> of 1..8 operator series in the Wannier basis of H as the
    matrix elements of LTM(elements=BandExpectation(...)), computed on the device (DeviceRule.ltm_expectation).
    `operators`: FourierSeries (or DeviceRule of the cache's grid that hold H planes); `components`: None for the
    expectations in order, or at most 16 entries, each an operator index i (q_i) or a pair (i, j) (the product q_i q_j).
    At a degenerate level only the sum of single expectations over the level is defined."""

    def __init__(self, operators, components=None):
        ops = list(operators) if isinstance(operators, (list, tuple)) else [operators]
        if not 1 <= len(ops) <= L.LTM_EXPECT_MAX_OPS:
            raise ValueError(f"BandExpectation: {len(ops)} operators, 1..{L.LTM_EXPECT_MAX_OPS} are taken")
        self.operators = tuple(ops)
        comps = expectation_components(components, len(ops), "BandExpectation")
        self.components = None if comps is None else tuple((int(i), int(j)) for i, j in comps)


class BandPairs:
    """Pairs of a lower and an upper band as the "bands" of LTM(pairs=BandPairs(...)): the joint density of states
    J(w) = sum_vc int dk delta(w - (e_c - e_v)) and, with operators, the interband spectra
    S_ij(w) = sum_vc int dk M^i_vc conj(M^j_vc) delta(w - (e_c - e_v)), M^i_vc = <u_v|O_i|u_c> (DeviceRule.ltm_pairs).
    Exactly one of `nocc` (the lowest nocc bands against all others: an insulator with nocc filled bands) and `lower` + `upper`
    (each a `range` or (start, count); lower below upper) is given; at most 64 pairs, so a model of many bands takes a window
    around the gap.  `operators`: None (energies only), 1..4 FourierSeries in the Wannier basis of H, or "velocities":
    velocity_operators(H, basis) of the cache's own H with the real parts of all products a <= b as components, in the order of
    velocity_components(d).  `components`: entries i (|M^i|^2), (i, j) (Re M^i conj(M^j)) or (i, j, "re" | "im"); None: |M^i|^2 of
    every operator.  The ranges are whole bands and carry no 1 / w weights; the occupation factors of a metal,
    theta(E_F - e_v) theta(e_c - E_F) inside every simplex, come from `joint_dos` / `interband` with `fermi=` or `nstates=`
    (PairRule.ltm_occupied on the cache's pair rule).  At a degenerate level only the sum of a component over all pairs between
    two levels is defined."""

    def __init__(self, nocc=None, lower=None, upper=None, operators=None, components=None, basis=None):
        if (nocc is None) == (lower is None and upper is None) or (lower is None) != (upper is None):
            raise ValueError("BandPairs: give exactly one of nocc and lower + upper")
        if nocc is not None:
            if not isinstance(nocc, (int, np.integer)) or nocc < 1:
                raise ValueError(f"BandPairs: nocc = {nocc!r} is not a positive number of bands")
            self.nocc, self.ranges = int(nocc), None
        else:
            self.nocc, self.ranges = None, pair_ranges(lower, upper, None, "BandPairs")
        self.basis = basis
        if isinstance(operators, str):
            if operators != "velocities":
                raise ValueError(f"BandPairs: operators = {operators!r} is neither 'velocities', None nor a sequence of FourierSeries")
            if components is not None:
                raise ValueError("BandPairs: operators = 'velocities' brings its own components (the real parts of all products a <= b)")
            self.operators, self.components = "velocities", None
            return
        if basis is not None:
            raise ValueError("BandPairs: basis goes with operators = 'velocities'")
        if operators is None:
            if components is not None:
                raise ValueError("BandPairs: components without operators")
            self.operators, self.components = None, None
            return
        ops = list(operators) if isinstance(operators, (list, tuple)) else [operators]
        if not 1 <= len(ops) <= L.LTM_PAIRS_MAX_OPS:
            raise ValueError(f"BandPairs: {len(ops)} operators, 1..{L.LTM_PAIRS_MAX_OPS} are taken")
        self.operators = tuple(ops)
        comps = pair_components(components, len(ops), "BandPairs")
        self.components = None if comps is None else tuple((int(i), int(j), "im" if part else "re") for i, j, part in comps)

    def resolve(self, h):
        """((v0, nv), (c0, nc), operators, components) for the Hamiltonian series `h`; ValueError when the ranges do not fit its
        bands or make more than 64 pairs."""
        if self.nocc is not None:
            if self.nocc >= h.n:
                raise ValueError(f"BandPairs: nocc = {self.nocc} leaves no upper band of the {h.n} bands")
            v0, nv, c0, nc = pair_ranges((0, self.nocc), (self.nocc, h.n - self.nocc), h.n, "BandPairs")
        else:
            v0, nv, c0, nc = pair_ranges((self.ranges[0], self.ranges[1]), (self.ranges[2], self.ranges[3]), h.n, "BandPairs")
        if isinstance(self.operators, str):
            return (v0, nv), (c0, nc), velocity_operators(h, self.basis), tuple((a, b, "re") for a, b in velocity_components(h.d))
        return (v0, nv), (c0, nc), None if self.operators is None else list(self.operators), self.components


def velocity_components(d):
    """All pairs a <= b of the d directions, in the order (0,0), (0,1), (0,2), (1,1), (1,2), (2,2)."""
    return tuple((a, b) for a in range(d) for b in range(a, d))


class LTM(DOSAlgorithm):
    """Linear tetrahedron method (Bloechl, Jepsen, Andersen, PRB 49, 16223) on the eigenvalues of
    the full periodic `npt^d` grid, cells cut by the Kuhn split.  `cumulative=True` returns the number of states N(E)
    below E instead of the DOS g(E).  The reference plans it: src/dos_algorithms.jl:1-7.

    `elements` weighs every band with a matrix element A_b(k), interpolated linearly inside a simplex like the energy:
    the solution is g_A(E) = sum_b int A_b delta(E - e_b) (or N_A with `cumulative`), `u` of shape [nE, ncomp]
    ([ncomp] for a scalar domain).
      "energy"    A = e itself, one component: E g(E), and the band energy as N_A;
      "orbitals"  the orbital-projected DOS, A_{a,b}(k) = |U_ab(k)|^2, ncomp = n.  With eigenvectors="host" (the default) a
                  host-side companion, not a performance path: the rule is built with H(k) as well, exported, and
                  diagonalised by numpy.linalg.eigh.  With eigenvectors="device" the rule keeps eigenvalues only and the
                  weights are computed on the GPU straight into the resident element block (DeviceRule.ltm_orbitals,
                  1...32 bands, Hermitian series); `orbitals`, a sequence of orbital indices (at most 16, needed above 16
                  bands), then selects the columns of `u`.  At a degenerate level either route weighs with some
                  orthonormal basis of the eigenspace: sums over the level agree, single weights need not;
      callable    f(x [nk, d], eig [nk, n]) -> [ncomp, nk, n] on the rule's exported nodes and eigenvalues;
      BandExpectation(operators, components)
                  band expectation values <u_b|O_i|u_b> of operator series in the Wannier basis of H, and products of two of
                  them, computed on the GPU into the resident element block (DeviceRule.ltm_expectation; 1...32 bands,
                  Hermitian series; the rule keeps eigenvalues only);
      "velocities"  the d fractional velocity operators dH/dkappa_j of the cache's own H (velocity_operators(H), rebuilt with
                  the cache) with all products a <= b as components, in the order (0,0), (0,1), (0,2), (1,1), (1,2), (2,2):
                  `u` [nE, d (d + 1) / 2] is the transport distribution sum_b int dk v_a v_b delta(E - e_b), with
                  `cumulative` its integral, with `eta` the broadened one.  Like "orbitals" both need symmetric=False
                  (expectation values are not invariant) and raise NotImplementedError on a k-sharded series.
    The elements are computed again whenever the cache rebuilds its eigenvalues.

    `symmetric=True` solves the eigenproblem at the irreducible nodes of the zone only and fills the full grid's eigenvalues
    from them on the device (e_b(S k) = e_b(k), DeviceRule.unfold); the tetrahedron sum still runs over the whole grid.  The
    zone's symmetries must be symmetries of H, the contract GGR and PTR have.  With one symmetry (FBZ) it is the plain full
    grid.  "energy" and a callable work as before, at every full-grid node; "orbitals" is refused: |U_ab|^2 is not
    invariant under operations that permute orbitals, and no H(k) is stored.

    `correction=True` (with `cumulative=True` and `elements`) adds Bloechl's curvature correction (eq. 22 of the paper)
    to N_A on every route above.  It removes the leading O(1/npt^2) error of a sum taken at FIXED FILLING, i.e. at the Fermi
    level of the same grid (`fermi_level`, `band_energy`); at a fixed energy the misplaced Fermi surface leaves an error
    of the same order (`optimized=True` below has no such limit).  The plain state count and the DOS have no correction.

    On a k-sharded series (dist.kshard) every rank builds its slab of the grid and the one halo plane behind it
    (DeviceRule.ltm_halo), scans the cells of its slab, and the partial sums are summed over the ranks: `elements` None or
    "energy", with or without `cumulative` and `correction`.  "orbitals", a callable, `symmetric=True` on a symmetric zone,
    `fermi_level` and `band_energy` raise NotImplementedError there.

    `eta > 0` returns the DOS broadened by a Lorentzian of half width eta instead, -Im tr G(E + i eta) / pi at the domain's
    real energies, from the closed-form mean of 1 / (z - e) over every simplex (DeviceRule.ltm_green, `green_trace`).  Its
    error is the interpolation error O(1/npt^2) whatever eta is -- a grid sum of the resolvent needs npt >~ bandwidth / eta --
    and it tends to the plain g(E) linearly in eta.  With `elements` ("energy", "orbitals" or a callable; `eigenvectors`,
    `orbitals` and `symmetric` combine as without `eta`) the solution is the projected DOS broadened by eta,
    -Im G_A(E + i eta) / pi as [nE, ncomp] ([ncomp] for a scalar domain), from the corner weights of every simplex
    (DeviceRule.ltm_green with `elements`, `green_weighted`): with "orbitals" the diagonal G_aa of the local Green's function.
    `cumulative` and `correction` raise ValueError with `eta`, a k-sharded series NotImplementedError.  Without `eta`
    nothing changes.

    `pairs=BandPairs(...)` scans band PAIRS instead of bands: the domain is then the transition energies w, and the solution is
    the joint density of states J(w) or, with operators, the interband spectra `u` [nw, ncomp] (DeviceRule.ltm_pairs: the pair
    energies e_c - e_v are the eigenvalue planes of a rule of their own, the interband products its attached elements).
    `cumulative`, `correction` and `eta` keep their meaning on the pair rule; with `eta` the solution is complex,
    sum_vc int dk M M^* / (w + i eta - (e_c - e_v)): -Im / pi is the broadened spectrum, Re its Kramers-Kronig partner.
    `correction` needs operators.  Refused when the cache is made: `pairs` with `elements`; `pairs` with operators and
    symmetric=True (matrix elements are not invariant; without operators symmetric=True gives the JDOS from irreducible
    nodes); a k-sharded series (NotImplementedError); more than 64 pairs.

    `optimized=True` (d = 3) scans with the optimized tetrahedron method of Kawamura, Gohda and Tsuneyuki, PRB 89, 094515
    (2014) instead (DeviceRule.ltm_optimized): every simplex takes the band, and the elements, at its 4 corners and at 16
    neighbouring grid points, and the closed forms run on the corner values of the linear function closest to the cubic
    through the 20 values.  Same eigenvalues, no further eigen-solve; the error falls like a higher power of 1/npt at ANY
    energy, for the DOS, `cumulative`, and `elements` "energy", "orbitals", a callable or a BandExpectation, with or without
    `symmetric` -- the rule at npt compares with the linear rule at 2 npt.  It replaces the curvature correction:
    `correction`, `eta` and `pairs` raise ValueError with it; a k-sharded series and d < 3 raise NotImplementedError when
    the cache is made.  `fermi_level` and `band_energy` follow the cache's rule."""

    def __init__(self, npt=50, cumulative=False, elements=None, symmetric=False, eigenvectors="host", orbitals=None,
                 correction=False, eta=None, pairs=None, optimized=False):
        self.npt = int(npt)
        self.optimized = bool(optimized)
        if self.optimized and correction:
            raise ValueError("LTM: optimized=True replaces the curvature correction: it does not go with correction=True")
        if self.optimized and eta is not None:
            raise ValueError("LTM: optimized=True does not go with eta (the solve path with eta is the linear rule's; the optimized Green's "
                             "functions: dos.green_trace / dos.green_weighted with optimized=True, DeviceRule.ltm_green_optimized)")
        if self.optimized and pairs is not None:
            raise ValueError("LTM: optimized=True does not go with pairs (pair rules are scanned with the linear rule)")
        if pairs is not None and not isinstance(pairs, BandPairs):
            raise ValueError(f"LTM: pairs = {pairs!r} is not a BandPairs")
        self.pairs = pairs
        if eta is not None:
            eta = float(eta)
            if not (np.isfinite(eta) and eta > 0.0):
                raise ValueError(f"LTM: eta = {eta!r} is not a positive finite broadening")
            if cumulative or correction:
                raise ValueError("LTM: eta gives the broadened DOS -Im G(E + i eta) / pi: it does not go with cumulative or correction")
        self.eta = eta
        self.cumulative = bool(cumulative)
        self.symmetric = bool(symmetric)
        if not (elements is None or isinstance(elements, BandExpectation) or callable(elements)
                or (isinstance(elements, str) and elements in ("energy", "orbitals", "velocities"))):
            raise ValueError(f"LTM: elements = {elements!r} is neither 'energy', 'orbitals', 'velocities', a BandExpectation nor a callable")
        self.elements = elements
        self.correction = bool(correction)
        if self.correction and not self.cumulative:
            raise ValueError("LTM: correction=True corrects the state sum N_A: it needs cumulative=True (the DOS has no correction)")
        if self.correction and elements is None and not (pairs is not None and pairs.operators is not None):
            raise ValueError("LTM: correction=True needs elements (the correction of the unweighted state count is zero)")
        if not (isinstance(eigenvectors, str) and eigenvectors in ("host", "device")):
            raise ValueError(f"LTM: eigenvectors = {eigenvectors!r} is neither 'host' nor 'device'")
        device = eigenvectors == "device"
        if device and not (isinstance(elements, str) and elements == "orbitals"):
            raise ValueError('LTM: eigenvectors = "device" computes orbital weights: it needs elements = "orbitals"')
        if orbitals is not None:
            if not device:
                raise ValueError('LTM: a selection of orbitals needs elements = "orbitals" with eigenvectors = "device"')
            sel = np.asarray(orbitals).reshape(-1)
            if sel.size < 1 or not np.issubdtype(sel.dtype, np.integer):
                raise ValueError(f"LTM: orbitals = {orbitals!r} is not a sequence of orbital indices")
            orbitals = tuple(int(a) for a in sel)
        self.eigenvectors = eigenvectors
        self.orbitals = orbitals


@dataclass
class DOSProblem:
    """ref: src/dos_interfaces.jl:33-38."""
    H: Any
    domain: Any
    p: Any = None


@dataclass
class DOSSolution:
    u: Any
    err: Any
    retcode: bool
    numevals: int


class DOSCache:
    """Mutable cache; assigning `H` marks it fresh so the eigen-data are rebuilt on the next solve.
    ref: src/dos_interfaces.jl:49-64."""

    def __init__(self, H, domain, p, alg, cacheval, kwargs):
        object.__setattr__(self, "H", H)
        self.domain, self.p, self.alg, self.cacheval, self.kwargs = domain, p, alg, cacheval, kwargs
        self.isfresh = False
        self.elements = _ltm_elements(cacheval, alg)

    def __setattr__(self, name, value):
        if name == "H":
            object.__setattr__(self, "isfresh", True)
        object.__setattr__(self, name, value)


def _pair_rule(h, p, alg, prev):
    """The pair rule of an LTM(pairs=...) cache: made from the source rule the cache would scan without `pairs` (kept by the pair
    rule as its `source`), or `prev`, the cache's pair rule so far, filled again from the series' current coefficients."""
    pairs = alg.pairs
    if alg.elements is not None:
        raise ValueError("LTM: pairs and elements do not go together (the elements of a pair rule are its interband products)")
    symmetric = alg.symmetric and p.syms is not None and len(p.syms) > 1
    if pairs.operators is not None and alg.symmetric:
        raise ValueError("LTM: pairs with operators need symmetric=False (interband matrix elements are not invariant under the "
                         "zone's symmetries, and an unfolded rule stores no H(k))")
    lower, upper, ops, comps = pairs.resolve(h)
    if any(_ksharded(dev) for dev in h._dev.values()):  # (the copies the series has: no device is asked for the refusal)
        raise NotImplementedError("LTM(pairs=...) on a k-sharded series is not implemented: a pair rule is made from a whole grid")
    h.invalidate()  # coefficients may have been mutated in place: re-upload, rules refill lazily
    dev = h.device()
    if isinstance(prev, PairRule) and not prev._closed:
        if prev.dev is dev and prev.npt == alg.npt and (prev.lower, prev.upper) == (range(lower[0], sum(lower)), range(upper[0], sum(upper))):
            prev.operators = [] if ops is None else list(ops)  # ("velocities": those of the Hamiltonian the cache holds now)
            prev.refill()
            return prev
        prev.close()  # another series, grid or ranges: its energies and elements leave the device now, not with the collector
    src = dev.rule(alg.npt, p.syms, L.WANT_EIG).unfold() if symmetric else dev.rule(alg.npt, None, L.WANT_EIG)
    return src.ltm_pairs(lower, upper, ops, comps)


def _init_cacheval(h, domain, p, alg, prev=None):
    """get_ggr_data on the GPU: eigenvalues + band velocities at every (irreducible) PTR node stay
    resident in HBM.  ref: src/dos_ggr.jl:1-44."""
    if not isinstance(alg, (GGR, LTM)):
        return None
    name = type(alg).__name__
    if not isinstance(h, FourierSeries):
        raise ValueError(f"{name} currently supports Fourier series Hamiltonians")
    if not isinstance(p, SymmetricBZ):
        raise ValueError(f"{name} supports BZ parameters from load_bz")
    if p.ndim != h.d:
        raise ValueError(f"{name}: BZ and series dimensions differ")
    if isinstance(alg, LTM) and alg.symmetric and isinstance(alg.elements, str) and alg.elements == "orbitals":
        raise ValueError('LTM: elements = "orbitals" needs symmetric=False (orbital weights are not invariant under the zone\'s '
                         "symmetries, and an unfolded rule stores no H(k))")
    if isinstance(alg, LTM) and alg.symmetric and _is_expectation(alg.elements) and p.syms is not None and len(p.syms) > 1:
        raise ValueError("LTM: band expectation values (elements = 'velocities' or a BandExpectation) need symmetric=False (they "
                         "are not invariant under the zone's symmetries, and an unfolded rule stores no H(k))")
    if isinstance(alg, LTM) and alg.pairs is not None:
        return _pair_rule(h, p, alg, prev)
    if isinstance(alg, LTM) and alg.optimized and h.d != 3:
        raise NotImplementedError(f"LTM(optimized=True) is implemented for d = 3 (the series has d = {h.d})")
    h.invalidate()  # coefficients may have been mutated in place (test/dos.jl:123): re-upload, rules refill lazily
    if isinstance(alg, LTM) and alg.optimized and _ksharded(h.device()):
        raise NotImplementedError("LTM(optimized=True) on a k-sharded series is not implemented: the 20-point stencil of a simplex "
                                  "needs three halo planes")
    if isinstance(alg, LTM) and alg.eta is not None and _ksharded(h.device()):
        raise NotImplementedError("LTM(eta=...) on a k-sharded series is not implemented: the trace of the Green's function is "
                                  "computed on whole grids")
    if isinstance(alg, LTM) and _ksharded(h.device()):
        # slabs of the full grid, each with its halo plane; what needs more than a sum of partial scans is refused here
        if alg.elements is not None and not (isinstance(alg.elements, str) and alg.elements == "energy"):
            raise NotImplementedError('LTM on a k-sharded series: elements = "orbitals" or a callable are not implemented (a slab '
                                      'scans elements None or "energy")')
        if alg.symmetric and p.syms is not None and len(p.syms) > 1:
            raise NotImplementedError("LTM on a k-sharded series: symmetric=True on a symmetric zone is not implemented (no "
                                      "unfolding into a slab)")
        rule = h.device().rule(alg.npt, None, L.WANT_EIG)
        rule.ltm_halo()
        return rule
    if isinstance(alg, LTM) and alg.symmetric and p.syms is not None and len(p.syms) > 1:
        # eigensolves at the irreducible nodes only; the full grid's eigenvalue planes are a gather from them
        return h.device().rule(alg.npt, p.syms, L.WANT_EIG).unfold()
    if isinstance(alg, LTM):
        # eigenvalues only, on the FULL grid whatever the zone's symmetries: the DOS is a scalar, so the full-zone sum is the
        # answer for every zone kind (symmetric=True above fills the same grid from the irreducible nodes; a symmetry-
        # reduced tetrahedron MESH is not implemented)
        host_vectors = isinstance(alg.elements, str) and alg.elements == "orbitals" and alg.eigenvectors == "host"  # numpy diagonalises the exported H(k)
        return h.device().rule(alg.npt, None, (L.WANT_H | L.WANT_EIG) if host_vectors else L.WANT_EIG)
    return h.device().rule(alg.npt, p.syms, L.WANT_EIG | L.WANT_VEL)


def _ksharded(dev):
    return bool(dev.kshard and dev.kshard[1] > 1)


class _DeviceOrbitals:
    """Orbital weights the rule computes itself (DeviceRule.ltm_orbitals); one object per refresh of a cache: the owner mark."""

    def __init__(self, orbitals):
        self.orbitals = orbitals


def _is_expectation(elements):
    return isinstance(elements, BandExpectation) or (isinstance(elements, str) and elements == "velocities")


class _DeviceExpectation:
    """Band expectation values the rule computes itself (DeviceRule.ltm_expectation); one object per refresh of a cache: the
    owner mark, and the operator series made from the Hamiltonian the cache held at that refresh."""

    def __init__(self, operators, components):
        self.operators, self.components = operators, components


def _ltm_elements(rule, alg):
    """What an LTM cache hands DeviceRule.ltm as `elements`: None, "energy", the host array [ncomp, nk, n] computed
    from the rule's current values, or the request for orbital weights made on the device."""
    if isinstance(alg, LTM) and alg.pairs is not None and rule is not None:
        return None if alg.pairs.operators is None else "attached"  # (the pair rule made them itself)
    if not isinstance(alg, LTM) or alg.elements is None or rule is None:
        return None
    if isinstance(alg.elements, BandExpectation):
        return _DeviceExpectation(alg.elements.operators, alg.elements.components)
    if isinstance(alg.elements, str) and alg.elements == "velocities":
        return _DeviceExpectation(tuple(velocity_operators(rule.dev.s)), velocity_components(rule.dev.s.d))
    if alg.elements == "energy":
        return "energy"
    if alg.elements == "orbitals" and alg.eigenvectors == "device":
        return _DeviceOrbitals(alg.orbitals)
    if alg.elements == "orbitals":
        ex = rule.export(x=False, w=False, H=True)
        H = ex["H"]
        if H.ndim == 1:  # scalar series
            return np.ones((1, len(H), 1))
        _, U = np.linalg.eigh(H)  # ascending, the order of the rule's eigenvalue planes
        return np.ascontiguousarray((np.abs(U) ** 2).transpose(1, 0, 2))  # [a, k, b]
    ex = rule.export(x=True, w=False, eig=True)
    A = np.asarray(alg.elements(ex["x"], ex["eig"]), dtype=np.float64)
    if A.ndim == 2:
        A = A[None]
    if A.ndim != 3 or A.shape[1:] != ex["eig"].shape:
        raise ValueError(f"LTM: elements(x, eig) returned shape {A.shape}, expected [ncomp, {ex['eig'].shape[0]}, {ex['eig'].shape[1]}]")
    return np.ascontiguousarray(A)


def _ltm_attach(rule, el):
    """The cache's elements `el` (an array, a _DeviceOrbitals or a _DeviceExpectation) attached to its rule, unless they still are."""
    rule.h  # a stale rule refills here and loses its elements
    if rule._ltm_ncomp == 0 or getattr(rule, "_ltm_owner", None) is not el:  # (another cache on the same rule attached its own)
        if isinstance(el, _DeviceOrbitals):
            rule.ltm_orbitals(el.orbitals)
        elif isinstance(el, _DeviceExpectation):
            rule.ltm_expectation(list(el.operators), el.components)
        else:
            rule.ltm_elements(el)
        rule._ltm_owner = el


def _ltm_solve(c, Es):
    rule, el = c.cacheval, c.elements
    if c.alg.eta is not None and c.alg.pairs is not None:  # the broadened spectrum (-Im / pi) with its Kramers-Kronig partner (Re)
        return rule.ltm_green(Es + 1j * c.alg.eta, elements=el)
    if c.alg.eta is not None:
        zs = Es + 1j * c.alg.eta
        if el is None:
            return -rule.ltm_green(zs).imag / np.pi
        if not isinstance(el, str):
            _ltm_attach(rule, el)
        return -rule.ltm_green(zs, elements=el if isinstance(el, str) else "attached").imag / np.pi
    if not (el is None or isinstance(el, str)):
        _ltm_attach(rule, el)
        el = "attached"
    if c.alg.optimized:
        return rule.ltm_optimized(Es, states=c.alg.cumulative, elements=el)
    return rule.ltm(Es, states=c.alg.cumulative, elements=el, correction=c.alg.correction)


def _refresh(c):
    """A cache whose H was assigned builds its eigen-data again (a pair rule is filled again in place) before its next use."""
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg, c.cacheval)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False


def init(prob: DOSProblem, alg: DOSAlgorithm, **kwargs):
    """ref: src/dos_interfaces.jl:82-86."""
    checkkwargs(kwargs)
    return DOSCache(prob.H, prob.domain, prob.p, alg, _init_cacheval(prob.H, prob.domain, prob.p, alg), kwargs)


def solve_(c: DOSCache):
    """solve!(cache).  ref: src/dos_interfaces.jl:104-112, dos_solve src/dos_ggr.jl:46-56."""
    _refresh(c)
    if not isinstance(c.alg, (GGR, LTM)):
        raise ValueError("unknown DOS algorithm")
    scalar = np.ndim(c.domain) == 0
    if not scalar and not isinstance(c.domain, (list, tuple, np.ndarray)):
        raise ValueError(f"{type(c.alg).__name__} supports domains of individual eigenvalues")
    Es = np.atleast_1d(np.asarray(c.domain, dtype=np.float64))
    u = _ltm_solve(c, Es) if isinstance(c.alg, LTM) else c.cacheval.ggr(Es)
    if u.ndim == 2:
        return DOSSolution(u[0].copy() if scalar else u, None, True, -1)
    return DOSSolution(u[0].item() if scalar else u, None, True, -1)


def fermi_level(prob_or_cache, nstates, tol=1e-10, optimized=None):
    """(E_F, N(E_F)) of `nstates` states per unit cell (0 < nstates < n) from the eigenvalues of an LTM cache, or of a
    DOSProblem (solved with LTM()): E_F is the upper end of an interval no wider than `tol` that N crosses `nstates` in.
    `optimized`: True for the level of the optimized tetrahedron rule's state count (DeviceRule.ltm_fermi_optimized, d = 3:
    a host search over device scans, the same contract), False for the linear rule's, None (the default) for the rule of
    the cache's algorithm, LTM(optimized=...)."""
    H = getattr(prob_or_cache, "H", None)
    if isinstance(H, FourierSeries) and _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
        raise NotImplementedError("fermi_level / band_energy on a k-sharded series are not implemented: the search for the level "
                                  "needs an all-reduce inside it")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    if not isinstance(c.alg, LTM):
        raise ValueError("fermi_level needs an LTM cache")
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    if c.alg.optimized if optimized is None else optimized:
        return c.cacheval.ltm_fermi_optimized(nstates, tol)
    return c.cacheval.ltm_fermi(nstates, tol)


def green_trace(prob_or_cache, zs, optimized=False):
    """tr G(z) = sum_b int dk / (z - e_b(k)) at the complex energies `zs` (Im z != 0), per unit cell, complex128 [nz], from the
    eigenvalues of an LTM cache or of a DOSProblem (solved with LTM()): DeviceRule.ltm_green on the cache's grid.
    `optimized=True`: the optimized tetrahedron rule instead (DeviceRule.ltm_green_optimized, d = 3), whose -Im / pi tends to the
    DOS of LTM(optimized=True) as Im z -> 0.  The default is the linear rule whatever the cache's algorithm is; the solve path
    LTM(eta=...) stays linear too (LTM(optimized=True, eta=...) is refused): this keyword is the way to the optimized trace."""
    H = getattr(prob_or_cache, "H", None)
    if isinstance(H, FourierSeries) and _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
        raise NotImplementedError("green_trace on a k-sharded series is not implemented: the trace of the Green's function is "
                                  "computed on whole grids")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    if not isinstance(c.alg, LTM):
        raise ValueError("green_trace needs an LTM cache")
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    if optimized:
        return c.cacheval.ltm_green_optimized(zs)
    return c.cacheval.ltm_green(zs)


def green_weighted(prob_or_cache, zs, optimized=False):
    """G_A(z) = sum_b int dk A_b(k) / (z - e_b(k)) at the complex energies `zs` (Im z != 0), per unit cell, complex128
    [nz, ncomp], with the elements of an LTM cache (`elements` = "energy", "orbitals" or a callable) or of a DOSProblem
    (solved with LTM(elements="energy")): DeviceRule.ltm_green with the cache's elements on the cache's grid.  With orbital
    weights it is the diagonal G_aa(z) of the local Green's function.  `optimized=True`: the optimized tetrahedron rule instead
    (DeviceRule.ltm_green_optimized, d = 3: elements and energies take the same 20-point fit per simplex).  The default is the
    linear rule whatever the cache's algorithm is, and the solve path LTM(eta=...) stays linear (LTM(optimized=True, eta=...)
    is refused): this keyword is the way to the optimized G_A."""
    H = getattr(prob_or_cache, "H", None)
    if isinstance(H, FourierSeries) and _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
        raise NotImplementedError("green_weighted on a k-sharded series is not implemented: the Green's function is computed on "
                                  "whole grids")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM(elements="energy"))
    if not isinstance(c.alg, LTM):
        raise ValueError("green_weighted needs an LTM cache")
    if c.alg.elements is None:
        raise ValueError("green_weighted needs an LTM cache with elements (green_trace gives the trace)")
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    el = c.elements
    if not isinstance(el, str):
        _ltm_attach(c.cacheval, el)
    green = c.cacheval.ltm_green_optimized if optimized else c.cacheval.ltm_green
    return green(zs, elements=el if isinstance(el, str) else "attached")


def _green_local_check(c, who):
    if not isinstance(c.alg, LTM):
        raise ValueError(f"{who} needs an LTM cache")
    if c.alg.symmetric and c.p.syms is not None and len(c.p.syms) > 1:
        raise ValueError(f"{who} needs symmetric=False (band projectors are not invariant under the zone's symmetries, and "
                         "an unfolded rule stores no H(k))")


def _green_local(prob_or_cache, zs, orbitals, fused, optimized=False):
    who = "green_local_fused" if fused else "green_local"
    if fused and isinstance(prob_or_cache, DOSCache):  # (a cache says what it is without its series' device being asked)
        _green_local_check(prob_or_cache, who)
    H = getattr(prob_or_cache, "H", None)
    if optimized and isinstance(H, FourierSeries) and H.d != 3:  # (before a device is asked for anything)
        raise NotImplementedError(f"{who}: optimized=True is implemented for d = 3 (the series has d = {H.d})")
    if isinstance(H, FourierSeries) and _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
        raise NotImplementedError(f"{who} on a k-sharded series is not implemented: the Green's function is computed on "
                                  "whole grids")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    _green_local_check(c, who)
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    if fused:
        return c.cacheval.ltm_green_node_weights_matrix(zs, orbitals, optimized=bool(optimized))
    return c.cacheval.ltm_green_matrix(zs, orbitals)


def green_local(prob_or_cache, zs, orbitals=None):
    """The local Green's function G_pq(z) = [int dk inv(z - H(k))]_pq on the orbitals `orbitals` (None: all n) at the complex
    energies `zs` (Im z != 0), per unit cell, complex128 [nz, m, m], on the grid of an LTM cache or of a DOSProblem (solved
    with LTM()): DeviceRule.ltm_green_matrix, the band projectors U_pb conj(U_qb) as elements of the tetrahedron method.  Its
    diagonal is `green_weighted` with orbital weights, its trace `green_trace`.  The cache's own elements are attached again by
    its next solve.
    `green_local_fused` computes the same matrix from the complex node weights W_b(k; z) and U(k) without attaching projectors.
    Crossover (measured on an MI355X, profiles/ltm_green_node_weights.txt): none in the number of z.  With ONE projector group of
    16 components (up to 4 orbitals) the two routes are close, `green_local_fused` 1.25 times faster at one z and 1.05 times at 8
    and 64 values (3 bands 48^3); with more groups it is faster at every number of z, 16...26 times for 16 bands (16 groups, 24^3)
    and 27...55 times for 32 bands (64 groups, 16^3).  What this route keeps: it needs no weight block of 16 nz n bytes per node."""
    return _green_local(prob_or_cache, zs, orbitals, False)


def green_local_fused(prob_or_cache, zs, orbitals=None, optimized=False):
    """`green_local` by the other route (DeviceRule.ltm_green_node_weights_matrix): the complex integration weights W_b(k; z)
    are gathered per node, 8 values of z at a time, and contracted with the eigenvectors by the kernel of `density_matrix`;
    no projector is attached and the cache's elements stay as they are.  Same solver, same basis, same arguments and refusals;
    the two routes agree to rounding, not to the bit.
    Cost: `green_local` repeats the eigen-solve of the grid and a scan of the simplices once per group of 16 projector
    components (1 group up to 4 orbitals, 16 for 16, 64 for 32); this route gathers the weights once per z ((d+1) times the
    simplices of a scan, one series per simplex where it is narrow) and solves the grid once per 4 weight sets for 1...4 bands,
    twice per z for 5...32 bands.  Measured (profiles/ltm_green_node_weights.txt): 1.25 times faster than `green_local` for 3
    bands at one z and 1.05 times at 8 and 64; 16...26 times faster for 16 bands and 27...55 times for 32 bands at 64...1 values.
    It holds a weight block of 16 nz n bytes per node (8 values at a time) that `green_local` does not need.
    `optimized=True` (d = 3): the weights of the optimized tetrahedron rule instead
    (DeviceRule.ltm_green_node_weights_optimized): tr G_pq(z) is then `green_trace(cache, zs, optimized=True)` and -Im G_pp / pi
    tends to the projected DOS of LTM(optimized=True) as Im z -> 0.  The default is the linear rule whatever the cache's algorithm
    is (the convention of `green_trace`); d < 3 and a k-sharded series raise NotImplementedError.  `green_local` has no such
    keyword: its scan route serves the linear rule."""
    return _green_local(prob_or_cache, zs, orbitals, True, optimized)


def green_weights(prob_or_cache, zs, fold=False, optimized=False):
    """(W, zs): the complex integration weights W_b(k; z) of the Green's function on the grid of an LTM cache, or of a DOSProblem
    (solved with LTM()), and the values of z they belong to: G_A(z) = sum_k sum_b W_b(k; z) A_b(k) for ANY A, complex or
    matrix-valued (DeviceRule.ltm_green_node_weights).  At most 8 values, Im z != 0; W is complex128 [nz, nk, n], [nk, n] for a
    scalar z.  Nodes and bands are ordered like the eigenvalues of the cache's rule (`cache.cacheval.export(eig=True)`).  With
    `LTM(symmetric=True)` on a symmetric zone and `fold=True` the weights come back summed over orbits on the irreducible nodes
    that were solved, [.., nirr, n] in the order of `cache.cacheval.source.export(eig=True)`: G_loc(z) is then a sum over
    those nodes followed by the caller's own symmetrisation; anywhere else `fold=True` raises ValueError.
    `optimized=True` (d = 3): the weights of the optimized tetrahedron rule instead (DeviceRule.ltm_green_node_weights_optimized):
    sum_k sum_b W A is the G_A(z) of `green_weighted(..., optimized=True)` for any A and sum W is `green_trace(..., optimized=True)`.
    The default is the linear rule whatever the cache's algorithm is (the convention of `green_trace`); d < 3 and a k-sharded
    series raise NotImplementedError."""
    scalar = np.ndim(zs) == 0
    zs = green_node_weight_zs(zs, "green_weights")

    def check(alg, p):
        if not isinstance(alg, LTM):
            raise ValueError("green_weights needs an LTM cache")
        if fold and not (alg.symmetric and getattr(p, "syms", None) is not None and len(p.syms) > 1):
            raise ValueError("green_weights: fold=True needs an LTM(symmetric=True) cache on a symmetric zone (nothing was unfolded)")

    # (a cache says what it is, and a problem is solved with LTM(), without the series' device being asked)
    if isinstance(prob_or_cache, DOSCache):
        check(prob_or_cache.alg, prob_or_cache.p)
    else:
        check(LTM(), getattr(prob_or_cache, "p", None))
    H = getattr(prob_or_cache, "H", None)
    if optimized and isinstance(H, FourierSeries) and H.d != 3:  # (before a device is asked for anything)
        raise NotImplementedError(f"green_weights: optimized=True is implemented for d = 3 (the series has d = {H.d})")
    if isinstance(H, FourierSeries) and _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
        raise NotImplementedError("green_weights on a k-sharded series is not implemented: a node's weight needs its whole "
                                  "neighbourhood, which a slab with its halo plane does not hold")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    rule = c.cacheval
    W = (rule.ltm_green_node_weights_optimized if optimized else rule.ltm_green_node_weights)(zs, export=not fold)
    if fold:
        W = rule.ltm_green_node_weights_fold()
    return (W[0], complex(zs[0])) if scalar else (W, zs)


def band_energy(prob_or_cache, nstates, tol=1e-10, correction=True):
    """(E_band, E_F): the band energy sum_b int e_b theta(E_F - e_b) of `nstates` states per unit cell.  E_F is
    `fermi_level`'s on the same grid; one single-energy scan with the energy as the element follows, with Bloechl's
    curvature correction unless `correction=False`.  The correction is made for exactly this use -- a sum at the grid's own
    Fermi level: it removes the leading O(1/npt^2) error of the linear interpolation.  On a cache of LTM(optimized=True) the
    level and the scan are those of the optimized rule, which takes no correction (`correction` is not read)."""
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    E_F, _ = fermi_level(c, nstates, tol)
    if c.alg.optimized:
        return float(c.cacheval.ltm_optimized(np.array([E_F]), states=True, elements="energy")[0, 0]), E_F
    u = c.cacheval.ltm(np.array([E_F]), states=True, elements="energy", correction=bool(correction))
    return float(u[0, 0]), E_F


def integration_weights(prob_or_cache, E=None, nstates=None, kind="states", correction=False, fold=False, optimized=False):
    """(W, E): Bloechl's integration weights w_b(k; E) of the grid of an LTM cache, or of a DOSProblem (solved with LTM()), and
    the energies they belong to.  Exactly one of `E` (at most 16 energies; W is [nE, nk, n], [nk, n] for a scalar) and `nstates`
    (W [nk, n] at `fermi_level`'s energy on the same rule: the occupations of that filling) is given.  `kind`: "states"
    (sum_k sum_b W A = N_A) or "dos" (= g_A); `correction=True` (with "states") adds Bloechl's curvature correction, made for
    sums at the grid's own Fermi level.  Nodes and bands are ordered like the eigenvalues of the cache's rule
    (`cache.cacheval.export(eig=True)`).  With `LTM(symmetric=True)` on a symmetric zone and `fold=True` the weights come back
    summed over orbits on the irreducible nodes that were solved, [.., nirr, n] in the order of
    `cache.cacheval.source.export(eig=True)`; anywhere else `fold=True` raises ValueError.
    `optimized=True` (d = 3): the weights of the optimized tetrahedron rule instead (DeviceRule.ltm_node_weights_optimized):
    sum_k sum_b W A is the N_A / g_A of LTM(optimized=True) for any A, and with `nstates` the level is
    `fermi_level(cache, nstates, optimized=True)`, so the occupations sum to `nstates`.  These weights are not confined to
    [0, 1 / nk]: a node next to the Fermi surface can weigh negative.  It does not go with `correction` (ValueError); d < 3 and a
    k-sharded series raise NotImplementedError.  The default is the linear rule whatever the cache's algorithm is (the
    convention of `green_trace`): on an LTM(optimized=True) cache with `nstates` the default takes that cache's optimized level
    and returns linear weights there, which do not sum to `nstates`."""
    if (E is None) == (nstates is None):
        raise ValueError("integration_weights: give exactly one of E and nstates")
    if optimized and correction:
        raise ValueError("integration_weights: optimized=True replaces the curvature correction: it does not go with correction=True")
    if kind not in ("states", "dos"):
        raise ValueError(f"integration_weights: kind = {kind!r} is neither 'states' nor 'dos'")
    if correction and kind != "states":
        raise ValueError("integration_weights: correction=True corrects the state sum: it needs kind='states' (the DOS has no correction)")
    H = getattr(prob_or_cache, "H", None)
    if optimized and isinstance(H, FourierSeries) and H.d != 3:  # (before a device is asked for anything)
        raise NotImplementedError(f"integration_weights: optimized=True is implemented for d = 3 (the series has d = {H.d})")
    if isinstance(H, FourierSeries) and _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
        raise NotImplementedError("integration_weights on a k-sharded series is not implemented: a node's weight needs its whole "
                                  "neighbourhood, which a slab with its halo plane does not hold")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    if not isinstance(c.alg, LTM):
        raise ValueError("integration_weights needs an LTM cache")
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    rule = c.cacheval
    if fold and not hasattr(rule, "ltm_node_weights_fold"):
        raise ValueError("integration_weights: fold=True needs an LTM(symmetric=True) cache on a symmetric zone (nothing was unfolded)")
    scalar = nstates is not None or np.ndim(E) == 0
    if nstates is not None:
        Es = np.array([(fermi_level(c, nstates, optimized=True) if optimized else fermi_level(c, nstates))[0]])
    else:
        Es = np.atleast_1d(np.asarray(E, dtype=np.float64)).reshape(-1)
    if optimized:
        W = rule.ltm_node_weights_optimized(Es, states=kind == "states", export=not fold)
    else:
        W = rule.ltm_node_weights(Es, states=kind == "states", correction=bool(correction), export=not fold)
    if fold:
        W = rule.ltm_node_weights_fold()
    return (W[0], float(Es[0])) if scalar else (W, Es)


def density_matrix(prob_or_cache, E=None, nstates=None, kind="states", correction=False, orbitals=None, optimized=False):
    """(rho, E): the density matrix rho_pq(E) = sum_k sum_b w_b(k; E) U_pb(k) conj(U_qb(k)) in the orbital basis, per unit cell,
    on the grid of an LTM cache or of a DOSProblem (solved with LTM()), and the energies it belongs to
    (DeviceRule.ltm_density_matrix: Bloechl's weights contracted with the eigenvectors inside one eigen-solve of the grid).
    Exactly one of `E` (at most 16 energies; rho is complex128 [nE, m, m], [m, m] for a scalar) and `nstates` (rho [m, m] at
    `fermi_level`'s energy on the same rule: the occupation matrix of that filling, tr rho = nstates) is given.  `kind`:
    "states" (occupations) or "dos" (the spectral-density matrix, tr rho = g(E)); `correction=True` (with "states") adds
    Bloechl's curvature correction.  `orbitals` (None: all n) selects the sub-block.  The cache's attached elements stay as
    they are; the rule's resident integration weights are replaced by those of E.
    `optimized=True` (d = 3): the weights of the optimized tetrahedron rule instead (DeviceRule.ltm_node_weights_optimized), and
    with `nstates` the level of `fermi_level(cache, nstates, optimized=True)`: tr rho = nstates on that rule.  It does not go with
    `correction` (ValueError); d < 3 and a k-sharded series raise NotImplementedError.  The default is the linear rule whatever the
    cache's algorithm is."""
    if (E is None) == (nstates is None):
        raise ValueError("density_matrix: give exactly one of E and nstates")
    if optimized and correction:
        raise ValueError("density_matrix: optimized=True replaces the curvature correction: it does not go with correction=True")
    if kind not in ("states", "dos"):
        raise ValueError(f"density_matrix: kind = {kind!r} is neither 'states' nor 'dos'")
    if correction and kind != "states":
        raise ValueError("density_matrix: correction=True corrects the state sum: it needs kind='states' (the DOS has no correction)")
    H = getattr(prob_or_cache, "H", None)
    if isinstance(H, FourierSeries):
        density_matrix_orbitals(orbitals, H.n, "density_matrix")
        if optimized and H.d != 3:  # (before a device is asked for anything)
            raise NotImplementedError(f"density_matrix: optimized=True is implemented for d = 3 (the series has d = {H.d})")
        if _ksharded(H.device()):  # (before a cache is made: nothing is built for the refusal)
            raise NotImplementedError("density_matrix on a k-sharded series is not implemented: a node's weight needs its whole "
                                      "neighbourhood, which a slab with its halo plane does not hold")
    c = prob_or_cache if isinstance(prob_or_cache, DOSCache) else init(prob_or_cache, LTM())
    if not isinstance(c.alg, LTM):
        raise ValueError("density_matrix needs an LTM cache")
    if c.alg.symmetric and c.p.syms is not None and len(c.p.syms) > 1:
        raise ValueError("density_matrix needs symmetric=False (band projectors are not invariant under the zone's symmetries, and "
                         "an unfolded rule stores no H(k))")
    if c.isfresh:
        c.cacheval = _init_cacheval(c.H, c.domain, c.p, c.alg)
        c.elements = _ltm_elements(c.cacheval, c.alg)
        c.isfresh = False
    scalar = nstates is not None or np.ndim(E) == 0
    if nstates is not None:
        Es = np.array([(fermi_level(c, nstates, optimized=True) if optimized else fermi_level(c, nstates))[0]])
    else:
        Es = np.atleast_1d(np.asarray(E, dtype=np.float64)).reshape(-1)
    rho = c.cacheval.ltm_density_matrix(Es, states=kind == "states", correction=bool(correction), orbitals=orbitals, optimized=bool(optimized))
    return (rho[0], float(Es[0])) if scalar else (rho, Es)


def _pairs_cache(prob_or_cache, who, npt, pairs, **alg):
    if isinstance(prob_or_cache, DOSCache):
        c = prob_or_cache
        if not (isinstance(c.alg, LTM) and c.alg.pairs is not None):
            raise ValueError(f"{who} needs an LTM(pairs=BandPairs(...)) cache")
        if pairs is not None:
            raise ValueError(f"{who}: a cache brings its own band pairs")
        return c
    if pairs is None:
        raise ValueError(f"{who}: give the band pairs (nocc, or lower and upper)")
    return init(prob_or_cache, LTM(npt=npt, pairs=pairs, **alg))


def _occupied_check(who, fermi, nstates, correction=False, x=None):
    """What `fermi` / `nstates` of joint_dos and interband do not go with; True when occupations were asked for."""
    if fermi is None and nstates is None:
        return False
    if fermi is not None and nstates is not None:
        raise ValueError(f"{who}: give at most one of fermi and nstates")
    if correction:
        raise ValueError(f"{who}: correction=True does not go with fermi / nstates (the curvature correction is not defined on the "
                         "cut simplices of the occupied region)")
    if x is not None and np.iscomplexobj(x):
        raise NotImplementedError(f"{who}: complex energies with fermi / nstates are not implemented (the broadened, Kramers-Kronig "
                                  "form of the spectra has no occupation factors; pass real transition energies)")
    return True


def _occupied_scan(c, who, ws, fermi, nstates, elements):
    """(u, E_F): PairRule.ltm_occupied on the pair rule of the cache `c`, at `fermi` or at the source grid's own level of `nstates`."""
    if c.alg.correction:
        raise ValueError(f"{who}: correction=True does not go with fermi / nstates (the curvature correction is not defined on the "
                         "cut simplices of the occupied region)")
    _refresh(c)
    pr = c.cacheval
    pr.h  # (a stale pair rule is refilled here, and its source with it)
    E_F = float(fermi) if fermi is not None else pr.source.ltm_fermi(nstates)[0]
    return pr.ltm_occupied(ws, E_F, states=c.alg.cumulative, elements=elements), E_F


def _occupied_all_pairs(prob, who, ws, fermi, nstates, npt, elements, pair_kw, alg_kw):
    """All pairs v < c of a DOSProblem as a staircase of pair rules lower = (v, 1), upper = (v + 1, n - v - 1), results added."""
    n = getattr(prob.H, "n", None)
    if not isinstance(prob.H, FourierSeries) or n < 2:
        raise ValueError(f"{who}: all pairs v < c need a Fourier series Hamiltonian of at least two bands")
    total, E_F = None, fermi
    for v in range(n - 1):
        c = init(prob, LTM(npt=npt, pairs=BandPairs(lower=(v, 1), upper=(v + 1, n - v - 1), **pair_kw), **alg_kw))
        try:
            u, E_F = _occupied_scan(c, who, ws, E_F, None if E_F is not None else nstates, elements)
        finally:
            c.cacheval.close()  # this step's energies and elements leave the device now, not with the collector
        total = u if total is None else total + u
    return total


def joint_dos(prob_or_cache, ws, nocc=None, lower=None, upper=None, npt=50, cumulative=False, symmetric=False, fermi=None, nstates=None):
    """The joint density of states J(w) = sum_vc int dk delta(w - (e_c(k) - e_v(k))) at the transition energies `ws`, per unit
    cell, [nw] (with `cumulative` its integral, the number of pairs below w): DeviceRule.ltm on the pair rule of an
    LTM(pairs=BandPairs(...)) cache, or of a DOSProblem with the pairs `nocc` or `lower` + `upper` on a grid of `npt` points
    (`symmetric=True`: eigenvalues from the irreducible nodes of the problem's zone).

    `fermi` or `nstates` (at most one): the occupied joint DOS of a metal at T = 0, with theta(E_F - e_v) theta(e_c - E_F) under the
    integral (PairRule.ltm_occupied: every simplex restricted to its occupied part).  `nstates` finds E_F with `ltm_fermi` on the
    source rule, the grid's own Fermi level.  On a DOSProblem without `nocc`, `lower`, `upper` all pairs v < c are taken, as a
    staircase of pair rules lower = (v, 1), upper = (v + 1, n - v - 1) whose results are added: n - 1 pair rules, each filled and
    scanned once.  Without `fermi` / `nstates` nothing changes."""
    pairs = None if nocc is None and lower is None and upper is None else BandPairs(nocc=nocc, lower=lower, upper=upper)
    if _occupied_check("joint_dos", fermi, nstates):
        ws = np.ascontiguousarray(np.asarray(ws, dtype=np.float64).reshape(-1))
        if pairs is None and not isinstance(prob_or_cache, DOSCache):
            return _occupied_all_pairs(prob_or_cache, "joint_dos", ws, fermi, nstates, npt, None, {}, dict(cumulative=cumulative, symmetric=symmetric))
        c = _pairs_cache(prob_or_cache, "joint_dos", npt, pairs, cumulative=cumulative, symmetric=symmetric)
        return _occupied_scan(c, "joint_dos", ws, fermi, nstates, None)[0]
    c = _pairs_cache(prob_or_cache, "joint_dos", npt, pairs, cumulative=cumulative, symmetric=symmetric)
    _refresh(c)
    ws = np.ascontiguousarray(np.asarray(ws, dtype=np.float64).reshape(-1))
    return c.cacheval.ltm(ws, states=c.alg.cumulative)


def interband(prob_or_cache, ws_or_zs, nocc=None, lower=None, upper=None, operators="velocities", components=None, basis=None, npt=50,
              cumulative=False, correction=False, fermi=None, nstates=None):
    """The interband spectra S_ij = sum_vc int dk M^i_vc conj(M^j_vc) delta(w - (e_c - e_v)) at real transition energies, [nw, ncomp]
    (with `cumulative` their integrals, with `correction` Bloechl's curvature correction on those), or at complex energies z
    (Im z != 0) sum_vc int dk M M^* / (z - (e_c - e_v)), complex128 [nz, ncomp]: -Im / pi at z = w + i eta is the spectrum
    broadened by eta, Re its Kramers-Kronig partner.  DeviceRule.ltm / ltm_green with the attached interband products of the
    pair rule of an LTM(pairs=BandPairs(..., operators=...)) cache, or of a DOSProblem with the pairs `nocc` or `lower` + `upper`
    and `operators` ("velocities": velocity_operators(H, basis)) on a grid of `npt` points.

    `fermi` or `nstates` (at most one): the spectra of a metal at T = 0, with theta(E_F - e_v) theta(e_c - E_F) under the integral
    (PairRule.ltm_occupied).  `nstates` finds E_F with `ltm_fermi` on the source rule, the grid's own Fermi level.  Complex
    energies raise NotImplementedError with them (the broadened form has no occupation factors), `correction=True` ValueError.  On
    a DOSProblem without `nocc`, `lower`, `upper` all pairs v < c are taken, as a staircase of pair rules lower = (v, 1),
    upper = (v + 1, n - v - 1) whose results are added.  Cost: one element build (an eigen-solve of the grid) per step, n - 1 in
    all.  Without `fermi` / `nstates` nothing changes."""
    if _occupied_check("interband", fermi, nstates, correction, np.asarray(ws_or_zs)):
        ws = np.ascontiguousarray(np.asarray(ws_or_zs, dtype=np.float64).reshape(-1))
        if nocc is None and lower is None and upper is None and not isinstance(prob_or_cache, DOSCache):
            if operators is None:
                raise ValueError("interband needs band pairs with operators (joint_dos scans the energies alone)")
            return _occupied_all_pairs(prob_or_cache, "interband", ws, fermi, nstates, npt, "attached",
                                       dict(operators=operators, components=components, basis=basis), dict(cumulative=cumulative))
    pairs = None
    if not (nocc is None and lower is None and upper is None):
        pairs = BandPairs(nocc=nocc, lower=lower, upper=upper, operators=operators, components=components, basis=basis)
    c = _pairs_cache(prob_or_cache, "interband", npt, pairs, cumulative=cumulative, correction=correction)
    if c.alg.pairs.operators is None:
        raise ValueError("interband needs band pairs with operators (joint_dos scans the energies alone)")
    if fermi is not None or nstates is not None:
        return _occupied_scan(c, "interband", np.ascontiguousarray(np.asarray(ws_or_zs, dtype=np.float64).reshape(-1)), fermi, nstates, "attached")[0]
    _refresh(c)
    x = np.asarray(ws_or_zs).reshape(-1)
    if np.iscomplexobj(x):
        return c.cacheval.ltm_green(x, elements="attached")
    return c.cacheval.ltm(np.ascontiguousarray(x, dtype=np.float64), states=c.alg.cumulative, elements="attached", correction=c.alg.correction)


def solve(prob: DOSProblem, alg: DOSAlgorithm, **kwargs):
    return solve_(init(prob, alg, **kwargs))
