"""Pair rules of the tetrahedron method (joint density of states, interband spectra), CPU side: the bindings of
abz_rule_ltm_pairs and abz_rule_ltm_bands, what BandPairs and LTM(pairs=...) accept, and the numpy restatement of the device
tests (tests/pairs_numpy.py) against identities that do not depend on it.  The kernels are checked in test_gpu_ltm_pairs.py."""
import inspect
import os
import re

import numpy as np
import pytest

import ltm_numpy as ln
import pairs_numpy as pn
import wltm_numpy as wn
from expect_numpy import hermitian_upper
from test_gpu_parity import rand_series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. bindings
def test_ltm_pairs_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert re.search(r"^int abz_rule_ltm_pairs\(abz_rule\* src, int v0, int nv, int c0, int nc, abz_rule\* const\* ops, int nops,\s*"
                     r"const int32_t\* comps(?: /\*.*?\*/)?, int ncomp, abz_rule\*\* out\);", hdr, flags=re.M)
    assert re.search(r"^int abz_rule_ltm_bands\(const abz_rule\* r, int\* nb\);", hdr, flags=re.M)
    assert re.search(r"^int abz_rule_ltm_elements_ptr\(const abz_rule\* r, void\*\* base, int64_t\* nbytes, int\* ncomp\);", hdr, flags=re.M)
    assert hasattr(abz.DeviceRule, "ltm_elements_ptr")
    for name in ("abz_rule_ltm_pairs", "abz_rule_ltm_bands", "abz_rule_ltm_elements_ptr"):
        assert name in L.PROTOTYPES and hasattr(L.lib(), name) and ":" + name in jl
    assert "function ltm_pairs(" in jl and "function ltm_pairs!(" in jl and "function ltm_bands(" in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert defs["ABZ_LTM_PAIRS_MAX_OPS"] == 4 == L.LTM_PAIRS_MAX_OPS and defs["ABZ_MAX_BANDS"] == 64 == L.MAX_BANDS
    doc = hdr[hdr.index("Pair rules: joint density of states"):hdr.index("int abz_rule_ltm_pairs(")]
    assert "Degenerate levels" in doc and "partial occupations" in doc
    assert list(inspect.signature(abz.DeviceRule.ltm_pairs).parameters) == ["self", "lower", "upper", "operators", "components"]
    assert issubclass(abz.series.PairRule, abz.DeviceRule) and hasattr(abz.series.PairRule, "refill")
    assert isinstance(abz.DeviceRule.nbands, property)
    assert abz.BandPairs is abz.dos.BandPairs and callable(abz.dos.joint_dos) and callable(abz.dos.interband)


# ---------------------------------------------------------------- 2. what the algorithm accepts
def small_series(abz, d=1, n=4, seed=3):
    c, first = rand_series(np.random.default_rng(seed), (3,) * d, n, hermitian=True)
    return abz.FourierSeries(c, period=1.0, first=first, ndim=d)


def test_band_pairs_validates():
    import autobzcore.jl_amd as abz
    s = small_series(abz)
    bp = abz.BandPairs(nocc=1)
    assert bp.resolve(s)[:2] == ((0, 1), (1, 3)) and bp.operators is None
    bp = abz.BandPairs(lower=range(0, 2), upper=(2, 2), operators=[s, s], components=[0, (0, 1), (1, 0, "im")])
    assert bp.components == ((0, 0, "re"), (0, 1, "re"), (1, 0, "im")) and bp.resolve(s)[:2] == ((0, 2), (2, 2))
    assert abz.BandPairs(lower=(0, 1), upper=(3, 1), operators=s).operators == (s,)
    v = abz.BandPairs(nocc=2, operators="velocities")
    lower, upper, ops, comps = v.resolve(s)
    assert len(ops) == 1 and comps == ((0, 0, "re"),) and (lower, upper) == ((0, 2), (2, 2))
    s3 = small_series(abz, d=3, n=2)
    assert abz.BandPairs(nocc=1, operators="velocities").resolve(s3)[3] == \
        ((0, 0, "re"), (0, 1, "re"), (0, 2, "re"), (1, 1, "re"), (1, 2, "re"), (2, 2, "re"))
    for bad in (dict(), dict(nocc=1, lower=(0, 1), upper=(1, 1)), dict(lower=(0, 1)), dict(nocc=0), dict(nocc=1.5),
                dict(lower=(0, 2), upper=(1, 2)),            # overlapping ranges
                dict(lower=(2, 1), upper=(0, 1)),            # out of order
                dict(lower=range(0, 4, 2), upper=(5, 1)),    # a stride
                dict(lower=(0, 9), upper=(9, 8)),            # 72 pairs
                dict(nocc=1, operators="velocity"), dict(nocc=1, operators=[]), dict(nocc=1, operators=[s] * 5),
                dict(nocc=1, components=[0]), dict(nocc=1, operators="velocities", components=[0]), dict(nocc=1, basis=np.eye(1)),
                dict(nocc=1, operators=[s], components=[]), dict(nocc=1, operators=[s], components=[0] * 17),
                dict(nocc=1, operators=[s], components=[1]), dict(nocc=1, operators=[s], components=[(0, -1)]),
                dict(nocc=1, operators=[s], components=[(0, 0, "abs")]), dict(nocc=1, operators=[s], components=[0.5])):
        with pytest.raises(ValueError):
            abz.BandPairs(**bad)
    with pytest.raises(ValueError, match="window"):
        abz.BandPairs(lower=(0, 9), upper=(9, 8))
    with pytest.raises(ValueError):
        abz.BandPairs(nocc=4).resolve(s)  # no upper band left
    with pytest.raises(ValueError):
        abz.BandPairs(lower=(0, 2), upper=(2, 3)).resolve(s)  # leaves the four bands
    s12 = small_series(abz, n=18)
    with pytest.raises(ValueError, match="window"):
        abz.BandPairs(nocc=9).resolve(s12)  # 81 pairs


def test_ltm_accepts_pairs_and_refuses_where_the_cache_is_made():
    import autobzcore.jl_amd as abz
    s = small_series(abz, d=3)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    bp, bo = abz.BandPairs(nocc=2), abz.BandPairs(nocc=2, operators="velocities")
    assert abz.LTM(pairs=bp).pairs is bp and abz.LTM().pairs is None
    assert abz.LTM(pairs=bp, cumulative=True).cumulative and abz.LTM(pairs=bp, eta=0.1).eta == 0.1 and abz.LTM(pairs=bp, symmetric=True).symmetric
    assert abz.LTM(pairs=bo, cumulative=True, correction=True).correction
    with pytest.raises(ValueError):
        abz.LTM(pairs=bp, cumulative=True, correction=True)  # the unweighted count has no correction
    with pytest.raises(ValueError):
        abz.LTM(pairs="bands")
    # raised where the cache is made, before the device is asked for
    with pytest.raises(ValueError, match="elements"):
        abz.dos.init(abz.DOSProblem(s, [1.0], bz), abz.LTM(npt=4, pairs=bp, elements="energy"))
    for zone in (bz, cub):
        with pytest.raises(ValueError, match="symmetric"):
            abz.dos.init(abz.DOSProblem(s, [1.0], zone), abz.LTM(npt=4, pairs=bo, symmetric=True))
    with pytest.raises(ValueError, match="window"):
        abz.dos.init(abz.DOSProblem(small_series(abz, d=3, n=18), [1.0], bz), abz.LTM(npt=4, pairs=abz.BandPairs(nocc=9)))
    with pytest.raises(ValueError):
        abz.dos.init(abz.DOSProblem(s, [1.0], bz), abz.LTM(npt=4, pairs=abz.BandPairs(nocc=4)))
    # a k-sharded series: refused from the copies the series has, no device is asked for
    import types
    s._dev[0] = types.SimpleNamespace(kshard=(0, 2), _h=None)
    try:
        for pairs in (bp, bo):
            with pytest.raises(NotImplementedError, match="k-sharded"):
                abz.dos.init(abz.DOSProblem(s, [1.0], bz), abz.LTM(npt=4, pairs=pairs))
    finally:
        del s._dev[0]
    with pytest.raises(ValueError, match="pairs"):
        abz.dos.joint_dos(abz.DOSProblem(s, None, bz), [1.0])
    with pytest.raises(ValueError, match="pairs"):
        abz.dos.interband(abz.DOSProblem(s, None, bz), [1.0])


# ---------------------------------------------------------------- 3. the restatement
def random_case(n, nops, seed, nk=7):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((nk, n, n)) + 1j * rng.standard_normal((nk, n, n))
    H = X + np.conj(np.swapaxes(X, 1, 2))
    ops = [rng.standard_normal((nk, n, n)) + 1j * rng.standard_normal((nk, n, n)) for _ in range(nops)]  # only the upper triangle counts
    return rng, H, ops


COMPS = [0, (0, 1), (1, 0, "im"), (2, 1, "re"), (1, 2, "im"), 2, (0, 1)]


def test_components_do_not_depend_on_the_phases_of_the_eigenvectors():
    rng, H, ops = random_case(6, 3, 11)
    _, U = np.linalg.eigh(H, UPLO="U")
    ref = pn.components(pn.interband(H, ops, 1, 2, 3, 3, U=U), COMPS)
    assert np.array_equal(ref, pn.elements(H, ops, 1, 2, 3, 3, COMPS))
    phases = np.exp(2j * np.pi * rng.random((len(H), 1, 6)))
    got = pn.components(pn.interband(H, ops, 1, 2, 3, 3, U=U * phases), COMPS)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(ref[2]).max() > 1e-3 and np.array_equal(ref[1], ref[6])  # an imaginary part that is there; duplicates
    assert np.allclose(ref[3], pn.components(pn.interband(H, ops, 1, 2, 3, 3, U=U), [(1, 2)])[0], rtol=0, atol=1e-12)  # Re is symmetric
    assert np.allclose(ref[4], -pn.components(pn.interband(H, ops, 1, 2, 3, 3, U=U), [(2, 1, "im")])[0], rtol=0, atol=1e-12)


def test_level_pair_sums_do_not_depend_on_the_basis_of_a_degenerate_level():
    """H = U diag(e) U^H with a doubly degenerate lower and a triply degenerate upper level: a random unitary inside each level
    changes single pairs and leaves the sums over the pairs between two levels."""
    rng, _, ops = random_case(7, 2, 5, nk=4)
    e = np.array([-2.0, -1.0, -1.0, 0.5, 2.0, 2.0, 2.0])
    eig = np.tile(e, (4, 1))
    Q = np.stack([np.linalg.qr(rng.standard_normal((7, 7)) + 1j * rng.standard_normal((7, 7)))[0] for _ in range(4)])

    def unitary(m):
        return np.linalg.qr(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m)))[0]

    R = np.stack([np.eye(7, dtype=complex)] * 4)
    for k in range(4):
        R[k, 1:3, 1:3] = unitary(2)
        R[k, 4:7, 4:7] = unitary(3)
    comps = [0, (0, 1), (0, 1, "im"), 1]
    a = pn.components(pn.interband(None, ops, 0, 3, 3, 4, U=Q), comps)
    b = pn.components(pn.interband(None, ops, 0, 3, 3, 4, U=Q @ R), comps)
    assert np.abs(a - b).max() > 1e-2  # single pairs moved
    sa, sb = pn.level_pair_sums(eig, a, 0, 3, 3, 4, 1e-8), pn.level_pair_sums(eig, b, 0, 3, 3, 4, 1e-8)
    assert np.abs(sa - sb).max() <= 1e-12 * np.abs(sa).max()
    # a pair of non-degenerate levels is its own sum
    assert np.array_equal(sa.reshape(4, 4, 3, 4)[:, :, 0, 0], a.reshape(4, 4, 3, 4)[:, :, 0, 0])


def test_trace_identity():
    """sum_{c != v} |M_vc|^2 + q_v^2 = (O^2)_vv in the eigenbasis, to 1e-12 of the scale."""
    n = 6
    _, H, ops = random_case(n, 1, 21)
    _, U = np.linalg.eigh(H, UPLO="U")
    O = hermitian_upper(ops[0])
    Ob = np.einsum("kav,kab,kbc->kvc", U.conj(), O, U)
    O2 = np.einsum("kav,kab,kbc->kvc", U.conj(), O @ O, U)
    for v in range(n):
        total = np.real(Ob[:, v, v]) ** 2
        if v > 0:  # v as the upper band of the pairs below it
            total = total + pn.elements(H, ops, 0, v, v, 1).reshape(len(H), v).sum(axis=1)
        if v < n - 1:
            total = total + pn.elements(H, ops, v, 1, v + 1, n - 1 - v).reshape(len(H), n - 1 - v).sum(axis=1)
        assert np.abs(total - np.real(O2[:, v, v])).max() <= 1e-12 * np.abs(O2).max()


def test_pairs_of_a_diagonal_two_band_model_are_one_band():
    """H = diag(-eps, eps), eps = a + b cos 2 pi k > 0: the pair energy is 2 eps, and the restatements of the scans on it give the
    one-band result of the series 2 eps."""
    npt, a, b = 24, 1.5, 0.7
    eps = a + b * np.cos(2 * np.pi * np.arange(npt) / npt)
    eig = np.stack([-eps, eps], axis=1)
    D = pn.pair_energies(eig, 0, 1, 1, 1)
    assert D.shape == (npt, 1) and np.array_equal(D[:, 0], eps - (-eps)) and np.array_equal(D[:, 0], 2 * eps)
    ws = np.linspace(2 * (a - b) - 0.1, 2 * (a + b) + 0.1, 23)
    one = (2 * eps).reshape(npt, 1)
    for got, ref in zip(ln.ltm(D, ws), ln.ltm(one, ws)):
        assert np.array_equal(got, ref)
    A = np.cos(2 * np.pi * np.arange(npt) / npt).reshape(1, npt, 1) ** 2
    for got, ref in zip(wn.wltm(D, A, ws), wn.wltm(one, A, ws)):
        assert np.array_equal(got, ref)
    # the cumulative JDOS counts the one pair
    assert abs(ln.ltm(D, ws)[1][-1] - 1.0) <= 1e-12 and ln.ltm(D, ws)[1][0] == 0.0


def test_pair_energies_layout():
    eig = np.sort(np.random.default_rng(2).standard_normal((5, 7)), axis=1)
    D = pn.pair_energies(eig, 1, 2, 4, 3)
    for v in range(2):
        for c in range(3):
            assert np.array_equal(D[:, v * 3 + c], eig[:, 4 + c] - eig[:, 1 + v])
    assert np.all(D > 0)
