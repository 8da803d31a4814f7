// Host side of the linear tetrahedron method (LTM) entry points of the C ABI (include/abzhip.h): checks, resident blocks, launches.
#include <algorithm>
#include <cmath>
#include <functional>

#include "abz_internal.h"

using namespace abz;

// The rule is a whole periodic grid with eigenvalues -- or, where the caller scans slabs (`slab_ok`: abz_rule_ltm and the
// energy-weighted abz_rule_ltm_weighted), a slab with its halo plane attached.  The simplices of a cell need all its 2^d
// corners: a slab lacks one halo plane, a list of irreducible nodes the mesh.
static int ltm_check_grid(const abz_rule* r, const char* who, bool slab_ok = false) {
    if (!r->E.base) {
        set_error("LTM needs a rule built with ABZ_WANT_EIG");
        return ABZ_ERR_ARG;
    }
    int64_t ngrid = 1;
    for (int j = 0; j < r->s->d; ++j) ngrid *= r->npt;
    if (!r->full || r->k_offset != 0 || r->nk != ngrid) {
        if (r->full && r->ltm_halo) {
            if (slab_ok) return ABZ_OK;
            set_error("%s: the rule is not a whole periodic grid (a slab of the outermost variable; its halo plane serves abz_rule_ltm and "
                      "abz_rule_ltm_weighted with ABZ_LTM_A_ENERGY only: attached elements, orbital weights, the Fermi level and unfolding "
                      "are not implemented on slabs); build it with abz_ptr_rule_build(s, npt, 0, NULL, NULL, ...)", who);
            return ABZ_ERR_UNSUPPORTED;
        }
        set_error("%s: the rule is not a whole periodic grid (%s); build it with abz_ptr_rule_build(s, npt, 0, NULL, NULL, ...)%s", who,
                  r->full ? "a slab of the outermost variable" : "irreducible nodes of a symmetric rule",
                  r->full && slab_ok ? ", or give the slab its halo plane: attach it with abz_rule_ltm_halo" : "");
        return ABZ_ERR_UNSUPPORTED;
    }
    return ABZ_OK;
}

// the slab arguments of a scan when the rule is a slab with its halo (ltm_check_grid let it through), else false
static bool ltm_slab_of(const abz_rule* r, LtmSlab& slab) {
    if (!r->ltm_halo) return false;
    slab.E = slab.A = r->ltm_halo->E;  // (the energy is the only element of a slab scan)
    slab.nz = rule_outer_planes(r);
    return true;
}

// ---- checks that several entry points make, each where its copy stood: the order of refusals is part of the interface
static int ltm_check_what(const char* who, int what, bool corrected_ok) {
    ABZ_REQUIRE(what == ABZ_LTM_DOS || what == ABZ_LTM_STATES || (corrected_ok && what == ABZ_LTM_STATES_CORRECTED),
                corrected_ok ? "%s: what = %d is neither ABZ_LTM_DOS, ABZ_LTM_STATES nor ABZ_LTM_STATES_CORRECTED"
                             : "%s: what = %d is neither ABZ_LTM_DOS nor ABZ_LTM_STATES", who, what);
    return ABZ_OK;
}

static int ltm_check_source(const char* who, int source) {
    ABZ_REQUIRE(source == ABZ_LTM_A_ELEMENTS || source == ABZ_LTM_A_ENERGY, "%s: source = %d is neither ABZ_LTM_A_ELEMENTS nor ABZ_LTM_A_ENERGY",
                who, source);
    return ABZ_OK;
}

// the three checks that the entry points of the optimized rule repeat
static int ltm_check_source3(const char* who, int source) {
    ABZ_REQUIRE(source == ABZ_LTM_A_ONE || source == ABZ_LTM_A_ENERGY || source == ABZ_LTM_A_ELEMENTS,
                "%s: source = %d is neither ABZ_LTM_A_ONE, ABZ_LTM_A_ENERGY nor ABZ_LTM_A_ELEMENTS", who, source);
    return ABZ_OK;
}

static int ltm_refuse_corrected(const char* who, int what) {
    ABZ_REQUIRE(what != ABZ_LTM_STATES_CORRECTED,
                "%s: ABZ_LTM_STATES_CORRECTED: the optimized rule replaces the curvature correction (ask for ABZ_LTM_STATES)", who);
    return ABZ_OK;
}

static int ltm_require_d3(const char* who, const abz_rule* r) {
    if (r->s->d != 3) {
        set_error("%s: d = %d; the optimized tetrahedron rule is implemented for d = 3", who, r->s->d);
        return ABZ_ERR_UNSUPPORTED;
    }
    return ABZ_OK;
}

// z [nz][2]: finite and off the real axis; `what`: "the trace is" / "G_A is" / "G is"
static int ltm_check_zs(const char* who, const double* z, int nz, const char* what) {
    for (int i = 0; i < nz; ++i) {
        const double re = z[2 * (size_t)i], im = z[2 * (size_t)i + 1];
        ABZ_REQUIRE(std::isfinite(re) && std::isfinite(im), "%s: z[%d] = (%g, %g) is not finite", who, i, re, im);
        ABZ_REQUIRE(im != 0.0, "%s: z[%d] = %g is real; %s computed off the real axis (Im z != 0)", who, i, re, what);
    }
    return ABZ_OK;
}

static int ltm_require_hermitian(const char* who, const abz_rule* r) {
    ABZ_REQUIRE(r->s->hermitian && (!r->H.base || r->herm),
                "%s: the series is not Hermitian (c(-R) = c(R)^dagger): U(k) is the eigenvector matrix of a Hermitian H(k)", who);
    return ABZ_OK;
}

// H(k) of the grid of r for the length of `body(H)`: the rule's own planes or, for a rule of eigenvalues only, the planes of a
// transient H-only rule of the same grid (one band: U = 1, no H needed, none built).  The body's status is the call's; a body
// that failed may have left launches behind, so the stream is synchronised before the transient rule goes.
template <class Body>
static int with_H(abz_rule* r, Body&& body) {
    abz_series* s = r->s;
    std::unique_ptr<abz_rule> tmp;
    if (!r->H.base && s->n > 1) {
        abz_rule* built = nullptr;
        const int rc = rule_build(s, r->npt, 0, nullptr, nullptr, ABZ_WANT_H | ABZ_WANT_H_COMPACT, 0, r->npt, &built, nullptr, false);
        if (rc) return rc;
        tmp.reset(built);
    }
    const int rc = body(tmp ? tmp->H : r->H);
    if (tmp) {
        if (rc) (void)hipStreamSynchronize(s->ctx->stream);
        tmp.reset();
        series_release(s);
    }
    return rc;
}

// out [nz][per][2] <- sets [2 nz][per]: set 2 i the real parts at z_i, set 2 i + 1 the imaginary parts
static void interleave_sets(const double* sets, int nz, size_t per, double* out) {
    for (int i = 0; i < 2 * nz; ++i) {
        const double* src = sets + (size_t)i * per;
        double* o = out + (size_t)(i >> 1) * per * 2 + (size_t)(i & 1);
        for (size_t x = 0; x < per; ++x) o[2 * x] = src[x];
    }
}

// THE path of the four producers of a resident weight block (the real and the complex weights of the linear and of the optimized
// rule): a new block of `sets` real sets tiled like the eigenvalue planes, `fill(ctx, n, W)` launches into its view, one
// synchronisation, then `out` if given -- set by set [sets][nk][n] in the node and band order of abz_rule_export's eig, or, `cplx`,
// the sets 2 i and 2 i + 1 as Re and Im of [sets / 2][nk][n][2] -- and the block becomes r->*which.  The block is complete before
// anything of it reaches `out` and before it replaces the resident one: a refusal or a failure leaves both as they were, and the
// half-made block goes with its DevBuf.
template <class Fill>
static int ltm_weight_block(abz_rule* r, const char* who, LtmBlock abz_rule::*which, int sets, bool cplx, double* out, Fill&& fill) {
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const int n = rule_bands(r);
    LtmBlock block;
    int rc = block.alloc(r->E, r->ntiles, n, sets);
    if (rc) return rc;
    rc = fill(ctx, n, block.view);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) {
        set_error("%s: the kernel failed", who);
        rc = ABZ_ERR_HIP;
    }
    const size_t per = (size_t)r->nk * (size_t)n;
    // complex: the two real sets of one z at a time through the staging of the export, interleaved on the host
    std::vector<double> pair(cplx && out && !rc ? 2 * per : 0);
    for (int i = 0; i < sets && !rc && out; ++i) {
        rc = export_planes(ctx, block.set_view(i, n), n, r->nk, cplx ? pair.data() + (size_t)(i & 1) * per : out + (size_t)i * per);  // (returns when the data has arrived)
        if (cplx && !rc && (i & 1)) interleave_sets(pair.data(), 1, per, out + (size_t)(i >> 1) * per * 2);
    }
    if (rc) return rc;
    r->*which = std::move(block);  // (the previous weights go here)
    return ABZ_OK;
}

extern "C" {

int abz_rule_ltm(abz_rule* r, const double* E, int nE, int what, double* out) try {
    int rc0 = check_rule(r);
    if (rc0) return rc0;
    ABZ_REQUIRE(E && out && nE >= 1, "abz_rule_ltm: bad arguments");
    int rc = ltm_check_what("abz_rule_ltm", what, false);
    if (rc || (rc = ltm_check_grid(r, "abz_rule_ltm", true))) return rc;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    LtmSlab slab;
    return launch_ltm(ctx, rule_bands(r), r->s->d, r->npt, r->E, E, nE, what == ABZ_LTM_STATES, out, ltm_slab_of(r, slab) ? &slab : nullptr);
} ABZ_CATCH_ALL

int abz_rule_ltm_green(abz_rule* r, const double* z, int nz, double* out) try {
    int rc0 = check_rule(r);
    if (rc0) return rc0;
    ABZ_REQUIRE(z && out && nz >= 1, "abz_rule_ltm_green: bad arguments");
    int rc = ltm_check_grid(r, "abz_rule_ltm_green");
    if (rc || (rc = ltm_check_zs("abz_rule_ltm_green", z, nz, "the trace is"))) return rc;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    return launch_ltm_green(ctx, rule_bands(r), r->s->d, r->npt, r->E, z, nz, out);
} ABZ_CATCH_ALL

int abz_rule_ltm_elements(abz_rule* r, const double* A, int ncomp) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE((A == nullptr) == (ncomp == 0), "abz_rule_ltm_elements: elements and ncomp = %d do not go together (drop with NULL, 0)", ncomp);
    ABZ_REQUIRE(ncomp >= 0 && ncomp <= ABZ_LTM_MAX_COMP, "abz_rule_ltm_elements: ncomp = %d outside 1..%d", ncomp, ABZ_LTM_MAX_COMP);
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_elements"))) return rc;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    ABZ_HIP(hipStreamSynchronize(ctx->stream));
    rule_drop_ltm_elements(r);
    if (!A) return ABZ_OK;
    const int n = rule_bands(r);
    if ((rc = r->elems.alloc(r->E, r->ntiles, n, ncomp))) return rc;
    DevBuf stage;  // one component at a time in the host's order
    const size_t cbytes = sizeof(double) * (size_t)r->nk * (size_t)n;
    rc = stage.reserve(cbytes);
    if (!rc && hipMemsetAsync(r->elems.buf.p, 0, r->elems.bytes(r->ntiles, n), ctx->stream) != hipSuccess) {  // the padding columns hold finite numbers
        set_error("abz_rule_ltm_elements: hipMemsetAsync failed");
        rc = ABZ_ERR_HIP;
    }
    for (int c = 0; c < ncomp && !rc; ++c) {
        rc = stage_h2d(ctx, stage.p, A + (size_t)c * (size_t)r->nk * (size_t)n, cbytes);
        if (!rc) rc = launch_ltm_repack(ctx, stage.as<double>(), r->elems.view, c * n, n, r->nk);
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) {
        set_error("abz_rule_ltm_elements: the upload failed");
        rc = ABZ_ERR_HIP;
    }
    if (rc) rule_drop_ltm_elements(r);
    return rc;
} ABZ_CATCH_ALL

// The same block filled on the device from the eigenvectors U(k) (kernels_ltm_orb.hip): |U_ab|^2 (abz_rule_ltm_orbitals) or the
// band projectors U_pb conj(U_qb) (abz_rule_ltm_projectors).  H(k) comes from the rule's own planes or, for a rule of
// eigenvalues only, from a transient H-only rule of the same grid that lives for this call.  Whatever was attached stays in
// place until the new block is complete: a refusal or a failure leaves it untouched.

// what both entry points ask of the rule, before they look at their selection
static int ltm_eigvec_check_rule(abz_rule* r, const char* who, const char* what) {
    int rc = ltm_check_grid(r, who);
    if (rc) return rc;
    if ((rc = refuse_pair_rule(r, who, "H(k) and eigenvectors belong to its source rule"))) return rc;
    if (r->node_of.p) {
        set_error("%s: the rule's eigenvalues were unfolded from irreducible nodes; eigenvectors at every grid "
                  "point are what such a rule avoids (build a full-grid rule with abz_ptr_rule_build)", who);
        return ABZ_ERR_UNSUPPORTED;
    }
    if (!ltm_orbitals_supported(r->s->n)) {
        set_error("%s: %d bands; %s are computed for 1...32", who, r->s->n, what);
        return ABZ_ERR_UNSUPPORTED;
    }
    return ABZ_OK;
}

// the block of `sets` sets of `per` planes tiled like the eigenvalue planes E, filled from H(k) of the grid of r (`fill(H, A)` launches the
// kernel; H: with_H), complete when this returns: the one synchronisation of the call
static int ltm_eigvec_block(abz_rule* r, const char* who, PlaneView E, int per, int sets, const std::function<int(PlaneView, PlaneView)>& fill,
                            LtmBlock& block) {
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    return with_H(r, [&](PlaneView H) {
        int rc = block.alloc(E, r->ntiles, per, sets);
        if (!rc) rc = fill(H, block.view);
        // the one synchronisation of the call: the block is complete, nothing reads the old one or the transient rule any more
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) {
            set_error("%s: the kernel failed", who);
            rc = ABZ_ERR_HIP;
        }
        return rc;
    });
}

// allocate the block of ncomp components, fill it, wait once, attach
static int ltm_eigvec_attach(abz_rule* r, const char* who, int ncomp, const std::function<int(PlaneView, PlaneView)>& fill) {
    LtmBlock block;
    const int rc = ltm_eigvec_block(r, who, r->E, r->s->n, ncomp, fill, block);
    if (rc) return rc;
    r->elems = std::move(block);  // (what was attached goes here)
    return ABZ_OK;
}

int abz_rule_ltm_orbitals(abz_rule* r, const int32_t* orb, int norb) try {
    int rc = check_rule(r);
    if (rc) return rc;
    if ((rc = ltm_eigvec_check_rule(r, "abz_rule_ltm_orbitals", "orbital weights"))) return rc;
    const abz_series* s = r->s;
    const int n = s->n;
    if (orb) {
        ABZ_REQUIRE(norb >= 1 && norb <= ABZ_LTM_MAX_COMP, "abz_rule_ltm_orbitals: norb = %d outside 1..%d", norb, ABZ_LTM_MAX_COMP);
        for (int c = 0; c < norb; ++c)
            ABZ_REQUIRE(orb[c] >= 0 && orb[c] < n, "abz_rule_ltm_orbitals: orb[%d] = %d outside 0..%d", c, orb[c], n - 1);
    } else {
        ABZ_REQUIRE(n <= ABZ_LTM_MAX_COMP, "abz_rule_ltm_orbitals: all %d orbitals are more than %d components; select some (orb, norb)", n,
                    ABZ_LTM_MAX_COMP);
    }
    if ((rc = ltm_require_hermitian("abz_rule_ltm_orbitals", r))) return rc;
    const int ncomp = orb ? norb : n;
    return ltm_eigvec_attach(r, "abz_rule_ltm_orbitals", ncomp, [&](PlaneView H, PlaneView A) {
        return launch_ltm_orbitals(s->ctx, n, r->npt, r->ntiles, H, A, orb, ncomp);
    });
} ABZ_CATCH_ALL

int abz_rule_ltm_projectors(abz_rule* r, const int32_t* pairs, int npairs) try {
    int rc = check_rule(r);
    if (rc) return rc;
    if ((rc = ltm_eigvec_check_rule(r, "abz_rule_ltm_projectors", "band projectors"))) return rc;
    const abz_series* s = r->s;
    const int n = s->n;
    ABZ_REQUIRE(pairs, "abz_rule_ltm_projectors: null pairs");
    ABZ_REQUIRE(npairs >= 1 && npairs <= ABZ_LTM_MAX_COMP, "abz_rule_ltm_projectors: npairs = %d outside 1..%d", npairs, ABZ_LTM_MAX_COMP);
    for (int i = 0; i < npairs; ++i)
        ABZ_REQUIRE(pairs[2 * i] >= 0 && pairs[2 * i] < n && pairs[2 * i + 1] >= 0 && pairs[2 * i + 1] < n,
                    "abz_rule_ltm_projectors: pairs[%d] = (%d, %d) outside 0..%d", i, pairs[2 * i], pairs[2 * i + 1], n - 1);
    const int ncomp = ltm_projector_components(pairs, npairs);
    ABZ_REQUIRE(ncomp <= ABZ_LTM_MAX_COMP,
                "abz_rule_ltm_projectors: %d pairs are %d components (one for p == q, two for p != q), more than %d; attach them in groups",
                npairs, ncomp, ABZ_LTM_MAX_COMP);
    if ((rc = ltm_require_hermitian("abz_rule_ltm_projectors", r))) return rc;
    return ltm_eigvec_attach(r, "abz_rule_ltm_projectors", ncomp, [&](PlaneView H, PlaneView A) {
        return launch_ltm_projectors(s->ctx, n, r->npt, r->ntiles, H, A, pairs, npairs);
    });
} ABZ_CATCH_ALL

// what the entry points that read operator rules (abz_rule_ltm_expectation, abz_rule_ltm_pairs) ask of ops[0 .. nops): H planes of
// Hermitian series on whole periodic grids of the context, npt, d and n of r, not row-major; O[i] <- their planes
static int ltm_check_operators(const char* who, const abz_rule* r, abz_rule* const* ops, int nops, PlaneView* O) {
    const abz_series* s = r->s;
    const int n = s->n;
    int rc = ABZ_OK;
    for (int i = 0; i < nops; ++i) {
        abz_rule* o = ops[i];
        ABZ_REQUIRE(o, "%s: ops[%d] is null", who, i);
        if ((rc = check_rule(o))) return rc;
        if (o->want & ABZ_WANT_H_ROW_MAJOR) {
            set_error("%s: ops[%d] was asked for in the row-major layout; operators are read from column-major or compact H planes", who, i);
            return ABZ_ERR_UNSUPPORTED;
        }
        int64_t ogrid = 1;
        for (int j = 0; j < o->s->d; ++j) ogrid *= o->npt;
        if (!o->full || o->k_offset != 0 || o->nk != ogrid || o->node_of.p) {
            set_error("%s: ops[%d] is not a whole periodic grid (%s); build it with abz_ptr_rule_build(s, npt, 0, NULL, NULL, "
                      "ABZ_WANT_H, ...)", who, i,
                      !o->full ? "irreducible nodes of a symmetric rule" : (o->node_of.p ? "an unfolded rule" : "a slab of the outermost variable"));
            return ABZ_ERR_UNSUPPORTED;
        }
        ABZ_REQUIRE(o->s->ctx == s->ctx, "%s: ops[%d] lives on another context than the rule", who, i);
        ABZ_REQUIRE(o->npt == r->npt && o->s->d == s->d && o->s->n == n && o->ntiles == r->ntiles,
                    "%s: ops[%d] has npt = %d, d = %d, n = %d; the rule has npt = %d, d = %d, n = %d", who, i, o->npt, o->s->d,
                    o->s->n, r->npt, s->d, n);
        ABZ_REQUIRE(o->H.base, "%s: ops[%d] holds no H planes (build it with ABZ_WANT_H)", who, i);
        ABZ_REQUIRE(o->s->hermitian && o->herm, "%s: the series of ops[%d] is not Hermitian (c(-R) = c(R)^dagger)", who, i);
        O[i] = o->H;
    }
    return ABZ_OK;
}

int abz_rule_ltm_expectation(abz_rule* r, abz_rule* const* ops, int nops, const int32_t* comps, int ncomp) try {
    const char* const who = "abz_rule_ltm_expectation";
    int rc = check_rule(r);
    if (rc) return rc;
    if ((rc = ltm_eigvec_check_rule(r, who, "band expectation values"))) return rc;
    const abz_series* s = r->s;
    const int n = s->n;
    ABZ_REQUIRE(ops, "abz_rule_ltm_expectation: null ops");
    ABZ_REQUIRE(nops >= 1 && nops <= ABZ_LTM_EXPECT_MAX_OPS, "abz_rule_ltm_expectation: nops = %d outside 1..%d", nops, ABZ_LTM_EXPECT_MAX_OPS);
    if (!comps) ncomp = nops;
    ABZ_REQUIRE(ncomp >= 1 && ncomp <= ABZ_LTM_MAX_COMP, "abz_rule_ltm_expectation: ncomp = %d outside 1..%d", ncomp, ABZ_LTM_MAX_COMP);
    for (int c = 0; comps && c < ncomp; ++c)
        ABZ_REQUIRE(comps[2 * c] >= 0 && comps[2 * c] < nops && comps[2 * c + 1] >= -1 && comps[2 * c + 1] < nops,
                    "abz_rule_ltm_expectation: comps[%d] = (%d, %d): an operator index outside 0..%d (second: -1 for a single expectation)", c,
                    comps[2 * c], comps[2 * c + 1], nops - 1);
    if ((rc = ltm_require_hermitian("abz_rule_ltm_expectation", r))) return rc;
    PlaneView O[ABZ_LTM_EXPECT_MAX_OPS];
    if ((rc = ltm_check_operators(who, r, ops, nops, O))) return rc;
    return ltm_eigvec_attach(r, who, ncomp, [&](PlaneView H, PlaneView A) {
        return launch_ltm_expectation(s->ctx, n, r->npt, r->ntiles, H, O, nops, A, comps, ncomp);
    });
} ABZ_CATCH_ALL

int abz_rule_ltm_elements_export(abz_rule* r, int* ncomp, double* A) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(ncomp, "abz_rule_ltm_elements_export: null ncomp");
    // a slab made scannable by abz_rule_ltm_halo names its limit here too (any other rule without elements answers 0 components)
    if (r->ltm_halo && (rc = ltm_check_grid(r, "abz_rule_ltm_elements_export"))) return rc;
    *ncomp = r->elems.sets;
    if (!A || !r->elems.buf.p) return ABZ_OK;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const int n = rule_bands(r);
    for (int c = 0; c < r->elems.sets; ++c)  // one component [nk][n] at a time, the order they came in
        if ((rc = export_planes(ctx, r->elems.set_view(c, n), n, r->nk, A + (size_t)c * (size_t)r->nk * (size_t)n))) return rc;
    return ABZ_OK;
} ABZ_CATCH_ALL

// where a resident block lives, its length and its sets (divided by `per_count`: a complex weight is two sets); all zero without one
static int ltm_block_ptr(const abz_rule* r, LtmBlock abz_rule::*which, int per_count, void** base, int64_t* nbytes, int* count) {
    const int rc = check_rule(r);
    if (rc) return rc;
    const LtmBlock& b = r->*which;
    if (base) *base = b.buf.p;
    if (nbytes) *nbytes = (int64_t)b.bytes(r->ntiles, rule_bands(r));
    if (count) *count = b.sets / per_count;
    return ABZ_OK;
}

int abz_rule_ltm_elements_ptr(const abz_rule* r, void** base, int64_t* nbytes, int* ncomp) try {
    return ltm_block_ptr(r, &abz_rule::elems, 1, base, nbytes, ncomp);
} ABZ_CATCH_ALL

int abz_rule_ltm_weighted(abz_rule* r, int source, const double* E, int nE, int what, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(E && out && nE >= 1, "abz_rule_ltm_weighted: bad arguments");
    if ((rc = ltm_check_what("abz_rule_ltm_weighted", what, true))) return rc;
    if ((rc = ltm_check_source("abz_rule_ltm_weighted", source))) return rc;
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_weighted", source == ABZ_LTM_A_ENERGY))) return rc;
    ABZ_REQUIRE(source == ABZ_LTM_A_ENERGY || r->elems.buf.p,
                "abz_rule_ltm_weighted: no matrix elements are attached (abz_rule_ltm_elements; abz_rule_rebuild drops them)");
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const bool energy = source == ABZ_LTM_A_ENERGY;
    LtmSlab slab;
    return launch_ltm_weighted(ctx, rule_bands(r), r->s->d, r->npt, r->E, energy ? r->E : r->elems.view, energy ? 1 : r->elems.sets, E, nE,
                               what, out, ltm_slab_of(r, slab) ? &slab : nullptr);
} ABZ_CATCH_ALL

// The optimized tetrahedron method (kernels_ltm_opt.hip).  Every check comes before anything is reserved or launched.
int abz_rule_ltm_optimized(abz_rule* r, int source, const double* E, int nE, int what, double* out) try {
    const char* const who = "abz_rule_ltm_optimized";
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(E && out && nE >= 1, "abz_rule_ltm_optimized: bad arguments");
    if ((rc = ltm_refuse_corrected(who, what))) return rc;
    if ((rc = ltm_check_what(who, what, false))) return rc;
    if ((rc = ltm_check_source3(who, source))) return rc;
    if ((rc = ltm_require_d3(who, r))) return rc;
    if ((rc = ltm_check_grid(r, who))) return rc;  // (no slab_ok: the stencil reaches one plane before the slab and two behind it)
    ABZ_REQUIRE(source != ABZ_LTM_A_ELEMENTS || r->elems.buf.p,
                "abz_rule_ltm_optimized: no matrix elements are attached (abz_rule_ltm_elements; abz_rule_rebuild drops them)");
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const bool elems = source == ABZ_LTM_A_ELEMENTS;
    return launch_ltm_optimized(ctx, rule_bands(r), r->npt, r->E, elems ? &r->elems.view : nullptr, source == ABZ_LTM_A_ENERGY,
                                elems ? r->elems.sets : 1, E, nE, what == ABZ_LTM_STATES, out);
} ABZ_CATCH_ALL

int abz_rule_ltm_green_weighted(abz_rule* r, int source, const double* z, int nz, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(z && out && nz >= 1, "abz_rule_ltm_green_weighted: bad arguments");
    if ((rc = ltm_check_source("abz_rule_ltm_green_weighted", source))) return rc;
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_green_weighted"))) return rc;
    ABZ_REQUIRE(source == ABZ_LTM_A_ENERGY || r->elems.buf.p,
                "abz_rule_ltm_green_weighted: no matrix elements are attached (abz_rule_ltm_elements, abz_rule_ltm_orbitals; "
                "abz_rule_rebuild drops them)");
    if ((rc = ltm_check_zs("abz_rule_ltm_green_weighted", z, nz, "G_A is"))) return rc;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const bool energy = source == ABZ_LTM_A_ENERGY;
    return launch_ltm_green_weighted(ctx, rule_bands(r), r->s->d, r->npt, r->E, energy ? r->E : r->elems.view, energy ? 1 : r->elems.sets, z, nz, out);
} ABZ_CATCH_ALL

// The Green's functions of the optimized rule (kernels_ltm_green_opt.hip).  Every check comes before anything is reserved or launched.
int abz_rule_ltm_green_optimized(abz_rule* r, int source, const double* z, int nz, double* out) try {
    const char* const who = "abz_rule_ltm_green_optimized";
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(z && out && nz >= 1, "abz_rule_ltm_green_optimized: bad arguments");
    if ((rc = ltm_check_source3(who, source))) return rc;
    if ((rc = ltm_require_d3(who, r))) return rc;
    if ((rc = refuse_pair_rule(r, who, "the effective corner values of e_c - e_v have not been looked at (abz_rule_ltm_green serves it)"))) return rc;
    if ((rc = ltm_check_grid(r, who))) return rc;  // (no slab_ok: the stencil reaches one plane before the slab and two behind it)
    ABZ_REQUIRE(source != ABZ_LTM_A_ELEMENTS || r->elems.buf.p,
                "abz_rule_ltm_green_optimized: no matrix elements are attached (abz_rule_ltm_elements, abz_rule_ltm_orbitals; "
                "abz_rule_rebuild drops them)");
    if ((rc = ltm_check_zs(who, z, nz, source == ABZ_LTM_A_ONE ? "the trace is" : "G_A is"))) return rc;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const bool elems = source == ABZ_LTM_A_ELEMENTS;
    return launch_ltm_green_optimized(ctx, rule_bands(r), r->npt, r->E, elems ? &r->elems.view : nullptr, source == ABZ_LTM_A_ENERGY,
                                      elems ? r->elems.sets : 1, z, nz, out);
} ABZ_CATCH_ALL

int abz_rule_ltm_fermi(abz_rule* r, double nstates, double tol, double* E_F, double* N_F) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(E_F, "abz_rule_ltm_fermi: null E_F");
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_fermi"))) return rc;
    ABZ_REQUIRE(nstates > 0.0 && nstates < (double)rule_bands(r), "abz_rule_ltm_fermi: nstates = %g outside (0, %d)", nstates, rule_bands(r));
    ABZ_REQUIRE(tol > 0.0, "abz_rule_ltm_fermi: tol = %g is not positive", tol);
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    return ltm_fermi(ctx, rule_bands(r), r->s->d, r->npt, r->E, r->nk, nstates, tol, E_F, N_F);
} ABZ_CATCH_ALL

// Integration weights w_b(k; E) per node and band (kernels_ltm_nodew.hip), resident through ltm_weight_block.
int abz_rule_ltm_node_weights(abz_rule* r, const double* E, int nE, int what, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(E, "abz_rule_ltm_node_weights: null energies");
    ABZ_REQUIRE(nE >= 1 && nE <= ABZ_LTM_NODEW_MAX_E, "abz_rule_ltm_node_weights: nE = %d outside 1..%d", nE, ABZ_LTM_NODEW_MAX_E);
    if ((rc = ltm_check_what("abz_rule_ltm_node_weights", what, true))) return rc;
    for (int i = 0; i < nE; ++i) ABZ_REQUIRE(std::isfinite(E[i]), "abz_rule_ltm_node_weights: E[%d] = %g is not finite", i, E[i]);
    // (no slab_ok: a node needs the plane BEFORE it as well, which a halo does not give)
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_node_weights"))) return rc;
    return ltm_weight_block(r, "abz_rule_ltm_node_weights", &abz_rule::nodew, nE, false, out, [&](abz_ctx* ctx, int n, PlaneView W) {
        return launch_ltm_node_weights(ctx, n, r->s->d, r->npt, r->E, W, E, nE, what);
    });
} ABZ_CATCH_ALL

// The weights of the optimized rule into the same resident block (kernels_ltm_opt_nodew.hip).  Every check comes before anything is
// reserved or launched.
int abz_rule_ltm_node_weights_optimized(abz_rule* r, const double* E, int nE, int what, double* out) try {
    const char* const who = "abz_rule_ltm_node_weights_optimized";
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(E, "abz_rule_ltm_node_weights_optimized: null energies");
    ABZ_REQUIRE(nE >= 1 && nE <= ABZ_LTM_NODEW_MAX_E, "abz_rule_ltm_node_weights_optimized: nE = %d outside 1..%d", nE, ABZ_LTM_NODEW_MAX_E);
    if ((rc = ltm_refuse_corrected(who, what))) return rc;
    if ((rc = ltm_check_what(who, what, false))) return rc;
    for (int i = 0; i < nE; ++i) ABZ_REQUIRE(std::isfinite(E[i]), "abz_rule_ltm_node_weights_optimized: E[%d] = %g is not finite", i, E[i]);
    if ((rc = ltm_require_d3(who, r))) return rc;
    if ((rc = ltm_check_grid(r, who))) return rc;  // (no slab_ok: the stencil reaches one plane before the slab and two behind it)
    return ltm_weight_block(r, who, &abz_rule::nodew, nE, false, out, [&](abz_ctx* ctx, int n, PlaneView W) {
        return launch_ltm_node_weights_optimized(ctx, n, r->npt, r->E, W, E, nE, what == ABZ_LTM_STATES);
    });
} ABZ_CATCH_ALL

int abz_rule_ltm_node_weights_ptr(const abz_rule* r, void** base, int64_t* nbytes, int* nE) try {
    return ltm_block_ptr(r, &abz_rule::nodew, 1, base, nbytes, nE);
} ABZ_CATCH_ALL

int abz_rule_ltm_node_weights_dot(abz_rule* r, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_node_weights_dot: null out");
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_node_weights_dot"))) return rc;
    ABZ_REQUIRE(r->nodew.buf.p, "abz_rule_ltm_node_weights_dot: the rule holds no integration weights (abz_rule_ltm_node_weights; "
                                "abz_rule_rebuild drops them)");
    ABZ_REQUIRE(r->elems.buf.p, "abz_rule_ltm_node_weights_dot: no matrix elements are attached (abz_rule_ltm_elements, abz_rule_ltm_orbitals, "
                                "abz_rule_ltm_projectors)");
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    return launch_ltm_node_weights_dot(ctx, rule_bands(r), r->npt, r->ntiles, r->nodew.view, r->nodew.sets, r->elems.view, r->elems.sets, out);
} ABZ_CATCH_ALL

// rho_pq(E_i) from the resident weights and U(k) in one eigen-solve (kernels_ltm_dens.hip).  Nothing is attached and nothing
// replaced: the rule's blocks are read only.  H(k) as in ltm_eigvec_attach: the rule's own planes, or a transient H-only rule.
int abz_rule_ltm_density_matrix(abz_rule* r, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_density_matrix: null out");
    if ((rc = ltm_eigvec_check_rule(r, "abz_rule_ltm_density_matrix", "density matrices"))) return rc;
    abz_series* s = r->s;
    const int n = s->n;
    ABZ_REQUIRE(r->nodew.buf.p, "abz_rule_ltm_density_matrix: the rule holds no integration weights (abz_rule_ltm_node_weights; "
                                "abz_rule_rebuild drops them)");
    if ((rc = ltm_require_hermitian("abz_rule_ltm_density_matrix", r))) return rc;
    abz_ctx* ctx = s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    // (synchronises once, at the delivery of the sums: nothing reads the transient rule after it)
    return with_H(r, [&](PlaneView H) { return launch_ltm_density_matrix(ctx, n, r->npt, r->ntiles, H, r->nodew.view, r->nodew.sets, out); });
} ABZ_CATCH_ALL

// out [nE][nirr][n] <- the orbit sums of the nE real weight sets of the block W of an unfolded rule.  The inverse of the orbit map
// is made once per rule (the map does not change with the values) and serves the real and the complex weights.
static int ltm_fold_sets(abz_rule* r, const char* who, PlaneView W, int nE, double* out) {
    int rc = ABZ_OK;
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const int n = r->s->n;
    const int64_t N = r->nk, nirr = r->unfold_nk;
    const size_t start_bytes = sizeof(int64_t) * ((size_t)nirr + 1);
    if (!r->unfold_inv.p) {
        std::vector<int32_t> node_of((size_t)N), member;
        std::vector<int64_t> start;
        if ((rc = stage_d2h(ctx, node_of.data(), r->node_of.p, sizeof(int32_t) * (size_t)N))) return rc;
        for (int64_t x = 0; x < N; ++x)
            if (node_of[(size_t)x] < 0 || node_of[(size_t)x] >= nirr) {
                set_error("%s: the orbit map names node %d at grid point %lld (the source has %lld nodes)", who, node_of[(size_t)x],
                          (long long)x, (long long)nirr);
                return ABZ_ERR_INTERNAL;
            }
        ltm_orbit_inverse(node_of.data(), N, nirr, start, member);
        DevBuf inv;
        if ((rc = inv.alloc(start_bytes + sizeof(int32_t) * (size_t)N))) return rc;
        if ((rc = stage_h2d(ctx, inv.p, start.data(), start_bytes))) return rc;
        if ((rc = stage_h2d(ctx, static_cast<char*>(inv.p) + start_bytes, member.data(), sizeof(int32_t) * (size_t)N))) return rc;
        r->unfold_inv = std::move(inv);
    }
    const size_t obytes = sizeof(double) * (size_t)nE * (size_t)nirr * (size_t)n;
    if ((rc = ctx->scratch[3].reserve(obytes))) return rc;
    const int64_t* start_dev = r->unfold_inv.as<int64_t>();
    const int32_t* member_dev = reinterpret_cast<const int32_t*>(static_cast<const char*>(r->unfold_inv.p) + start_bytes);
    if ((rc = launch_ltm_node_weights_fold(ctx, n, W, nE, start_dev, member_dev, nirr, ctx->scratch[3].as<double>()))) return rc;
    return stage_d2h(ctx, out, ctx->scratch[3].p, obytes);
}

int abz_rule_ltm_node_weights_fold(abz_rule* r, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_node_weights_fold: null out");
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_node_weights_fold"))) return rc;
    ABZ_REQUIRE(r->node_of.p, "abz_rule_ltm_node_weights_fold: the rule was not made by abz_rule_ltm_unfold: it has no orbits to fold over");
    ABZ_REQUIRE(r->nodew.buf.p, "abz_rule_ltm_node_weights_fold: the rule holds no integration weights (abz_rule_ltm_node_weights; a new "
                                "gather drops them)");
    return ltm_fold_sets(r, "abz_rule_ltm_node_weights_fold", r->nodew.view, r->nodew.sets, out);
} ABZ_CATCH_ALL

int abz_rule_ltm_green_node_weights_fold(abz_rule* r, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_green_node_weights_fold: null out");
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_green_node_weights_fold"))) return rc;
    ABZ_REQUIRE(r->node_of.p, "abz_rule_ltm_green_node_weights_fold: the rule was not made by abz_rule_ltm_unfold: it has no orbits to fold over");
    ABZ_REQUIRE(r->gnodew.buf.p, "abz_rule_ltm_green_node_weights_fold: the rule holds no complex integration weights "
                                 "(abz_rule_ltm_green_node_weights; a new gather drops them)");
    // [2 nz][nirr][n] of the real sets -> [nz][nirr][n][2]
    const int nz = r->gnodew.sets / 2;
    const size_t per = (size_t)r->unfold_nk * (size_t)r->s->n;
    std::vector<double> sets((size_t)2 * nz * per);
    if ((rc = ltm_fold_sets(r, "abz_rule_ltm_green_node_weights_fold", r->gnodew.view, 2 * nz, sets.data()))) return rc;
    interleave_sets(sets.data(), nz, per, out);
    return ABZ_OK;
} ABZ_CATCH_ALL

// Complex integration weights W_b(k; z) of the Green's function per node and band (kernels_ltm_green_nodew.hip), resident in a
// block of their own: 2 nz real weight sets to the dot, the fold and the density-matrix contraction, which are launched as they
// are.  Resident through ltm_weight_block, as the real weights.
int abz_rule_ltm_green_node_weights(abz_rule* r, const double* z, int nz, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(z, "abz_rule_ltm_green_node_weights: null z");
    ABZ_REQUIRE(nz >= 1 && nz <= ABZ_LTM_GREEN_NODEW_MAX_Z, "abz_rule_ltm_green_node_weights: nz = %d outside 1..%d", nz,
                ABZ_LTM_GREEN_NODEW_MAX_Z);
    if ((rc = ltm_check_zs("abz_rule_ltm_green_node_weights", z, nz, "G is"))) return rc;
    // (no slab_ok: a node needs the plane BEFORE it as well, which a halo does not give)
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_green_node_weights"))) return rc;
    return ltm_weight_block(r, "abz_rule_ltm_green_node_weights", &abz_rule::gnodew, 2 * nz, true, out, [&](abz_ctx* ctx, int n, PlaneView W) {
        return launch_ltm_green_node_weights(ctx, n, r->s->d, r->npt, r->E, W, z, nz);
    });
} ABZ_CATCH_ALL

// The complex weights of the optimized rule into the same resident block (kernels_ltm_green_opt_nodew.hip).  Every check comes
// before anything is reserved or launched.
int abz_rule_ltm_green_node_weights_optimized(abz_rule* r, const double* z, int nz, double* out) try {
    const char* const who = "abz_rule_ltm_green_node_weights_optimized";
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(z, "abz_rule_ltm_green_node_weights_optimized: null z");
    ABZ_REQUIRE(nz >= 1 && nz <= ABZ_LTM_GREEN_NODEW_MAX_Z, "abz_rule_ltm_green_node_weights_optimized: nz = %d outside 1..%d", nz,
                ABZ_LTM_GREEN_NODEW_MAX_Z);
    if ((rc = ltm_check_zs(who, z, nz, "G is"))) return rc;
    if ((rc = ltm_require_d3(who, r))) return rc;
    if ((rc = ltm_check_grid(r, who))) return rc;  // (no slab_ok: the stencil reaches one plane before the slab and two behind it)
    return ltm_weight_block(r, who, &abz_rule::gnodew, 2 * nz, true, out, [&](abz_ctx* ctx, int n, PlaneView W) {
        return launch_ltm_green_node_weights_optimized(ctx, n, r->npt, r->E, W, z, nz);
    });
} ABZ_CATCH_ALL

int abz_rule_ltm_green_node_weights_ptr(const abz_rule* r, void** base, int64_t* nbytes, int* nz) try {
    return ltm_block_ptr(r, &abz_rule::gnodew, 2, base, nbytes, nz);
} ABZ_CATCH_ALL

int abz_rule_ltm_green_node_weights_dot(abz_rule* r, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_green_node_weights_dot: null out");
    if ((rc = ltm_check_grid(r, "abz_rule_ltm_green_node_weights_dot"))) return rc;
    ABZ_REQUIRE(r->gnodew.buf.p, "abz_rule_ltm_green_node_weights_dot: the rule holds no complex integration weights "
                                 "(abz_rule_ltm_green_node_weights; abz_rule_rebuild drops them)");
    ABZ_REQUIRE(r->elems.buf.p, "abz_rule_ltm_green_node_weights_dot: no matrix elements are attached (abz_rule_ltm_elements, "
                                "abz_rule_ltm_orbitals, abz_rule_ltm_projectors)");
    abz_ctx* ctx = r->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    // [2 nz][ncomp] of the real sets is [nz][Re, Im][ncomp]
    const int nz = r->gnodew.sets / 2, ncomp = r->elems.sets;
    std::vector<double> sets((size_t)2 * nz * ncomp);
    if ((rc = launch_ltm_node_weights_dot(ctx, rule_bands(r), r->npt, r->ntiles, r->gnodew.view, 2 * nz, r->elems.view, ncomp, sets.data())))
        return rc;
    interleave_sets(sets.data(), nz, (size_t)ncomp, out);
    return ABZ_OK;
} ABZ_CATCH_ALL

// G_pq(z_i) from the resident complex weights and U(k): the contraction of abz_rule_ltm_density_matrix over the 2 nz real sets,
// X = rho[Re W] and Y = rho[Im W] paired on the host.  Nothing is attached and nothing replaced.
int abz_rule_ltm_green_node_weights_matrix(abz_rule* r, double* out) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_green_node_weights_matrix: null out");
    if ((rc = ltm_eigvec_check_rule(r, "abz_rule_ltm_green_node_weights_matrix", "Green's function matrices"))) return rc;
    abz_series* s = r->s;
    const int n = s->n;
    ABZ_REQUIRE(r->gnodew.buf.p, "abz_rule_ltm_green_node_weights_matrix: the rule holds no complex integration weights "
                                 "(abz_rule_ltm_green_node_weights; abz_rule_rebuild drops them)");
    if ((rc = ltm_require_hermitian("abz_rule_ltm_green_node_weights_matrix", r))) return rc;
    abz_ctx* ctx = s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const int nz = r->gnodew.sets / 2;
    const size_t nn = (size_t)n * (size_t)n;
    std::vector<double> sets((size_t)2 * nz * nn * 2);  // [2 nz][n][n][2]: X(z_0), Y(z_0), X(z_1), ...
    // (synchronises once, at the delivery of the sums: nothing reads the transient rule after it)
    rc = with_H(r, [&](PlaneView H) { return launch_ltm_density_matrix(ctx, n, r->npt, r->ntiles, H, r->gnodew.view, 2 * nz, sets.data()); });
    if (rc) return rc;
    // X and Y are Hermitian as they come (the lower triangle the exact conjugate of the upper): entry (p, q) of either triangle
    // is X_pq + i Y_pq, which is conj(X) + i conj(Y) of the mirrored entry
    for (int i = 0; i < nz; ++i) {
        const double* X = sets.data() + (size_t)(2 * i) * nn * 2;
        const double* Y = X + nn * 2;
        double* o = out + (size_t)i * nn * 2;
        for (size_t e = 0; e < nn; ++e) {
            o[2 * e] = X[2 * e] - Y[2 * e + 1];
            o[2 * e + 1] = X[2 * e + 1] + Y[2 * e];
        }
    }
    return ABZ_OK;
} ABZ_CATCH_ALL

// A new whole-grid rule of eigenvalues only (an unfolded rule, a pair rule): `planes` planes of nk = npt^d nodes in padded rows, no
// contraction plan (abz_rule_rebuild refuses it), no values yet: the caller allocates them and sets E.base, and takes the
// reference on the series when it hands the rule out.
static std::unique_ptr<abz_rule> ltm_new_grid_rule(abz_series* s, int npt, int64_t nk, int planes) {
    std::unique_ptr<abz_rule> r(new abz_rule());
    rule_set_empty_plan(r.get());
    r->s = s;
    r->npt = npt;
    r->want = ABZ_WANT_EIG;
    r->full = true;
    r->nk = nk;
    r->ntiles = nk / npt;
    r->planes = planes;
    const int row = (npt + 15) / 16 * 16;
    r->E.tile = (int64_t)planes * row;
    r->E.pitch = row;
    r->E.line_len = npt;
    r->E.row = row;
    return r;
}

// One eigenvalue per band is a scalar that the zone's symmetries leave alone, e_b(S k) = e_b(k): the planes of the whole grid
// are a gather from the irreducible nodes.  The orbit map depends on (npt, d, syms, node list) only and stays with the rule.
int abz_rule_ltm_unfold(abz_rule* src, const int32_t* syms, int nsyms, abz_rule** out) try {
    int rc = check_rule(src);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_unfold: null out");
    ABZ_REQUIRE(syms && nsyms >= 1, "abz_rule_ltm_unfold: no symmetries (syms = %s, nsyms = %d)", syms ? "given" : "NULL", nsyms);
    ABZ_REQUIRE(src->E.base, "abz_rule_ltm_unfold: the source rule holds no eigenvalues (build it with ABZ_WANT_EIG)");
    if (src->full) {
        set_error("abz_rule_ltm_unfold: the source rule is %s, not a list of irreducible nodes: there is nothing to unfold",
                  src->node_of.p ? "an unfolded grid" : "a full grid or a slab of one");
        return ABZ_ERR_UNSUPPORTED;
    }
    abz_series* s = src->s;
    abz_ctx* ctx = s->ctx;
    const int d = s->d, n = s->n, npt = src->npt;
    int64_t N = 1;
    for (int j = 0; j < d; ++j) N *= npt;
    if (N >= ((int64_t)1 << 31)) {
        set_error("abz_rule_ltm_unfold: a grid of %lld points does not fit the 32-bit orbit map", (long long)N);
        return ABZ_ERR_UNSUPPORTED;
    }
    ABZ_HIP(hipSetDevice(ctx->device));
    if (abz_rule* const r = *out) {  // gather again through the map the rule has
        if ((rc = check_rule(r))) return rc;
        ABZ_REQUIRE(r->node_of.p && r != src, "abz_rule_ltm_unfold: *out is not a rule made by abz_rule_ltm_unfold (pass NULL to create one)");
        ABZ_REQUIRE(r->s == s && r->npt == npt && r->unfold_nk == src->nk,
                    "abz_rule_ltm_unfold: *out was unfolded from another geometry (series, npt = %d, %lld nodes; the source has npt = %d, %lld nodes)",
                    r->npt, (long long)r->unfold_nk, npt, (long long)src->nk);
        ABZ_REQUIRE(r->unfold_syms.size() == (size_t)nsyms * d * d && std::equal(r->unfold_syms.begin(), r->unfold_syms.end(), syms),
                    "abz_rule_ltm_unfold: *out was unfolded under another symmetry set (its orbit map does not fit these %d matrices)", nsyms);
        if (r->elems.buf.p || r->nodew.buf.p || r->gnodew.buf.p) {  // matrix elements and integration weights described the old eigenstates
            ABZ_HIP(hipStreamSynchronize(ctx->stream));
            rule_drop_ltm_elements(r);
            rule_drop_ltm_node_weights(r);
        }
        r->herm = src->herm;
        if ((rc = launch_ltm_unfold(ctx, src->E, r->E, r->node_of.as<int32_t>(), n, npt, r->ntiles))) return rc;
        ABZ_HIP(hipStreamSynchronize(ctx->stream));
        return ABZ_OK;
    }
    std::unique_ptr<abz_rule> r = ltm_new_grid_rule(s, npt, N, n);
    r->herm = src->herm;
    r->unfold_nk = src->nk;
    r->unfold_syms.assign(syms, syms + (size_t)nsyms * d * d);
    DevBuf rank;  // scratch: int32 [N] node of a point, then the counter of points without one
    int missing = 0;
    if ((rc = r->vals.alloc(LtmBlock::bytes(r->E, r->ntiles, n)))) return rc;
    if ((rc = r->node_of.alloc(sizeof(int32_t) * (size_t)N))) return rc;
    if ((rc = rank.alloc(sizeof(int32_t) * ((size_t)N + 1)))) return rc;
    r->E.base = r->vals.as<double>();
    int* const missing_dev = reinterpret_cast<int*>(rank.as<int32_t>() + N);
    rc = launch_ltm_orbit_map(ctx, npt, d, syms, nsyms, src->idx.as<int32_t>(), src->nk, rank.as<int32_t>(), r->node_of.as<int32_t>(), missing_dev);
    if (!rc) rc = launch_ltm_unfold(ctx, src->E, r->E, r->node_of.as<int32_t>(), n, npt, r->ntiles);
    // the call's one synchronisation: the counter, the map and the planes have arrived
    hipError_t e = hipMemcpyAsync(&missing, missing_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess && !rc) {
        set_error("abz_rule_ltm_unfold: %s", hipGetErrorString(e));
        rc = ABZ_ERR_HIP;
    }
    if (rc) return rc;
    if (missing != 0) {
        set_error("abz_rule_ltm_unfold: %d of the %lld grid points have no image under the %d symmetries among the %lld nodes of the source rule "
                  "(the node list does not cover every orbit)", missing, (long long)N, nsyms, (long long)src->nk);
        return ABZ_ERR_ARG;
    }
    s->refs += 1;
    *out = r.release();  // (the handle: not a device block)
    return ABZ_OK;
} ABZ_CATCH_ALL

// Pair rule: the differences e_c - e_v of two band ranges of `src` as the eigenvalue planes of a whole-grid rule of its own, and
// the interband products M^i_vc conj(M^j_vc) as its attached elements (kernels_ltm_pairs.hip).  Every scan that reads E, attached
// elements or weight blocks sizes itself by rule_bands() and takes it as it takes an unfolded rule.  Both blocks are complete
// before they replace anything: a refusal or a failure leaves *out and src as they were.
int abz_rule_ltm_bands(const abz_rule* r, int* nb) try {
    int rc = check_rule(r);
    if (rc) return rc;
    ABZ_REQUIRE(nb, "abz_rule_ltm_bands: null nb");
    *nb = rule_bands(r);
    return ABZ_OK;
} ABZ_CATCH_ALL

int abz_rule_ltm_pairs(abz_rule* src, int v0, int nv, int c0, int nc, abz_rule* const* ops, int nops, const int32_t* comps, int ncomp,
                       abz_rule** out) try {
    const char* const who = "abz_rule_ltm_pairs";
    int rc = check_rule(src);
    if (rc) return rc;
    ABZ_REQUIRE(out, "abz_rule_ltm_pairs: null out");
    ABZ_REQUIRE(nops >= 0 && nops <= ABZ_LTM_PAIRS_MAX_OPS, "abz_rule_ltm_pairs: nops = %d outside 0..%d", nops, ABZ_LTM_PAIRS_MAX_OPS);
    if ((rc = refuse_pair_rule(src, who, "pairs are formed from the bands of a rule of the series"))) return rc;
    // without operators: what abz_rule_ltm takes as a whole grid; with them: what abz_rule_ltm_expectation takes
    if ((rc = nops ? ltm_eigvec_check_rule(src, who, "interband matrix elements") : ltm_check_grid(src, who))) return rc;
    abz_series* s = src->s;
    abz_ctx* ctx = s->ctx;
    const int n = s->n, npt = src->npt;
    ABZ_REQUIRE(!(nops && n == 1), "abz_rule_ltm_pairs: one band has no pairs");
    ABZ_REQUIRE(v0 >= 0 && nv >= 1 && nc >= 1 && c0 >= 0 && (int64_t)v0 + nv <= c0 && (int64_t)c0 + nc <= n,
                "abz_rule_ltm_pairs: ranges [%d, %d + %d) and [%d, %d + %d) of %d bands: 0 <= v0, nv >= 1, nc >= 1, v0 + nv <= c0, c0 + nc <= n",
                v0, v0, nv, c0, c0, nc, n);
    ABZ_REQUIRE((int64_t)nv * nc <= ABZ_MAX_BANDS, "abz_rule_ltm_pairs: %d x %d pairs are more than the %d pseudo-bands a scan takes; use a window of bands",
                nv, nc, ABZ_MAX_BANDS);
    const int nb = nv * nc;
    PlaneView O[ABZ_LTM_PAIRS_MAX_OPS];
    std::vector<int32_t> cv;  // [ncomp][3]
    if (nops) {
        ABZ_REQUIRE(ops, "abz_rule_ltm_pairs: null ops");
        if (!comps) ncomp = nops;
        ABZ_REQUIRE(ncomp >= 1 && ncomp <= ABZ_LTM_MAX_COMP, "abz_rule_ltm_pairs: ncomp = %d outside 1..%d", ncomp, ABZ_LTM_MAX_COMP);
        cv.resize((size_t)3 * ncomp);
        for (int c = 0; c < ncomp; ++c) {
            cv[3 * c] = comps ? comps[3 * c] : c;
            cv[3 * c + 1] = comps ? comps[3 * c + 1] : c;
            cv[3 * c + 2] = comps ? comps[3 * c + 2] : 0;
            ABZ_REQUIRE(cv[3 * c] >= 0 && cv[3 * c] < nops && cv[3 * c + 1] >= 0 && cv[3 * c + 1] < nops && (cv[3 * c + 2] == 0 || cv[3 * c + 2] == 1),
                        "abz_rule_ltm_pairs: comps[%d] = (%d, %d, %d): operator indices inside 0..%d, part 0 (Re) or 1 (Im)", c, cv[3 * c],
                        cv[3 * c + 1], cv[3 * c + 2], nops - 1);
        }
        if ((rc = ltm_require_hermitian(who, src))) return rc;
        if ((rc = ltm_check_operators(who, src, ops, nops, O))) return rc;
    } else {
        ncomp = 0;
    }
    abz_rule* const old = *out;
    if (old) {
        if ((rc = check_rule(old))) return rc;
        ABZ_REQUIRE(old->nb && old != src, "abz_rule_ltm_pairs: *out is not a rule made by abz_rule_ltm_pairs (pass NULL to create one)");
        ABZ_REQUIRE(old->s == s && old->npt == npt && old->pair_v0 == v0 && old->pair_nv == nv && old->pair_c0 == c0 && old->pair_nc == nc &&
                        old->pair_nops == nops && old->pair_comps == cv,
                    "abz_rule_ltm_pairs: *out was made for another series, npt, band ranges or components (npt = %d, [%d, %d + %d) x [%d, %d + %d), "
                    "%d operators)", old->npt, old->pair_v0, old->pair_v0, old->pair_nv, old->pair_c0, old->pair_c0, old->pair_nc, old->pair_nops);
    }
    ABZ_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<abz_rule> made;  // a new rule takes its values below, once they are complete
    if (!old) made = ltm_new_grid_rule(s, npt, src->nk, nb);
    abz_rule* const r = old ? old : made.get();
    PlaneView E = r->E;  // the nb planes of the pair energies, tiled like the planes of an unfolded rule
    DevBuf vals;
    LtmBlock elems;
    if ((rc = vals.alloc(LtmBlock::bytes(E, src->ntiles, nb)))) return rc;
    E.base = vals.as<double>();
    // the energies always from the source's planes: the spectra sit on the eigenvalues the source's own scans see
    rc = launch_ltm_pair_energies(ctx, npt, src->ntiles, src->E, E, v0, nv, c0, nc);
    if (!rc && nops)
        rc = ltm_eigvec_block(src, who, E, nb, ncomp, [&](PlaneView H, PlaneView Ab) {
            return launch_ltm_pairs(ctx, n, npt, src->ntiles, H, O, nops, Ab, v0, nv, c0, nc, cv.data(), ncomp);
        }, elems);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) {
        set_error("abz_rule_ltm_pairs: the kernel failed");
        rc = ABZ_ERR_HIP;
    }
    if (rc) return rc;
    if (made) {
        r->nb = nb;
        r->pair_v0 = v0;
        r->pair_nv = nv;
        r->pair_c0 = c0;
        r->pair_nc = nc;
        r->pair_nops = nops;
        r->pair_comps = cv;
    }
    r->herm = src->herm;
    r->vals = std::move(vals);  // (the old energies and elements go here)
    r->E = E;
    rule_drop_ltm_node_weights(r);  // they described the old energies
    r->elems = std::move(elems);    // (an empty block without operators)
    if (made) {
        s->refs += 1;
        *out = made.release();  // (the handle: not a device block)
    }
    return ABZ_OK;
} ABZ_CATCH_ALL

// The scans of a pair rule with the occupations of a metal (kernels_ltm_pairs_occ.hip).  Every check comes before anything is reserved
// or launched; nothing is attached, replaced or dropped on either rule.
int abz_rule_ltm_pairs_occupied(abz_rule* src, abz_rule* pairs, double E_F, int source, const double* w, int nw, int what, double* out) try {
    const char* const who = "abz_rule_ltm_pairs_occupied";
    int rc = check_rule(src);
    if (rc || (rc = check_rule(pairs))) return rc;
    ABZ_REQUIRE(w && out && nw >= 1, "abz_rule_ltm_pairs_occupied: bad arguments (w = %s, out = %s, nw = %d)", w ? "given" : "NULL",
                out ? "given" : "NULL", nw);
    ABZ_REQUIRE(pairs->nb, "abz_rule_ltm_pairs_occupied: `pairs` is not a rule made by abz_rule_ltm_pairs");
    if ((rc = refuse_pair_rule(src, who, "the occupations are those of the bands of the pair rule's source"))) return rc;
    if (what == ABZ_LTM_STATES_CORRECTED) {
        set_error("abz_rule_ltm_pairs_occupied: ABZ_LTM_STATES_CORRECTED: the curvature correction is not defined on cut simplices");
        return ABZ_ERR_UNSUPPORTED;
    }
    if ((rc = ltm_check_what(who, what, false))) return rc;
    ABZ_REQUIRE(source == ABZ_LTM_A_ELEMENTS || source == ABZ_LTM_A_ONE, "%s: source = %d is neither ABZ_LTM_A_ELEMENTS nor ABZ_LTM_A_ONE", who,
                source);
    if ((rc = ltm_check_grid(src, who)) || (rc = ltm_check_grid(pairs, who))) return rc;
    ABZ_REQUIRE(src->s == pairs->s && src->npt == pairs->npt,
                "abz_rule_ltm_pairs_occupied: the rules differ in their series or grid (src: npt = %d, pairs: npt = %d)", src->npt, pairs->npt);
    ABZ_REQUIRE(pairs->pair_c0 + pairs->pair_nc <= rule_bands(src), "abz_rule_ltm_pairs_occupied: the upper range [%d, %d + %d) leaves the %d bands of src",
                pairs->pair_c0, pairs->pair_c0, pairs->pair_nc, rule_bands(src));
    ABZ_REQUIRE(source == ABZ_LTM_A_ONE || pairs->elems.buf.p,
                "abz_rule_ltm_pairs_occupied: the pair rule has no elements (abz_rule_ltm_pairs with operators, abz_rule_ltm_elements); "
                "ABZ_LTM_A_ONE gives the joint DOS");
    ABZ_REQUIRE(std::isfinite(E_F), "abz_rule_ltm_pairs_occupied: E_F = %g is not finite", E_F);
    abz_ctx* ctx = src->s->ctx;
    ABZ_HIP(hipSetDevice(ctx->device));
    const bool one = source == ABZ_LTM_A_ONE;
    return launch_ltm_pairs_occupied(ctx, src->s->d, src->npt, src->E, one ? nullptr : &pairs->elems.view, one ? 1 : pairs->elems.sets, pairs->nb,
                                     pairs->pair_v0, pairs->pair_c0, pairs->pair_nc, E_F, w, nw, what == ABZ_LTM_STATES, out);
} ABZ_CATCH_ALL

}  // extern "C"
