/*
 * abzhip.h -- C ABI of libabzhip.so: the MI355X (gfx950) hot path behind AutoBZCore.jl's
 * integrand/algorithm dispatch boundary.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, and returns an int status
 * (0 = ok, negative = error; abz_last_error() gives the message).  No C++ exceptions cross the
 * boundary.  Host arrays are owned by the caller (Julia must GC.@preserve them for the ccall);
 * device memory lives behind opaque handles owned by the library.  Handles are NOT thread-safe:
 * use one abz_ctx (one HIP stream) per host thread, like the reference gives every thread its own
 * workspace and deep-copied solver (src/fourier.jl:60-86, src/interfaces.jl:213).  What MAY run
 * concurrently: calls on handles of different contexts; and the abz_*_destroy calls on any handle
 * beside other threads' work on the same context -- the context <- series <- rule reference counts
 * are atomic, so a finalizer thread of a garbage-collected host language may release handles while
 * another thread builds rules from the same series.  Everything else on one context is serial.
 *
 * Citations `ref:` are file:line into lxvm/AutoBZCore.jl v0.3.8 -- the reference interface each
 * entry point replaces.  The reference-side binding (Julia ccall shim) is in INTEGRATION.md and
 * julia/AutoBZCoreHIP.jl.
 *
 * Coefficient memory order is the reference's own (Julia, column-major): interleaved (re, im)
 * doubles; inside one coefficient the n x n block is column-major (row index fastest); blocks are
 * ordered with i_1 fastest ... i_d slowest, i.e. exactly `Array{SMatrix{n,n,ComplexF64},d}`
 * (aps_example/aps_example.jl:15-27).  A scalar series is n = 1.
 */
#ifndef ABZHIP_H
#define ABZHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABZ_VERSION 502

/* status codes */
#define ABZ_OK 0
#define ABZ_ERR_ARG (-1)     /* ref: ArgumentError sites src/fourier.jl:167,267,506 */
#define ABZ_ERR_HIP (-2)     /* a HIP runtime call failed */
#define ABZ_ERR_NOGPU (-3)   /* no usable gfx950 device: the product has NO CPU fallback */
#define ABZ_ERR_UNSUPPORTED (-4)
#define ABZ_ERR_NOMEM (-5)
#define ABZ_ERR_INTERNAL (-6) /* a C++ exception was caught at the boundary (none crosses it); text in abz_last_error() */

#define ABZ_MAX_DIM 3        /* BZ dimension d = 1..3 (ref tests: test/fourier.jl:10,43) */
#define ABZ_MAX_BANDS 64     /* n x n Hamiltonians up to n = 64 (33...64: kernels_big.hip, kernels_big_vec.hip) */

typedef struct abz_ctx abz_ctx;       /* device + stream + scratch + profiling */
typedef struct abz_series abz_series; /* device-resident Fourier coefficients (FourierSeries / FourierWorkspace) */
typedef struct abz_rule abz_rule;     /* device-resident cached rule values (FourierPTR / FourierMonkhorstPack / GGR data) */

/* what a rule / node evaluation materialises (bit mask) */
#define ABZ_WANT_H 1    /* series values H(k): FourierValue.s, ref src/fourier.jl:111-114 */
#define ABZ_WANT_EIG 2  /* ascending eigenvalues of Hermitian(H(k)) (upper triangle), ref src/dos_ggr.jl:19,34 */
#define ABZ_WANT_VEL 4  /* band velocities Re diag(U' dH/dk_j U) * t_j, ref src/dos_ggr.jl:20,35 (implies EIG) */
/* With ABZ_WANT_H, for a Hermitian series of n <= 16 bands: keep H(k) as its UPPER TRIANGLE only (what Hermitian(h) reads,
 * src/dos_ggr.jl:19,34) -- n^2 value planes instead of 2 n^2, e.g. 96 instead of 168 bytes per k-point for 3 bands + eig.
 * The lower triangle is the conjugate of the upper one bit for bit, so nothing is lost: abz_rule_export still returns
 * the full matrices and every built-in integrand reads the compact planes.  Ignored (full layout) for series that are
 * not Hermitian or have more than 16 bands; abz_rule_info reports the bit only when the rule really is compact.
 * Plane order inside a tile: Re H[a][b], Im H[a][b] for a < b at planes b^2 + 2a, b^2 + 2a + 1; H[b][b] at b^2 + 2b. */
#define ABZ_WANT_H_COMPACT 8
/* abz_eval_nodes only: H_out holds every matrix ROW-major (element (a, b) at 2 (a n + b) + {re, im}) instead of the reference's
 * column-major blocks -- for hosts whose arrays are row-major (the Python mirror: transposing 4 096 matrices of 32 x 32 on the
 * host took longer than evaluating them). */
#define ABZ_WANT_H_ROW_MAJOR 16

/* built-in device integrands f(FourierValue(k, H(k)), params...; sweep) -- the integrands that
 * appear in the reference's tests, docs and example (user closures cannot cross a C ABI; they get
 * H(k) batches through abz_rule_export / abz_eval_nodes instead).  Values are complex. */
#define ABZ_F_ONE 0        /* 1                                   ref test/brillouin.jl:38        ncomp 1  */
#define ABZ_F_LINEAR 1     /* a*s + b, scalar s = H[1,1]          ref test/fourier.jl:41          ncomp 1; params {a, b} */
#define ABZ_F_LINEAR_X 2   /* a*s*x .+ b                          ref test/fourier.jl:16          ncomp d; params {a, b} */
#define ABZ_F_DOS 3        /* -Im tr inv((w+i eta)I - H)/pi       ref aps_example/aps_example.jl:30  ncomp 1; params {eta}; sweep w */
#define ABZ_F_TRGLOC 4     /* tr inv((w+i eta)I - H)              ref docs/src/examples.md:21    ncomp 1; params {eta}; sweep w */
#define ABZ_F_GLOC 5       /* inv((w+i eta)I - H)  (n x n, col-major) ref docs/src/examples.md:90  ncomp n*n; params {eta}; sweep w */
#define ABZ_F_DOS_EIG 6    /* (eta/pi) sum_b 1/((w-e_b)^2+eta^2) from cached eigenvalues == ABZ_F_DOS  ncomp 1 */

/* iterated limits for IAI (ref: src/brillouin.jl:2-5,267,304) */
#define ABZ_LIMS_CUBIC 0        /* CubicLimits(a, b) */
#define ABZ_LIMS_TETRAHEDRAL 1  /* TetrahedralLimits(a): 0 <= x_1 <= ... <= x_d <= a_d (scaled) */
/* General convex irreducible zones (ext/SymmetryReduceBZExt.jl:33-58, ext/ibzlims.jl:198-289):
 * lim_a = packed polytope, lim_b[0] = number of doubles in lim_a.
 *   POLYHEDRAL (d = 3): per face [nv, x y z of its nv vertices in order around the face]; vertices shared
 *                       between faces must be bit-identical.
 *   POLYGON (d = 2):    vertices (x, y) in order around the boundary. */
#define ABZ_LIMS_POLYHEDRAL 2
#define ABZ_LIMS_POLYGON 3

/* profiled kernels (abz_prof_read) */
#define ABZ_K_CONTRACT 0   /* outer-dimension contraction (workspace_contract!)      */
#define ABZ_K_EVAL 1       /* innermost 1-D evaluation (+ fused eig)  (workspace_evaluate!) -- the Fourier-eval kernel */
#define ABZ_K_REDUCE 2     /* integrand scan + reduce over a cached rule (quadsum)   */
#define ABZ_K_GGR 3        /* GGR formula scan (sum_ggr)                             */
#define ABZ_K_EIG 4        /* stand-alone Hermitian eigensolve                        */
#define ABZ_K_GGRBUILD 5   /* fused GGR build: H, dH/dk, eig, velocities per node (get_ggr_data, ref src/dos_ggr.jl:14-44) */
#define ABZ_K_LTM 6        /* linear tetrahedron scan over cached eigenvalues (abz_rule_ltm) */
#define ABZ_K_EVAL_FUSED 7 /* launches only, no time: the ABZ_K_EVAL launches that contracted the last outer variable themselves */
#define ABZ_K_COUNT 8      /* the ids above: the timed kernels and the first launch counter */
#define ABZ_K_EVAL_PASSWAVE 8 /* launches only, no time: the ABZ_K_EVAL_FUSED launches that ran one pass of a line pair per wave */
#define ABZ_K_SLOTS 9      /* ids abz_prof_read takes: 0 ... ABZ_K_SLOTS - 1 */

/* The library's own view of its memory, for leak checks and capacity planning (no reference counterpart):
 * info[0] device bytes handed out by its allocator and not yet returned (all contexts: coefficients, contracted
 * sets, rule values, scratch), info[1] device bytes parked in its cache of freed blocks (ABZ_POOL_MB), info[2] the
 * part of info[0] that is `ctx`'s grow-only scratch, info[3] `ctx`'s pinned host staging bytes, info[4] live blocks.
 * ctx may be NULL (then info[2] = info[3] = 0). */
int abz_mem_info(abz_ctx* ctx, int64_t* info);

/* ---------------------------------------------------------------- library / context */
const char* abz_last_error(void);
int abz_version(void);
/* Number of visible HIP devices; ABZ_ERR_NOGPU (and *n = 0) if there is none. */
int abz_device_count(int* n);
/* One context per host thread / rank: binds `device`, creates its stream. */
int abz_ctx_create(int device, abz_ctx** out);
/* The same on a stream the caller owns (a `hipStream_t`, e.g. the current stream of the PyTorch harness):
 * the library's launches are then ordered with the caller's own work and with RCCL collectives enqueued on
 * that stream -- the sharded sweep needs no host synchronisation between its scan and its gather.  The
 * stream is borrowed: abz_ctx_destroy does not destroy it.  Replaces: nothing in the reference (it has no
 * device queue); the per-thread workspace rule of src/fourier.jl:60-86 still applies, one context per thread. */
int abz_ctx_create_on_stream(int device, void* hip_stream, abz_ctx** out);
int abz_ctx_destroy(abz_ctx* ctx);
int abz_ctx_sync(abz_ctx* ctx);
/* HIP-event timing of the library's own launches on the context's stream.  on = 0: off; 1: every
 * kernel id; otherwise a mask with bit (k+1) selecting ABZ_K_<k>.  The events are bound to the kernel
 * dispatches themselves (no marker packets between launches): a timed call of several launches runs
 * from the start of its first kernel to the end of its last; memsets and copies are not timed. */
int abz_prof_enable(abz_ctx* ctx, int on);
int abz_prof_reset(abz_ctx* ctx);
int abz_prof_read(abz_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

/* ---------------------------------------------------------------- series
 * Replaces: FourierSeries(c; period, offset) + workspace_allocate_vec (src/fourier.jl:56-86).
 * dims[j] = M_j, first[j] = integer frequency of the first coefficient along dim j
 * (= 1 + offset_j of FourierSeriesEvaluators, or the OffsetArray's first axis value),
 * s(x) = sum_i c[i] exp(2 pi i sum_j (first_j + i_j) x_j / period_j), i_j = 0..M_j-1. */
int abz_series_create(abz_ctx* ctx, const double* coef_reim, int d, const int32_t* dims,
                      const int32_t* first, const double* period, int n, abz_series** out);
int abz_series_destroy(abz_series* s);
/* Replace the coefficients in place (same shape).  Replaces: mutating `h.c` / assigning cache.H
 * (test/dos.jl:122-129); rules built from the series become stale until abz_rule_rebuild. */
int abz_series_update(abz_series* s, const double* coef_reim);
/* How the device inverts (omega + i eta) I - H(k) for this series' resolvent integrands (ABZ_F_DOS, ABZ_F_TRGLOC, ABZ_F_GLOC).
 * ABZ_PIVOT_NONE, the default: the fastest route for the series, band count and integrand (closed forms, p'/p of the
 * tridiagonal form, Gauss-Jordan without pivoting); what that covers is written at abz_rule_reduce.
 * ABZ_PIVOT_PARTIAL: every such value comes from a Gauss-Jordan inverse with partial pivoting by rows, the choice LAPACK's
 * `inv` makes (at each step the row left with the largest |entry|^2 in the pivot column; entries below 1e-154 in magnitude
 * count as zero for the choice): accurate wherever cond(z I - H(k)) is modest, Hermitian or not, at any eta.  A column that
 * is exactly zero gives Inf / NaN where LAPACK would raise a singular-matrix error.  Hermitian series give up their
 * tridiagonal and closed-form routes in this mode, and every series is inverted node by node: the cost is tabulated in
 * DESIGN.md section 9.  Results are the same bits on every repeat of a call.
 * The mode belongs to the series and is read when a scan, sum or solve is launched: it holds for abz_rule_reduce(_device),
 * abz_ptr_sum, abz_autoptr_solve(_many) and abz_iai_solve(_many) / abz_eval_line_nodes, for rules built before or after the
 * call (their H(k) do not depend on it), and survives abz_series_update.  A scan in this mode needs the matrices: a rule
 * without ABZ_WANT_H answers ABZ_ERR_UNSUPPORTED; ABZ_WANT_H_COMPACT rules are expanded as they are read.  Up to 4 bands the
 * scans of a series that is not Hermitian are the default's (they pivot already, or use p'/p of the characteristic polynomial
 * for the traces of 2 and 3 bands).  abz_iai_solve* above 4 bands keeps the innermost adaptive loops on the host in this mode
 * (the device panel kernels do not pivot) and is slower for it.  Other integrands, ABZ_F_DOS_EIG among them, are untouched.
 * A mode that is neither, or a null pointer: ABZ_ERR_ARG.  Entry points added without a change of ABZ_VERSION. */
#define ABZ_PIVOT_NONE 0     /* default: today's routes, bit for bit */
#define ABZ_PIVOT_PARTIAL 1  /* every inverse of (w + i eta) I - H(k) taken for this series pivots by rows */
int abz_series_set_pivoting(abz_series* s, int mode);
int abz_series_get_pivoting(const abz_series* s, int* mode);

/* ---------------------------------------------------------------- arbitrary nodes
 * Replaces: the fallback evaluator f.w(x) (src/fourier.jl:120-122) and the body of a
 * BatchIntegrand f!(y, x, p) (src/batch.jl:1-38) for FourierValue batches.
 * k is [nk][d] (x_1 first).  Outputs (host, nullable per `want`):
 *   H_out   [nk][n*n][2]  column-major blocks (reference layout)
 *   eig_out [nk][n]
 * Evaluation is hierarchical when nodes share outer coordinates; results do not depend on it. */
int abz_eval_nodes(abz_series* s, const double* k, int64_t nk, int want, double* H_out,
                   double* eig_out);

/* ---------------------------------------------------------------- PTR rules
 * Replaces: FourierPTR ctor + fourier_ptr! (src/fourier.jl:132-174), FourierMonkhorstPack ctor +
 * _fourier_symptr! (:216-277), nextrule (:315-321), and get_ggr_data (src/dos_ggr.jl:14-44).
 * Full grid:  irr_idx = wsym = NULL, nirr = 0  -> nodes are all npt^d grid points, i_1 fastest.
 * Symmetric:  irr_idx [nirr][d] 0-based grid indices in column-major order and their integer
 *             weights wsym [nirr] (from abz_symptr_rule).
 * The values stay resident in HBM (planar layout). */
int abz_ptr_rule_build(abz_series* s, int npt, int64_t nirr, const int32_t* irr_idx,
                       const int64_t* wsym, int want, abz_rule** out);

/* Symmetric rule built entirely on the device: orbit representatives, weights, the contraction plan of the node
 * list and the values, from the symmetry matrices syms [nsyms][d][d] (row-major integers, a group).  Same nodes,
 * weights and values as abz_symptr_rule + abz_ptr_rule_build, without the node list crossing PCIe twice; the integer
 * tables of a grid are cached per context (they do not depend on the series).
 * Replaces: the FourierMonkhorstPack constructor, which builds wsym / flags and fills the values in one go
 * (src/fourier.jl:265-277). */
int abz_ptr_rule_build_sym(abz_series* s, int npt, const int32_t* syms, int nsyms, int want,
                           abz_rule** out);

/* A slab of the full grid: only i_d in [outer_begin, outer_end) of the outermost variable (d >= 2),
 * i.e. one rank's share when a single solve is sharded over k (the recursion of fourier_ptr! is
 * independent per outer index, src/fourier.jl:148-164).  Weights and abz_rule_reduce's 1/npt^d
 * normalisation are those of the whole grid, so the partial sums of disjoint slabs add up to the
 * full rule value (one all-reduce).  A symmetric rule is sharded by passing a subset of
 * the irreducible nodes to abz_ptr_rule_build instead. */
int abz_ptr_rule_build_slab(abz_series* s, int npt, int outer_begin, int outer_end, int want,
                            abz_rule** out);
int abz_rule_destroy(abz_rule* r);
/* Re-evaluate every cached value of the rule from the series' current coefficients, in place and
 * without host synchronisation (launches only).  Replaces: the re-init of a stale cache,
 * solve!(::DOSCache) with isfresh (src/dos_interfaces.jl:104-109), and nextrule rebuilding a grid
 * (src/fourier.jl:315-321) when the buffers can be reused. */
int abz_rule_rebuild(abz_rule* r);
int abz_rule_info(const abz_rule* r, int64_t* nk, int* n, int* d, int* npt, int* want);
/* Copy rule contents to the host in the reference's layout (any pointer may be NULL):
 *   x [nk][d], w [nk] (1 on a full grid), H [nk][n*n][2], eig [nk][n], vel [nk][d][n]. */
int abz_rule_export(abz_rule* r, double* x, double* w, double* H, double* eig, double* vel);

/* Replaces: rule(f, B) = quadsum(AffineQuad(rule, B), f, vol/N) (src/fourier.jl:204-207,289-292)
 * for a built-in integrand, for n_sweep parameter values in one pass (batchsolve's omega sweep,
 * src/interfaces.jl:210-222, fused).  out_reim [n_sweep][ncomp][2] receives
 *   (sum_k w_k f(k, H(k); sweep_i)) / (npt^d * nsyms)        (nsyms = 1 on a full grid)
 * -- the caller applies |det B| and symmetrisation like do_solve_autobz (src/brillouin.jl:337-355).
 * By default (ABZ_PIVOT_NONE) DOS, TRGLOC and GLOC invert (omega + i eta) I - H(k) WITHOUT PIVOTING.  That is stable, with an
 * error of a modest multiple of eps sum_k ||G_k||^2 (||H_k|| + |z|) (times ||z - H_k|| / eta at worst), for a Hermitian series
 * with eta > 0 and for a dissipative series H = H_h - i Gamma, Gamma >= gamma I > 0, at eta >= 0; at eta = 0 a Hermitian
 * series needs omega in a gap AND definite leading blocks of omega I - H(k) (a diagonally dominant diag(+D, -D) + hopping has
 * them).  A series that is neither Hermitian nor dissipative, or a Hermitian one outside those conditions ([[0,1],[1,0]] at
 * omega = eta = 0), can lose every digit that way: set ABZ_PIVOT_PARTIAL on the series (abz_series_set_pivoting) and every
 * inverse pivots by rows like LAPACK's, tested against it within 64 eps sum_k ||G_k||^2 (||H_k|| + |z|) on such cases. */
int abz_rule_reduce(abz_rule* r, int integrand, const double* params, int nparams,
                    const double* sweep, int n_sweep, int nsyms, double* out_reim);

/* abz_rule_reduce without the host round trip: `sweep_dev` [n_sweep] and `out_dev_reim`
 * [n_sweep][ncomp][2] are DEVICE pointers, the call only enqueues work on the context's stream and returns.
 * This is the per-rank leg of a sharded sweep / of a k-sharded solve: the partial sums stay in HBM and go
 * straight into the RCCL all_gather / all_reduce (src/interfaces.jl:210-222's fan-in). */
int abz_rule_reduce_device(abz_rule* r, int integrand, const double* params, int nparams,
                           const double* sweep_dev, int n_sweep, int nsyms, double* out_dev_reim);
/* Device address and size in bytes of the rule's value block (tiled planar layout; with
 * ABZ_WANT_H_COMPACT the H planes of a tile are the n^2 upper-triangle planes in the order given at that flag):
 * zero-copy views for a device-side harness, and the placement log of bench.py. */
int abz_rule_values_ptr(const abz_rule* r, void** base, int64_t* nbytes);

/* Whole AutoPTR solve(s) inside the library: the p-adaptive loop of AutoSymPTR.autosymptr on the library's own integrands.
 * Replaces: do_solve(::FourierIntegrand, ::Basis, p, ::AutoSymPTRJL, cacheval) (src/fourier.jl:385-389, src/algorithms.jl:
 * 418-432) with its rule family (src/fourier.jl:296-321): I1 = rule(n0), I2 = rule(n0 + dn), err = norm(I2 - I1); while
 * err > max(abstol, reltol norm(I2)) and numevals < maxevals: I1 = I2, I2 = rule(next npt).  n0 / dn are the INTEGERS of
 * MonkhorstPackRule (defaults 50 / 50).  abstol < 0 / reltol < 0 mean `nothing` (both nothing: reltol = sqrt(eps)).
 * syms [nsyms][d][d] row-major (NULL: the full grid): symmetric rules with integer weights, dvol = 1 / (npt^d nsyms)
 * (src/fourier.jl:289-292); every rule value is multiplied by `value_factor` before the error is formed -- nsyms for the
 * TrivialRep symmetrisation inside a SymmetricRule (src/brillouin.jl:127-130), 1 otherwise.  The caller applies |det B|
 * (abstol / |det B| in, I |det B| out: src/brillouin.jl:429-444).
 * Rules of the first `keepmost` grids (the reference's `keepmost` = 2) stay with the series and serve every later call
 * (they refill themselves after abz_series_update); a larger grid is summed on the fly where the store-free kernel applies
 * and few values share it, otherwise built, scanned and dropped.  The first two grids are in flight together: a converged
 * solve with cached rules costs two scan launches and ONE stream synchronisation.
 * The _many form solves for n_sweep values of the swept parameter in lock-step (batchsolve, src/interfaces.jl:210-222):
 * each solve makes exactly the decisions it would make alone; a grid is visited once for all solves still active.
 * out_reim [n_sweep][ncomp][2], err [n_sweep] (norm(I2 - I1), nullable), numevals [n_sweep] (sum of the node counts of the
 * rules used, nullable), npt_last [n_sweep] (nullable). */
int abz_autoptr_solve(abz_series* s, const int32_t* syms, int nsyms, int integrand, const double* params, int nparams,
                      double sweep, int n0, int dn, double abstol, double reltol, int64_t maxevals, int keepmost,
                      double value_factor, double* out_reim, double* err, int64_t* numevals, int32_t* npt_last);
int abz_autoptr_solve_many(abz_series* s, const int32_t* syms, int nsyms, int integrand, const double* params, int nparams,
                           const double* sweeps, int n_sweep, int n0, int dn, double abstol, double reltol,
                           int64_t maxevals, int keepmost, double value_factor, double* out_reim, double* err,
                           int64_t* numevals, int32_t* npt_last);
/* Drop the rules the series keeps for abz_autoptr_solve* (they are also dropped by abz_series_destroy). */
int abz_series_drop_rules(abz_series* s);

/* Store-free rule value: the same number as abz_rule_reduce on the full grid (or on the slab
 * [outer_begin, outer_end) of its outermost variable), computed without materialising H(k): the
 * Fourier evaluation feeds the integrand directly and only the sums leave the kernel.  For grids that are
 * used once (an AutoPTR refinement step) or do not fit in HBM (1000^3 k-points = 168 GB of rule values).
 * DOS, TRGLOC and GLOC: every series and grid up to ABZ_MAX_BANDS bands (Hermitian series: closed forms up to 4 bands on lines of
 * more than 128 points, the tridiagonal form of every node above; GLOC above 4 bands, series that are not Hermitian and short
 * lines: the inverse of every node, chunk by chunk).  Other integrands: Hermitian series of n <= 4 bands with npt > 128;
 * ABZ_ERR_UNSUPPORTED otherwise (build a rule instead).
 * By default the resolvents are inverted without pivoting, as in abz_rule_reduce, and the same cases are covered; with
 * ABZ_PIVOT_PARTIAL on the series every node's inverse pivots by rows (1...64 bands, every series, lines of < 65536 points).
 * Replaces: FourierPTR ctor + rule(f, B) back to back (src/fourier.jl:166-207). */
int abz_ptr_sum(abz_series* s, int npt, int outer_begin, int outer_end, int integrand,
                const double* params, int nparams, const double* sweep, int n_sweep, int nsyms,
                double* out_reim);

/* Replaces: sum_ggr / ggr_formula (src/dos_ggr.jl:58-104) for nE energies; rule must hold VEL. */
int abz_rule_ggr(abz_rule* r, const double* E, int nE, double* out);

/* Linear tetrahedron method (Bloechl, Jepsen, Andersen, PRB 49, 16223) on the eigenvalues of a
 * full-grid rule (needs ABZ_WANT_EIG; velocities not needed).  The periodic grid's cells are cut into d! simplices by the
 * Kuhn split, band b of a simplex is the b-th ascending eigenvalue at each corner.  out [nE] receives, per unit cell and
 * summed over bands, the density of states g(E) (what = ABZ_LTM_DOS, integral over E = n) or the number of states below
 * E (ABZ_LTM_STATES, n above all bands, exactly 0 below them).  Rules that are not a whole periodic grid (irreducible
 * nodes, symmetric rules, slabs) return ABZ_ERR_UNSUPPORTED; a slab is taken once abz_rule_ltm_halo gave it its halo plane.  The curvature correction of the paper (eq. 22) of an
 * unweighted count is zero, so `what` is one of these two here and ABZ_LTM_STATES_CORRECTED (abz_rule_ltm_weighted) is
 * refused with ABZ_ERR_ARG.
 * Replaces: nothing yet -- the reference plans "LTM" (src/dos_algorithms.jl:1-7); entry point added without a change
 * of ABZ_VERSION. */
#define ABZ_LTM_DOS 0
#define ABZ_LTM_STATES 1
int abz_rule_ltm(abz_rule* r, const double* E, int nE, int what, double* out);

/* Tetrahedron method with matrix elements, and the Fermi level.  The same whole periodic grids as abz_rule_ltm, the same
 * refusals (ABZ_ERR_UNSUPPORTED for slabs and irreducible nodes, ABZ_ERR_ARG without eigenvalues).
 * Replaces: nothing yet -- the reference plans LTM for "any function or H_R" (src/dos_algorithms.jl:5-7). */
#define ABZ_LTM_MAX_COMP 16
/* Attach matrix elements to a full-grid rule that holds eigenvalues: A [ncomp][nk][n] host doubles, node order and band
 * order those of abz_rule_export's eig [nk][n] (i_1 fastest, bands ascending).  They stay resident in HBM in the layout of the
 * eigenvalue planes until replaced, dropped (A = NULL, ncomp = 0), abz_rule_rebuild (they described the old eigenstates) or
 * abz_rule_destroy. */
int abz_rule_ltm_elements(abz_rule* r, const double* A, int ncomp);
/* Orbital weights as LTM matrix elements, computed on the device: component c, band b, node k gets
 * |U_{orb[c], b}(k)|^2, U(k) = orthonormal eigenvectors of Hermitian(H(k)) (upper triangle), bands ascending as in
 * the rule's eigenvalue planes.  orb == NULL: all n orbitals (norb ignored, n <= ABZ_LTM_MAX_COMP).  The result is
 * attached exactly like abz_rule_ltm_elements would attach it (replaces what was attached; dropped by the same events).
 * 1...32 bands, Hermitian series.  H(k) is read from the rule when it holds it (either layout), else from a transient rule of
 * the series' CURRENT coefficients that lives for the call: rebuild a stale rule first.  At a degenerate level the weights
 * are those of some orthonormal basis of the eigenspace: their sum over the level and sum_a = sum_b = 1 are defined, no more.
 * ABZ_ERR_UNSUPPORTED: not a whole periodic grid, a rule of abz_rule_ltm_unfold, more than 32 bands.  ABZ_ERR_ARG: no
 * eigenvalues, norb outside 1..ABZ_LTM_MAX_COMP, an index outside 0..n-1 (duplicates are fine), orb == NULL with
 * n > ABZ_LTM_MAX_COMP, a series that is not Hermitian.  A refusal or failure leaves attached elements as they were. */
int abz_rule_ltm_orbitals(abz_rule* r, const int32_t* orb, int norb);
/* Band projectors as LTM matrix elements, computed on the device like the orbital weights and attached like them:
 * P^b_pq(k) = U_pb(k) conj(U_qb(k)), which no phase of an eigenvector changes.  Pair i = (pairs[2i], pairs[2i+1]) = (p, q) takes
 * one component for p == q, |U_pb|^2 (the planes of abz_rule_ltm_orbitals, bit for bit), and two consecutive ones for p != q,
 * Re P^b_pq = ur_p ur_q + ui_p ui_q, then Im P^b_pq = ui_p ur_q - ur_p ui_q; components follow the order of the pairs.  With
 * them abz_rule_ltm_green_weighted returns G_{Re P}(z) and G_{Im P}(z), and the local Green's function is
 *      G_pq(z) = sum_b int dk P^b_pq(k) / (z - e_b(k)) = G_{Re P}(z) + i G_{Im P}(z),   G_qp(z) = G_{Re P}(z) - i G_{Im P}(z).
 * At a degenerate level single projectors are those of some orthonormal basis of the eigenspace; their sum over the level,
 * sum_b P^b_pq = delta_pq and sum_b e_b P^b_pq = H_pq(k) are defined.  Rules, H(k), refusals and what a refusal leaves in place:
 * as abz_rule_ltm_orbitals.  ABZ_ERR_ARG also for pairs == NULL, npairs < 1, an index outside 0..n-1, more than
 * ABZ_LTM_MAX_COMP components in all (attach them in groups).  Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_projectors(abz_rule* r, const int32_t* pairs /* [npairs][2] */, int npairs);
/* Band expectation values of operator series as LTM matrix elements, computed on the device like the orbital weights and
 * attached like them (replaces what was attached; dropped by the same events).  For operator i, band b and node k:
 *      q_i = Re u_b(k)^H Hermitian(O_i(k)) u_b(k),   O_i(k) = sum_R e^{2 pi i k.R} O_{i,R} in the Wannier basis of H,
 * the upper triangle of O_i read the way H is read, u_b the eigenvector the orbital and projector kernels use, bands ascending
 * as in the rule's eigenvalue planes.  Component c with comps[c] = (i, j) is q_i for j == -1 and the product q_i q_j for
 * 0 <= j < nops; comps == NULL: the nops expectations in order (ncomp = nops, the argument is ignored).  1 <= ncomp <=
 * ABZ_LTM_MAX_COMP; duplicates are fine.  With O = S_z: the spin-resolved DOS; with O_a = dH/dk_a and products: the transport
 * distribution sum_b int dk v_a v_b delta(E - e_b) from abz_rule_ltm_weighted.
 * r: what abz_rule_ltm_orbitals takes (a whole periodic grid with eigenvalues, 1...32 bands, a Hermitian series, not a rule of
 * abz_rule_ltm_unfold); H(k) from its own planes or a transient rule, as there.  ops[i]: rules that hold H planes (full or
 * Hermitian-compact) of Hermitian series on whole periodic grids of the same context, npt, d and n as r; ops[i] == r is allowed
 * when r holds H.  The caller keeps them current (abz_rule_rebuild after abz_series_update).
 * At a degenerate level single expectations belong to some orthonormal basis of the eigenspace: only their sum over the level
 * is defined, and products are not defined there at all.
 * ABZ_ERR_UNSUPPORTED: slabs, node lists, symmetric rules, rules of abz_rule_ltm_unfold, more than 32 bands, the row-major
 * layout.  ABZ_ERR_ARG: a NULL pointer, nops outside 1..ABZ_LTM_EXPECT_MAX_OPS, ncomp outside 1..ABZ_LTM_MAX_COMP, an operator
 * index out of range, mismatched geometry or context, an operator without H planes, an operator series that is not Hermitian,
 * r without eigenvalues.  Nothing is reserved or launched on a refusal; a refusal or failure leaves attached elements as they
 * were.  Entry point added without a change of ABZ_VERSION. */
#define ABZ_LTM_EXPECT_MAX_OPS 8
int abz_rule_ltm_expectation(abz_rule* r, abz_rule* const* ops, int nops, const int32_t* comps /* [ncomp][2] or NULL */, int ncomp);
/* Attached elements back to the host: *ncomp (0 if none), and, if A != NULL, A [ncomp][nk][n] in the order
 * abz_rule_ltm_elements takes them. */
int abz_rule_ltm_elements_export(abz_rule* r, int* ncomp, double* A);
/* The resident element block as it lies on the device: *base (NULL if nothing is attached), *nbytes and *ncomp; any pointer may
 * be NULL.  Layout: double [ntiles][ncomp * nb planes][row], ntiles = nk / npt grid lines, plane c * nb + b = component c of band
 * b (nb: abz_rule_ltm_bands), row = npt rounded up to a multiple of 16; the padding columns npt .. row-1 hold zeros.  The address
 * is valid until the elements are replaced or dropped.  Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_elements_ptr(const abz_rule* r, void** base, int64_t* nbytes, int* ncomp);
#define ABZ_LTM_A_ELEMENTS 0   /* the attached elements, ncomp components */
#define ABZ_LTM_A_ENERGY 1     /* A_b(k) = e_b(k) itself, 1 component, nothing attached needed */
/* out [nE][ncomp]: g_A(E) (ABZ_LTM_DOS) or N_A(E) (ABZ_LTM_STATES), per unit cell, summed over bands; A is interpolated
 * linearly inside each simplex like the band energy.
 * ABZ_LTM_STATES_CORRECTED: N_A(E) with Bloechl's curvature correction, for both sources and in the same launches:
 *   N_A^corr(E) = N_A(E) + w sum_T g_T(E) kappa_T,   kappa_T = f_d sum_i A_i (sum_l e_l - (d+1) e_i),   f_d = 1 / (2 (d+1)(d+2))
 * over the simplices T with e_1 <= E < e_{d+1}, g_T the simplex's own DOS, w = 1 / (d! npt^d); f_3 = 1/40 is eq. 22 of
 * the paper, f_2 = 1/24, f_1 = 1/12.  It removes the leading O(1/npt^2) error of a sum taken at FIXED FILLING, i.e. at
 * the Fermi level of the same grid (abz_rule_ltm_fermi: for A = 1 the correction vanishes, the level has none); at a
 * fixed energy the misplaced Fermi surface leaves an error of the same order (abz_rule_ltm_optimized below has no such limit).
 * Any other `what`: ABZ_ERR_ARG. */
#define ABZ_LTM_STATES_CORRECTED 2
int abz_rule_ltm_weighted(abz_rule* r, int source, const double* E, int nE, int what, double* out);
/* Fermi level: E_F with N(E_F) >= nstates (1 - 1e-12) and N(E) below that for every sampled E <= E_F - tol;
 * 0 < nstates < n.  N_F (nullable) receives N(E_F).  Below a gap (g = 0 exactly from some energy on while N is still
 * nstates to 1e-12) E_F is moved up to the lowest energy with g(E_F) = 0, the top of the band, to within tol. */
int abz_rule_ltm_fermi(abz_rule* r, double nstates, double tol, double* E_F, double* N_F);
/* Full-grid eigenvalue rule filled from the irreducible nodes of `src` (built with ABZ_WANT_EIG by abz_ptr_rule_build_sym or
 * from an explicit node list) under syms [nsyms][d][d]: node x of the grid gets the eigenvalues of the node of `src` in its
 * orbit.  *out == NULL: creates the rule; *out != NULL (a rule this function made for the same src geometry): gathers again
 * into it, reusing its orbit map -- what a caller does after abz_rule_rebuild(src).
 * The map addresses the nodes of `src` by their position in its list: a refresh must come with the same symmetries (checked)
 * and a source whose nodes stand in the same ORDER as when the map was made (only their count is checked) -- the same handle
 * rebuilt, or a rule built the same way.
 * The symmetries must be symmetries of H, H(S k) = H(k) up to a unitary: then e_b(S k) = e_b(k) and the gather is exact.  The
 * result is a whole periodic grid with eigenvalues only: abz_rule_ltm, _elements, _weighted, _fermi, abz_rule_export (x, w,
 * eig), abz_rule_info and abz_rule_destroy take it like a rule of abz_ptr_rule_build(s, npt, 0, NULL, NULL, ABZ_WANT_EIG, ...);
 * abz_rule_rebuild answers ABZ_ERR_UNSUPPORTED (rebuild src and unfold again; that drops attached matrix elements).  It
 * keeps its series alive and does not hold `src`.  ABZ_ERR_ARG: src without eigenvalues, nsyms < 1 or syms NULL, *out not
 * an unfolded rule of the same series, npt, node count and symmetries, or a node list that does not hold a node of every orbit (the
 * message counts the uncovered points).  ABZ_ERR_UNSUPPORTED: src is a full grid or a slab, or npt^d >= 2^31.  Costs 4 B
 * per grid point for the orbit map beside the n planes. */
int abz_rule_ltm_unfold(abz_rule* src, const int32_t* syms, int nsyms, abz_rule** out);
/* Pair rules: joint density of states and interband spectra from the scans above.
 * The difference of two linearly interpolated bands is linear in a simplex, so Delta_p(k) = e_c(k) - e_v(k) of a lower band v and an
 * upper band c is a pseudo-band the tetrahedron scans treat exactly like a band.  abz_rule_ltm_pairs makes, from the lower range
 * [v0, v0 + nv) and the upper range [c0, c0 + nc) of the ascending bands of `src` (0 <= v0, nv >= 1, nc >= 1, v0 + nv <= c0,
 * c0 + nc <= n, nv nc <= ABZ_MAX_BANDS), a whole periodic grid of nb = nv nc pseudo-bands p = (v - v0) nc + (c - c0), want =
 * ABZ_WANT_EIG.  An insulator with nocc filled bands is (0, nocc, nocc, n - nocc); a model of many bands takes a window around the
 * gap.  On the result
 *      abz_rule_ltm                     J(w)    = sum_vc int dk delta(w - Delta_vc)                    (and its cumulative)
 *      abz_rule_ltm_weighted            S_ij(w) = sum_vc int dk M^i_vc conj(M^j_vc) delta(w - Delta_vc) (cumulative, corrected)
 *      abz_rule_ltm_green[_weighted]    sum_vc int dk M M^* / (z - Delta_vc): -Im / pi the broadened spectrum, Re its Kramers-Kronig partner
 * and abz_rule_ltm_elements, _elements_export, _fermi, _node_weights(+ _ptr, _dot), _green_node_weights(+ _ptr, _dot) and
 * abz_rule_export (x, w, eig [nk][nb]) work unchanged: they size themselves by abz_rule_ltm_bands, which is n for every other
 * rule.  With O = dH/dk, S is the absorptive part of the optical conductivity up to prefactors and 1 / w.
 * Energies: Delta = e_c - e_v, one subtraction per node from the eigenvalue planes of `src` as they are (never from another
 * eigen-solve): the spectra sit on the eigenvalues the scans of `src` see.
 * nops == 0: ops, comps and ncomp are ignored, the result has energies only, nothing with eigenvectors is launched; src is any
 * whole grid abz_rule_ltm takes (1...64 bands, rules of abz_rule_ltm_unfold included).
 * 1 <= nops <= ABZ_LTM_PAIRS_MAX_OPS: src and ops[i] are what abz_rule_ltm_expectation takes (src: 2...32 bands, a Hermitian
 * series, a whole grid that was not unfolded, H(k) from its own planes or a transient rule of the series' CURRENT coefficients;
 * ops[i]: H planes of Hermitian series of the same context, npt, d, n, not row-major).  Component (i, j, part) = comps[c][0..2] is
 * Re (part 0) or Im (part 1) of M^i_vc conj(M^j_vc), M^i_vc = u_v^H Hermitian(O_i) u_c, which the phases of u_v and u_c do not
 * change; comps == NULL: the nops components |M^i_vc|^2 (ncomp = nops).  1 <= ncomp <= ABZ_LTM_MAX_COMP; duplicates are fine.  The
 * block is attached to the result as abz_rule_ltm_elements would attach it ([ncomp][nk][nb]).
 * *out == NULL: a new rule; it holds its own reference on the series and does not depend on src afterwards.  *out != NULL: a pair
 * rule of the same series, npt, ranges, operator count and components, filled again in place -- the call to make after
 * abz_rule_rebuild(src); its weight blocks are dropped (they described the old energies).  Energies and elements are complete
 * before they replace anything: a refusal or failure leaves *out, src and every attached block as they were.
 * Degenerate levels: u_v, u_c are some orthonormal bases of their eigenspaces; only the SUM of a component over all pairs between
 * two levels is defined (it is what a scan adds up, since those pairs share Delta).
 * The scans above take whole bands; partial occupations (the factor f_v (1 - f_c) of a metal restricts each simplex to its occupied
 * part) are what abz_rule_ltm_pairs_occupied below adds at T = 0.
 * Not handled: weights Delta^-m inside the elements (divide exported elements by exported energies and attach them
 * with abz_rule_ltm_elements), the Berry-connection term of the Wannier velocity (operators are what the caller passes), 33...64
 * bands with operators, slabs, more than ABZ_MAX_BANDS pairs per rule.
 * A pair rule has no H(k), eigenvectors or plan: abz_rule_ltm_orbitals, _projectors, _expectation, _density_matrix,
 * _green_node_weights_matrix, _halo, abz_rule_rebuild, abz_rule_reduce and abz_rule_ltm_pairs with a pair rule as src answer
 * ABZ_ERR_UNSUPPORTED, launch nothing and leave it as it was.
 * ABZ_ERR_ARG: range errors, one band with operators, nops outside 0..ABZ_LTM_PAIRS_MAX_OPS, ncomp outside 1..ABZ_LTM_MAX_COMP, an
 * index or part out of range, NULL pointers, *out not a matching pair rule, the operator errors of abz_rule_ltm_expectation.
 * ABZ_ERR_UNSUPPORTED: slabs, node lists, with operators more than 32 bands or an unfolded src.  Kernels: the energies under
 * ABZ_K_LTM, the elements under ABZ_K_EIG.  Entry points added without a change of ABZ_VERSION. */
#define ABZ_LTM_PAIRS_MAX_OPS 4
int abz_rule_ltm_pairs(abz_rule* src, int v0, int nv, int c0, int nc, abz_rule* const* ops, int nops,
                       const int32_t* comps /* [ncomp][3] or NULL */, int ncomp, abz_rule** out);
/* Interband spectra of a metal: the scans of a pair rule with the T = 0 occupation factor inside every simplex,
 *      J^occ(w)    = sum_vc int dk theta(E_F - e_v) theta(e_c - E_F) delta(w - Delta_vc)                    (ABZ_LTM_A_ONE)
 *      S^occ_ij(w) = sum_vc int dk theta(E_F - e_v) theta(e_c - E_F) M^i_vc conj(M^j_vc) delta(w - Delta_vc)  (ABZ_LTM_A_ELEMENTS)
 * for what = ABZ_LTM_DOS, and with theta(w - Delta_vc) in place of delta for ABZ_LTM_STATES; out [nw][ncomp], ncomp = 1 for
 * ABZ_LTM_A_ONE.  `pairs` is a rule of abz_rule_ltm_pairs, `src` the whole grid it was made from (same series and npt, at least
 * c0 + nc bands; a rule of abz_rule_ltm_unfold is fine: only its eigenvalues are read, as they are now -- after abz_rule_rebuild(src)
 * fill the pair rule again first).  Inside a simplex e_v, e_c and Delta are linear, so the occupied region is the simplex cut by two
 * planes; it is split into sub-simplices of non-negative volume (at most 1, 2 x 2, 3 x 3 for d = 1, 2, 3) and each goes through the
 * closed forms of abz_rule_ltm_weighted with interpolated corner values, weight 1 / (d! npt^d) per simplex as everywhere.
 * Ties follow the half-open rule of the scans (N(E) counts e <= E): a corner is occupied iff e_v <= E_F and empty iff e_c > E_F.
 * E_F is the caller's (abz_rule_ltm_fermi on src gives the grid's own).  Nothing is attached, replaced or dropped on either rule.
 * Not handled: finite temperature, the broadened (Green's function) form with occupations, node weights of the cut, slabs, and
 * Bloechl's correction: ABZ_LTM_STATES_CORRECTED answers ABZ_ERR_UNSUPPORTED (the curvature correction is not defined on cut
 * simplices).
 * ABZ_ERR_ARG: NULL pointers, nw < 1, `pairs` not a pair rule, another `what` or `source`, rules of different series or npt, an upper
 * range outside the bands of src, ABZ_LTM_A_ELEMENTS without elements on `pairs`, E_F not finite, src without eigenvalues.
 * ABZ_ERR_UNSUPPORTED: src a slab, a node list or a pair rule.  A refusal launches nothing and leaves both rules as they were.
 * Kernels under ABZ_K_LTM.  Entry point added without a change of ABZ_VERSION. */
#define ABZ_LTM_A_ONE 2   /* A = 1: the joint DOS of abz_rule_ltm_pairs_occupied; g and N of abz_rule_ltm_optimized */
int abz_rule_ltm_pairs_occupied(abz_rule* src, abz_rule* pairs, double E_F, int source, const double* w, int nw, int what,
                                double* out /* [nw][ncomp], ncomp = 1 for A_ONE */);
/* *nb: bands of the rule's eigenvalue planes, attached elements and weight blocks: nv nc of a pair rule, n of any other.
 * abz_rule_info keeps reporting the series' n (the bands of the source) for a pair rule: size the buffers of abz_rule_export's
 * eig, abz_rule_ltm_elements(_export) and the node weights by *nb, not by that n. */
int abz_rule_ltm_bands(const abz_rule* r, int* nb);
/* Optimized tetrahedron method (Kawamura, Gohda, Tsuneyuki, PRB 89, 094515 (2014)), d = 3: the sums of abz_rule_ltm and
 * abz_rule_ltm_weighted without the leading O(1/npt^2) error of linear interpolation, at any energy, from the same eigenvalue
 * planes and with no further eigen-solve.  A Kuhn simplex of cell i is the path v1 = i, v2 = v1 + e_a, v3 = v2 + e_b, v4 = v3 + e_c
 * over a permutation (a, b, c) of the axes.  The band is taken at the 20 grid points
 *      p1..p4   = v1..v4
 *      p5..p16  = 2 v_i - v_j,  (i, j) = (1,2) (2,3) (3,4) (4,1) (1,3) (2,4) (3,1) (4,2) (1,4) (2,1) (3,2) (4,3)
 *      p17..p20 = v4 - v1 + v2,  v1 - v2 + v3,  v2 - v3 + v4,  v3 - v4 + v1
 * (indices mod npt, any npt >= 1), the cubic through the 20 values is fitted, and the 4 corner values are replaced by those of the
 * linear function closest to it in the least-squares sense over the simplex, x'_m = sum_j P[m][j] x(p_j); P is 4 x 20 with rows
 * summing to 1 (DESIGN section 4e has 1260 P).  For band b, x is the b-th ascending eigenvalue at each point; elements A_b take
 * the same P at the same points.  The closed forms of abz_rule_ltm_weighted then apply to (e'; A'), weight 1 / (6 npt^3) per
 * simplex; a simplex wholly below E counts 1, or the mean of its A'.
 * source: ABZ_LTM_A_ONE (g, N: one component), ABZ_LTM_A_ENERGY (A = e, one component) or ABZ_LTM_A_ELEMENTS (the attached
 * block).  what: ABZ_LTM_DOS or ABZ_LTM_STATES.  out [nE][ncomp] and the energy list as for abz_rule_ltm_weighted (any order,
 * results in the caller's order).  N is n above all bands and exactly 0 below them; a flat band gives g = 0 and a unit step; two
 * calls return the same bits.  The rule is a whole periodic 3-d grid; rules of abz_rule_ltm_unfold and of abz_rule_ltm_pairs are
 * taken where abz_rule_ltm_weighted takes them.
 * ABZ_ERR_ARG: NULL pointers, nE < 1, another `what` -- ABZ_LTM_STATES_CORRECTED too: this rule replaces the correction --,
 * another `source`, ABZ_LTM_A_ELEMENTS with nothing attached, a rule without eigenvalues.  ABZ_ERR_UNSUPPORTED: d != 3, a slab
 * (with or without its halo: the stencil needs three planes around it), a list of irreducible nodes.  A refusal launches nothing
 * and leaves `out` and the rule as they were.  Not handled: d = 1, 2, slabs, node weights, occupied pair scans (the Green's
 * functions: abz_rule_ltm_green_optimized below).  Kernels under ABZ_K_LTM.  Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_optimized(abz_rule* r, int source, const double* E, int nE, int what, double* out);
/* Tetrahedron scans on a slab: attach the halo plane.  r: a rule of abz_ptr_rule_build_slab over [outer_begin, outer_end) that
 * holds eigenvalues (other `want` bits are fine).  The simplices of the cells of the slab's last plane reach into plane
 * outer_end mod npt; this builds that one plane, eigenvalues only, with the builder of the slab itself (1 / npt of the grid, no
 * exchange between ranks) and hands it to r: it is freed by abz_rule_destroy(r), counted by abz_mem_info, refilled by a second
 * call and by abz_rule_rebuild(r) (same call, same stream), and is not a rule of its own to the caller.
 * With the halo, abz_rule_ltm (DOS, STATES) and abz_rule_ltm_weighted with ABZ_LTM_A_ENERGY (DOS, STATES, STATES_CORRECTED)
 * take the slab and return its PARTIAL sum: the sum over the cells whose outermost index lies in [outer_begin, outer_end), every
 * simplex with the whole grid's weight 1 / (d! npt^d).  The partial sums of the slabs of a partition of [0, npt) add up to the
 * whole grid's value; N is exactly 0 below the bands on every slab.  Everything else keeps refusing slabs with
 * ABZ_ERR_UNSUPPORTED, halo or not: ABZ_LTM_A_ELEMENTS, abz_rule_ltm_elements, _orbitals, _projectors, _elements_export, _fermi,
 * _unfold.
 * ABZ_ERR_ARG: a whole periodic grid (nothing to attach), a rule without eigenvalues.  ABZ_ERR_UNSUPPORTED: a node list or
 * symmetric rule, a rule of abz_rule_ltm_unfold.  A refusal or failure leaves r as it was.  Entry point added without a
 * change of ABZ_VERSION. */
int abz_rule_ltm_halo(abz_rule* r);
/* Trace of the Green's function at complex energies by the tetrahedron method: out[i] = tr G(z_i),
 *      tr G(z) = w sum_{cells} sum_{d! simplices} sum_{bands} J[x_0 .. x_d](z),   w = 1 / (d! npt^d),
 * per unit cell and summed over bands, on the mesh, weights and band convention of abz_rule_ltm, so that
 * -Im tr G(E + i0) / pi -> g(E) of abz_rule_ltm and z tr G(z) -> n as |z| -> inf.  J[x_0 .. x_m](z) is the mean of 1 / (z - e)
 * over a simplex in which e is linear with the sorted corner values x_0 <= .. <= x_m; with u_i = z - x_i:
 *      m = 0: 1 / u_0;   m = 1: (log u_0 - log u_1) / (x_1 - x_0), principal logs;
 *      m >= 2: J[x_0..x_m] = m / (m-1) (u_0 J[x_0..x_{m-1}] - u_m J[x_1..x_m]) / (x_m - x_0).
 * Evaluation rule: a sub-range x_i..x_j with x_j - x_i < rho |z - mean|, rho = 1/2, is summed by its Taylor series about the
 * mean, sum_k m! k! / (m+k)! h_k(x - mean) / (z - mean)^(k+1) (h_k: complete homogeneous symmetric polynomial), truncated where
 * (max |x_l - mean| / |z - mean|)^k < 2^-52, at most 37 terms; only wider sub-ranges recurse, so nothing is divided by a width
 * below rho |z - mean|, and equal corners give 1 / u.  The error is the interpolation error O(1 / npt^2) whatever Im z is.
 * Im z < 0 is computed as the conjugate of the value at conj(z): tr G(conj z) == conj(tr G(z)) to the bit.  No floating-point
 * atomics: two calls return the same bits.
 * Takes the whole periodic grids abz_rule_ltm takes (full-grid rules and rules of abz_rule_ltm_unfold, 1...64 bands, d = 1...3).
 * ABZ_ERR_UNSUPPORTED: slabs, with or without a halo; lists of irreducible nodes; symmetric rules.  ABZ_ERR_ARG: a rule without
 * eigenvalues, nz < 1, a NULL pointer, any Im z == 0 or non-finite z.  Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_green(abz_rule* r, const double* z /* [nz][2]: re, im */, int nz, double* out /* [nz][2] */);

/* The same with matrix elements: G_A,c(z) = sum_b int dk A_{c,b}(k) / (z - e_b(k)) of every component c, per unit cell, e and A
 * linear inside each simplex; with the orbital weights |U_ab|^2 of abz_rule_ltm_orbitals attached, the diagonal G_aa(z) of the
 * local Green's function.  `source` as in abz_rule_ltm_weighted: ABZ_LTM_A_ENERGY (one component, A = e) or ABZ_LTM_A_ELEMENTS
 * (what abz_rule_ltm_elements / abz_rule_ltm_orbitals attached, at most ABZ_LTM_MAX_COMP components).  out [nz][ncomp][2].
 *      G_A,c(z) = w sum_{cells} sum_{d! simplices} sum_{bands} sum_{i=0..d} A_{c,i} W_i(z),   W_i = J[x_0 .. x_d, x_i](z) / (d + 1):
 * the mean of lambda_i / (z - e) over a simplex is the J above with the knot x_i doubled (the recursion holds for repeated knots,
 * J[x, x] = 1 / u).  The same evaluation rule, rho = 1/2, now on up to five knots: at most 39 terms of the series.  The d + 1
 * weights of a (simplex, z) are formed once per group of components (4s, then a 2, then a 1) and every component contracts with
 * them.  sum_i W_i = J and sum_i x_i W_i = z J - 1: elements == 1 give the trace, ABZ_LTM_A_ENERGY gives z tr G(z) - n.
 * Im z < 0: the conjugate of the value at conj(z), to the bit.  No floating-point atomics: two calls return the same bits.
 * Takes the rules abz_rule_ltm_green takes.  ABZ_ERR_UNSUPPORTED: slabs, with or without a halo; lists of irreducible nodes;
 * symmetric rules.  ABZ_ERR_ARG: a `source` that is neither, ABZ_LTM_A_ELEMENTS with nothing attached, a rule without
 * eigenvalues, nz < 1, a NULL pointer, any Im z == 0 or non-finite z; nothing is reserved, launched or written then.
 * Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_green_weighted(abz_rule* r, int source, const double* z /* [nz][2] */, int nz, double* out /* [nz][ncomp][2] */);

/* The Green's functions of the optimized tetrahedron method, d = 3: abz_rule_ltm_green and abz_rule_ltm_green_weighted on the
 * effective corner values of abz_rule_ltm_optimized, so that -Im tr G(E + i eta) / pi tends to the g(E) of abz_rule_ltm_optimized as
 * eta -> 0 and the error at npt compares with the linear rule's at 2 npt whatever eta is.  For every cell, Kuhn simplex and band b:
 * e'_m = sum_j P[m][j] e_b(p_j) and A'_{c,m} = sum_j P[m][j] A_{c,b}(p_j) over the 20 stencil points (the same P, points and wrap
 * mod npt, any npt >= 1; the band index is followed).  Then
 *      tr G(z)  = w sum_{cells} sum_{6 simplices} sum_{bands} J[sort(e'_1 .. e'_4)](z),       w = 1 / (6 npt^3)
 *      G_A,c(z) = w sum ... sum_{i=0..3} A'_{c,i} W_i(z),                                     W_i = J[x_0 .. x_3, x_i](z) / 4
 * by the evaluation rule of abz_rule_ltm_green (rho = 1/2, Taylor series for narrow sub-ranges, principal logs of one half plane).
 * source: ABZ_LTM_A_ONE (the trace, ncomp = 1, nothing loaded), ABZ_LTM_A_ENERGY (A' = e', one component: z tr G(z) - n) or
 * ABZ_LTM_A_ELEMENTS (the attached block, in groups of 4, 2, 1 components).  out [nz][ncomp][2].  Im z < 0: the conjugate of the
 * value at conj(z), to the bit.  No floating-point atomics: two calls return the same bits.  A flat band gives 1 / (z - e).
 * Takes full-grid rules and rules of abz_rule_ltm_unfold.  ABZ_ERR_ARG: NULL pointers, nz < 1, any Im z == 0 or non-finite z,
 * another `source`, ABZ_LTM_A_ELEMENTS with nothing attached, a rule without eigenvalues.  ABZ_ERR_UNSUPPORTED: d != 3; slabs, with
 * or without a halo; lists of irreducible nodes; pair rules of abz_rule_ltm_pairs (e'_c - e'_v has not been looked at).  A refusal
 * launches nothing and leaves `out` and the rule as they were.  Not handled: the node-weight forms W_b(k; z), the local matrix
 * G_pq(z) other than through attached projectors, d < 3.  Kernels under ABZ_K_LTM.  Entry point added without a change of
 * ABZ_VERSION. */
int abz_rule_ltm_green_optimized(abz_rule* r, int source, const double* z /* [nz][2] */, int nz, double* out /* [nz][ncomp][2] */);

/* Bloechl's integration weights themselves, per grid point and band: the numbers w_b(k; E) with
 *      N_A(E) = sum_k sum_b w_b(k; E) A_b(k)     (ABZ_LTM_STATES; likewise g_A with ABZ_LTM_DOS and the corrected N_A with
 *                                                 ABZ_LTM_STATES_CORRECTED)
 * for ANY A on the mesh, band convention, half-open regions and simplex weight 1 / (d! npt^d) of abz_rule_ltm: what
 * abz_rule_ltm_weighted forms inside its scan and contracts at once.  The weight of node k is the sum, over the (d+1)! Kuhn
 * simplices that contain k (2, 6 or 24: their corners are the 3^d neighbours k + {-1,0,1}^d, indices wrapped mod npt), of what
 * the simplex gives that corner.  ABZ_LTM_STATES: a simplex wholly below E gives 1 / (d+1) to each corner, so a node whose whole
 * neighbourhood lies below E weighs 1 / npt^d and one whose neighbourhood lies above E exactly 0.0; ABZ_LTM_DOS: a flat simplex
 * gives nothing; ABZ_LTM_STATES_CORRECTED: plus g_T(E) f_d (sum_l e_l - (d+1) e_k) per simplex inside its window, kappa_T of
 * abz_rule_ltm_weighted split by corner (the block then sums to N(E): the correction of A = 1 is zero).
 * E [nE], 1 <= nE <= ABZ_LTM_NODEW_MAX_E, in any order, duplicates allowed.  out [nE][nk][n] (or NULL: nothing is copied) is in
 * the node and band order of abz_rule_export's eig, as abz_rule_ltm_elements takes elements.  A gather without atomics: two calls
 * write the same bits.
 * The weights stay resident in HBM, nE n planes tiled like an element block of abz_rule_ltm_elements (plane i n + b of a grid
 * line's tile: band b at E[i]; padding columns zero), until the next call replaces them, abz_rule_rebuild or a new gather of
 * abz_rule_ltm_unfold (they described the old eigenvalues), or abz_rule_destroy; attaching or dropping ELEMENTS leaves them
 * alone: attach, dot, attach, dot costs one pass over memory each.  They are counted by abz_mem_info.
 * Takes full-grid rules and rules of abz_rule_ltm_unfold, d = 1...3, 1...64 bands.  ABZ_ERR_UNSUPPORTED: slabs, with or without
 * a halo (a node needs the plane BEFORE it as well), lists of irreducible nodes, symmetric rules.  ABZ_ERR_ARG: a rule without
 * eigenvalues, E == NULL, nE outside 1..ABZ_LTM_NODEW_MAX_E, a non-finite energy, a `what` that is none of the three.  A refusal
 * or failure leaves the resident weights as they were.  Entry points added without a change of ABZ_VERSION. */
#define ABZ_LTM_NODEW_MAX_E 16
int abz_rule_ltm_node_weights(abz_rule* r, const double* E, int nE, int what, double* out /* [nE][nk][n] or NULL */);
/* The resident weights: device address, bytes and energies of the block; NULL, 0, 0 when the rule holds none (any of the three
 * pointers may be NULL). */
int abz_rule_ltm_node_weights_ptr(const abz_rule* r, void** base, int64_t* nbytes, int* nE);
/* out [nE][ncomp] = sum_k sum_b w_b(k; E_i) A_{c,b}(k): the resident weights against the attached elements
 * (abz_rule_ltm_elements, _orbitals, _projectors), i.e. abz_rule_ltm_weighted(r, ABZ_LTM_A_ELEMENTS, E, nE, what, out) of the
 * call that made the weights, without another walk over the simplices.  Fixed-order reduction: two calls return the same bits.
 * ABZ_ERR_ARG: no resident weights, nothing attached, out == NULL; ABZ_ERR_UNSUPPORTED as above. */
int abz_rule_ltm_node_weights_dot(abz_rule* r, double* out /* [nE][ncomp] */);
/* For a rule of abz_rule_ltm_unfold: the resident weights summed over each orbit onto the nirr nodes of the source rule, in the
 * source's node order; with them sum_j sum_b fold_b(j) A_b(j) is the full-grid N_A for every A that is invariant under the zone's
 * symmetries, from values at the irreducible nodes alone.  The Kuhn mesh is invariant under 12 of the 48 cubic operations only,
 * so w(S k) != w(k) in general: the fold is the plain sum over the orbit, not multiplicity x w.  The inverse of the rule's orbit
 * map is made at the first call and kept (8 B per node, 4 B per grid point, counted by abz_mem_info).  No floating-point atomics:
 * two calls return the same bits.  ABZ_ERR_ARG: a rule that was not unfolded, no resident weights, out == NULL. */
int abz_rule_ltm_node_weights_fold(abz_rule* r, double* out /* [nE][nirr][n] */);
/* The integration weights of the OPTIMIZED tetrahedron rule (abz_rule_ltm_optimized; Kawamura, Gohda, Tsuneyuki, who publish the
 * method in this form), d = 3: the numbers w_b(k; E) with
 *      sum_k sum_b w_b(k; E) A_b(k) = the N_A(E) (ABZ_LTM_STATES) or g_A(E) (ABZ_LTM_DOS) of abz_rule_ltm_optimized
 * for ANY A; sum w = N(E) or g(E), sum w e = the ABZ_LTM_A_ENERGY sums.  Every Kuhn simplex forms the corner weights of the
 * linear rule on its effective corner energies e' = P e and scatters them with P transposed onto its 20 stencil points:
 *      w_b(k; E) = 1 / (6 npt^3) sum_t sum_j sum_m P[m][j] w'_m(simplex t of the cell k - off_{t,j}; E),
 * every index wrapped mod npt (any npt >= 1).  Half-open regions e'_1 <= E < e'_4; a simplex with max e' <= E gives 1/4 to each
 * corner under ABZ_LTM_STATES, a flat one nothing under ABZ_LTM_DOS.  The columns of P have negative sums away from the corners:
 * these weights are NOT confined to [0, 1 / nk], and a node next to the Fermi surface can weigh negative (nk w down to -0.12 has
 * been seen).  Where every e' lies above E the weights are 0.0 exactly; where every e' lies below E they are 1 / nk to rounding.
 * Arguments, order of `out` and limits are those of abz_rule_ltm_node_weights, and the weights fill the SAME resident block:
 * abz_rule_ltm_node_weights_ptr, _dot, _fold and abz_rule_ltm_density_matrix then work on the optimized weights as they are.
 * No atomics: two calls write the same bits, and so does every value of the switch ABZ_LTM_OPTW_CHUNK_MB, which bounds the
 * scratch the corner weights of a slab of grid planes take (not part of the rule, not resident).
 * Takes full-grid rules and rules of abz_rule_ltm_unfold.  ABZ_ERR_ARG: a rule without eigenvalues, E == NULL, nE outside
 * 1..ABZ_LTM_NODEW_MAX_E, a non-finite energy, a `what` that is neither ABZ_LTM_DOS nor ABZ_LTM_STATES
 * (ABZ_LTM_STATES_CORRECTED is refused: this rule replaces the correction).  ABZ_ERR_UNSUPPORTED: d != 3, slabs with or without
 * a halo, lists of irreducible nodes, a stride between grid lines beyond 2^31 doubles.  A refusal or failure leaves the resident
 * weights as they were; a refusal, or a failure of the kernels (the copy to `out` starts after they have finished), `out` too.  Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_node_weights_optimized(abz_rule* r, const double* E, int nE, int what, double* out /* [nE][nk][n] or NULL */);
/* The density matrix in the orbital basis from the resident weights and the eigenvectors U(k) of Hermitian(H(k)), bands ascending:
 *      rho_pq(E_i) = sum_k sum_b w_b(k; E_i) U_pb(k) conj(U_qb(k)),      out [nE][n][n][2], per unit cell,
 * for the nE energies of the last abz_rule_ltm_node_weights call, whose `what` says what rho is: the occupation matrix
 * (ABZ_LTM_STATES; ABZ_LTM_STATES_CORRECTED: with the curvature correction) or the spectral-density matrix (ABZ_LTM_DOS).  The
 * call takes no energies of its own, like abz_rule_ltm_node_weights_dot.  tr rho = N(E) (g(E)); rho = 0.0 exactly below the
 * bands and I above them (ABZ_LTM_STATES).  One eigen-solve per node (and per group of up to 4 energies for 1...4 bands, per
 * energy for 5...32): neither U nor the band projectors reach HBM, where abz_rule_ltm_projectors in groups of
 * ABZ_LTM_MAX_COMP components + abz_rule_ltm_node_weights_dot repeats the solve of the whole grid for every group.  The upper
 * triangle is summed in a fixed order without atomics (two calls return the same bits) and the lower one is filled as its exact
 * conjugate: out is Hermitian to the bit.  No phase of an eigenvector changes rho; at a degenerate level U holds some
 * orthonormal basis of the eigenspace, and rho is defined as far as the weights of the level's bands agree (the tetrahedron
 * weights of exactly degenerate bands do).
 * H(k) is read from the rule when it holds it (either layout), else from a transient rule of the series' CURRENT coefficients
 * that lives for the call, as for abz_rule_ltm_orbitals.  Attached elements and the resident weights are left as they were, on
 * success and on failure; one synchronisation; the results leave through the pinned mailbox.
 * ABZ_ERR_ARG: out == NULL, no resident weights, a rule without eigenvalues, a series that is not Hermitian.
 * ABZ_ERR_UNSUPPORTED: more than 32 bands, a rule of abz_rule_ltm_unfold (no H(k) at every grid point), slabs with or without a
 * halo, lists of irreducible nodes, symmetric rules.  Entry point added without a change of ABZ_VERSION. */
int abz_rule_ltm_density_matrix(abz_rule* r, double* out /* [nE][n][n][2] */);

/* The complex integration weights of the Green's function, per grid point and band: the numbers W_b(k; z) with
 *      G_A(z) = sum_k sum_b W_b(k; z) A_b(k)
 * for ANY A -- complex, matrix-valued, or not known when the weights are made -- on the mesh of abz_rule_ltm_green: what
 * abz_rule_ltm_green_weighted forms inside its scan and contracts at once with real attached elements.
 *      W_b(k; z) = w sum_{T contains k} W^T_{i(k)}(z),   w = 1 / (d! npt^d),   W^T_i = J[x_0 .. x_d, x_i](z) / (d + 1),
 * over the (d+1)! Kuhn simplices that contain k (the geometry of abz_rule_ltm_node_weights), with the evaluation rule of
 * abz_rule_ltm_green_weighted (rho = 1/2, Taylor series for narrow sub-ranges, principal logs of one half plane).
 * z [nz][2] (re, im), 1 <= nz <= ABZ_LTM_GREEN_NODEW_MAX_Z, Im z != 0, in any order, duplicates allowed.  out [nz][nk][n][2]
 * (or NULL: nothing is copied) is interleaved complex in the node and band order of abz_rule_export's eig.  Im z < 0: the
 * conjugate of the value at conj(z), to the bit.  A gather without atomics: two calls write the same bits.
 * The weights stay resident in HBM in a block of their own, 2 nz n planes tiled like the eigenvalue planes: plane
 * (2 i + part) n + b of a grid line's tile is Re (part 0) or Im (part 1) of band b at z_i, padding columns zero -- 2 nz real
 * weight sets to every consumer of a real weight block.  The block is separate from the one of abz_rule_ltm_node_weights:
 * neither call touches the other's.  It lives as that one does: until the next call replaces it, abz_rule_rebuild, a new gather
 * of abz_rule_ltm_unfold or abz_rule_destroy; attaching or dropping elements leaves it alone.  Counted by abz_mem_info.
 * Takes full-grid rules and rules of abz_rule_ltm_unfold, d = 1...3, 1...64 bands.  ABZ_ERR_UNSUPPORTED: slabs, with or without
 * a halo, lists of irreducible nodes, symmetric rules.  ABZ_ERR_ARG: a rule without eigenvalues, z == NULL, nz outside
 * 1..ABZ_LTM_GREEN_NODEW_MAX_Z, any Im z == 0 or non-finite z.  A refusal or failure leaves both weight blocks and the attached
 * elements as they were.  Entry points added without a change of ABZ_VERSION. */
#define ABZ_LTM_GREEN_NODEW_MAX_Z 8   /* 2 nz real weight sets <= ABZ_LTM_NODEW_MAX_E */
int abz_rule_ltm_green_node_weights(abz_rule* r, const double* z /* [nz][2] */, int nz, double* out /* [nz][nk][n][2] or NULL */);
/* The complex integration weights of the OPTIMIZED tetrahedron rule (abz_rule_ltm_green_optimized), d = 3: the numbers W_b(k; z)
 * with
 *      sum_k sum_b W_b(k; z) A_b(k) = the G_A(z) of abz_rule_ltm_green_optimized
 * for ANY A; sum W = its tr G(z), sum W e = z tr G(z) - n.  Every Kuhn simplex forms the complex corner weights
 * W'_m = J[sort(e'), e'_m](z) / 4 of the linear rule on its effective corner energies e' = P e (the evaluation rule of
 * abz_rule_ltm_green_weighted) and scatters them with P transposed onto its 20 stencil points:
 *      W_b(k; z) = 1 / (6 npt^3) sum_t sum_j sum_m P[m][j] W'_m(simplex t of the cell k - off_{t,j}; z),
 * every index wrapped mod npt (any npt >= 1).  They differ from the weights of abz_rule_ltm_green_node_weights by O(1 / npt^2).
 * Arguments, order of `out` and limits are those of abz_rule_ltm_green_node_weights, and the weights fill the SAME resident
 * block: abz_rule_ltm_green_node_weights_ptr, _dot, _fold and _matrix then work on the optimized weights as they are; the real
 * weights of abz_rule_ltm_node_weights and the attached elements are not touched.  Im z < 0: the conjugate of the value at
 * conj(z), to the bit.  No atomics: two calls write the same bits, and so does every value of the switch
 * ABZ_LTM_OPTW_CHUNK_MB, which bounds the scratch the corner weights of a slab of grid planes take.
 * Takes full-grid rules and rules of abz_rule_ltm_unfold.  ABZ_ERR_ARG: a rule without eigenvalues, z == NULL, nz outside
 * 1..ABZ_LTM_GREEN_NODEW_MAX_Z, any Im z == 0 or non-finite z.  ABZ_ERR_UNSUPPORTED: d != 3, slabs with or without a halo, lists
 * of irreducible nodes, a stride between grid lines beyond 2^31 doubles.  A refusal or failure leaves both weight blocks, the
 * attached elements and `out` as they were (the copy to `out` starts after the kernels have finished).  Entry point added
 * without a change of ABZ_VERSION. */
int abz_rule_ltm_green_node_weights_optimized(abz_rule* r, const double* z /* [nz][2] */, int nz, double* out /* [nz][nk][n][2] or NULL */);
/* The resident complex weights: device address, bytes and values of z of the block; NULL, 0, 0 when the rule holds none (any of
 * the three pointers may be NULL). */
int abz_rule_ltm_green_node_weights_ptr(const abz_rule* r, void** base, int64_t* nbytes, int* nz);
/* out [nz][ncomp][2] = sum_k sum_b W_b(k; z_i) A_{c,b}(k): the resident complex weights against the attached elements, i.e.
 * abz_rule_ltm_green_weighted(r, ABZ_LTM_A_ELEMENTS, z, nz, out) without another walk over the simplices (the dot of
 * abz_rule_ltm_node_weights_dot over the 2 nz real sets).  ABZ_ERR_ARG: no resident complex weights, nothing attached, out == NULL. */
int abz_rule_ltm_green_node_weights_dot(abz_rule* r, double* out /* [nz][ncomp][2] */);
/* For a rule of abz_rule_ltm_unfold: the resident complex weights summed over each orbit onto the nirr nodes of the source rule
 * (the fold of abz_rule_ltm_node_weights_fold over the 2 nz real sets): sum_j sum_b fold_b(j) A_b(j) is the full-grid G_A(z) of
 * every A that the zone's symmetries leave alone.  ABZ_ERR_ARG: a rule that was not unfolded, no resident complex weights,
 * out == NULL. */
int abz_rule_ltm_green_node_weights_fold(abz_rule* r, double* out /* [nz][nirr][n][2] */);
/* The local Green's function in the orbital basis from the resident complex weights and the eigenvectors U(k):
 *      G_pq(z_i) = sum_k sum_b W_b(k; z_i) U_pb(k) conj(U_qb(k)),      out [nz][n][n][2], per unit cell,
 * by the contraction of abz_rule_ltm_density_matrix over the 2 nz real sets: with X = rho[Re W], Y = rho[Im W], both Hermitian,
 * G_pq = X_pq + i Y_pq and G_qp = conj(X_pq) + i conj(Y_pq).  G is not Hermitian; G(z)^dagger = G(conj z).  Nothing is attached.
 * H(k), refusals and codes as abz_rule_ltm_density_matrix (1...32 bands, not a rule of abz_rule_ltm_unfold, a Hermitian series);
 * ABZ_ERR_ARG: no resident complex weights, out == NULL. */
int abz_rule_ltm_green_node_weights_matrix(abz_rule* r, double* out /* [nz][n][n][2] */);

/* Replaces: AutoSymPTR.symptr_rule as called at src/fourier.jl:271 (host, integer-exact).
 * syms [nsyms][d][d] row-major integer matrices acting on fractional coordinates.
 * First call with irr_idx = NULL to get *nirr; then with buffers irr_idx [nirr][d], wsym [nirr]. */
int abz_symptr_rule(int npt, int d, const int32_t* syms, int nsyms, int64_t* nirr,
                    int32_t* irr_idx, int64_t* wsym);
/* `syms` must be a group (closed, with the identity) as AutoSymPTR assumes: orbits are then equivalence
 * classes and "first member in column-major order" is well defined.
 * Same tables computed on the GPU (orbit kernel + order-preserving compaction): bit-identical output,
 * ~50x faster on large grids (the reference calls this step its likely bottleneck, src/fourier.jl:270). */
int abz_symptr_rule_device(abz_ctx* ctx, int npt, int d, const int32_t* syms, int nsyms,
                           int64_t* nirr, int32_t* irr_idx, int64_t* wsym);

/* ---------------------------------------------------------------- IAI building blocks + driver
 * Replaces: workspace_contract!(w, x) on a batch of nodes (src/fourier.jl:468,478):
 * contracts the outermost remaining variable of `src_level` coefficient sets (src_level = 2..d).  The
 * library keeps contracted sets in its own device pool; `slots_out[i]` identifies the set made from parent
 * slot `parents[i]` (slot 0 at level d = the series itself) at coordinate x[i].
 * Slots are numbered consecutively per level from the level's current count: a call with nnodes nodes while
 * the level below src_level holds c sets returns c .. c + nnodes - 1 and keeps the sets made before it.
 * Slots are invalidated by abz_release_level, abz_iai_solve*, and abz_series_update (the counts go back to 0).
 * nnodes < 0 is ABZ_ERR_ARG; nnodes == 0 is ABZ_OK with nothing launched and the counts unchanged.
 * Every parents[i] must be 0 when src_level == d, otherwise a live slot of level src_level, 0 <= parents[i] <
 * its count: anything else is ABZ_ERR_ARG before any device work (the message names the first bad index, its
 * value and the number of live slots), with slots_out and the counts untouched. */
int abz_contract_nodes(abz_series* s, int src_level, const int64_t* parents, const double* x,
                       int64_t nnodes, int64_t* slots_out);
/* Replaces: workspace_evaluate!(w, x) + integrand at a batch of innermost nodes
 * (src/fourier.jl:445-446,454-455): values_reim [nnodes][ncomp][2].  tail [nnodes][d-1] gives the
 * outer coordinates (x_2..x_d) of each node's line (needed by ABZ_F_LINEAR_X only; may be NULL).
 * nnodes < 0 is ABZ_ERR_ARG; nnodes == 0 is ABZ_OK with nothing launched.
 * Every parents[i] must be 0 for d = 1, otherwise a live level-1 slot, 0 <= parents[i] < the level's count:
 * anything else is ABZ_ERR_ARG before any device work.  Every refused call (these, or an integrand that is not
 * built for the series' band count) leaves values_reim untouched. */
int abz_eval_line_nodes(abz_series* s, const int64_t* parents, const double* x, const double* tail,
                        int64_t nnodes, int integrand, const double* params, int nparams,
                        double sweep, double* values_reim);
/* Drop all contracted sets below `level` (1..d): their slots are invalid from here on and the next
 * abz_contract_nodes into those levels numbers from 0 again. */
int abz_release_level(abz_series* s, int level);

/* Whole IAI solve with the adaptive GK(7,15) loops on the host and every node batch on the GPU.
 * Replaces: do_solve(::FourierIntegrand, lims, p, ::NestedQuad, cacheval) (src/fourier.jl:493-510)
 * with init_nest (:432-486) and AuxQuadGKJL (src/algorithms.jl:215-239).  Sibling 1-D integrals
 * advance in lockstep so each round is one batch; every 1-D integral makes exactly the scalar
 * refinement decisions of the reference (pop worst panel, bisect), so panel trees are identical.
 * lim_a/lim_b: CubicLimits a, b (len d) or TetrahedralLimits a (lim_b ignored).
 * abstol < 0 / reltol < 0 mean `nothing`.  max_batch = 0: scalar refinement (the reference's default
 * IAI()); max_batch > 0: the BatchIntegrand / NestedBatchIntegrand refinement at every level (pop
 * panels while the error of the remaining ones exceeds the tolerance, 2*15*popped <= max_batch;
 * ref src/batch.jl:41-77, src/fourier.jl:441-473).  out_reim [ncomp][2]; err = the outermost GK
 * error estimate; panels (nullable, [max_panels][2]) receives the outermost integral's final panels. */
int abz_iai_solve(abz_series* s, int lims_kind, const double* lim_a, const double* lim_b,
                  int integrand, const double* params, int nparams, double sweep, double abstol,
                  double reltol, int64_t maxevals, int64_t max_batch, double* out_reim, double* err,
                  int64_t* numevals, double* panels, int64_t max_panels, int64_t* npanels);

/* The same for n_sweep values of the swept parameter at once (batchsolve over omega with IAI,
 * src/interfaces.jl:210-222): the solves are independent adaptive integrals that advance in lock-step,
 * so every contraction / evaluation launch carries the nodes of all of them.  Each solve makes exactly
 * the decisions it would make alone.  out_reim [n_sweep][ncomp][2], err [n_sweep], numevals [n_sweep];
 * panels: outermost panels of the first solve. */
int abz_iai_solve_many(abz_series* s, int lims_kind, const double* lim_a, const double* lim_b,
                       int integrand, const double* params, int nparams, const double* sweeps,
                       int n_sweep, double abstol, double reltol, int64_t maxevals, int64_t max_batch,
                       double* out_reim, double* err, int64_t* numevals, double* panels,
                       int64_t max_panels, int64_t* npanels);

/* ONE IAI solve on several GPUs (disjoint sets of the inner integrals of every refinement round).  All
 * ranks call abz_iai_solve(_many) with the same arguments; every round's innermost integrals are dealt to the ranks in
 * blocks of 64 nodes, each rank integrates its share on its own GPU, and `fn(user, buf, per_rank)` all-gathers the results:
 * `buf` holds world * per_rank doubles, segment `rank` is filled on entry, all segments must be filled on return (RCCL
 * / MPI / gloo: the library does not link a communication layer).  Every rank returns the same value, bit-identical to the
 * single-GPU solve.  fn = NULL switches it off (world = 1 with a hook is allowed: a one-rank rehearsal of the transport).
 * Errors: a rank whose share fails locally (HIP error, out of memory) still joins the collective -- every segment ends in a
 * status word -- and ALL ranks return that rank's ABZ_ERR_* code after the exchange; nobody is left waiting.  `fn` itself
 * must fail on every rank or on none (it is the caller's collective; return non-zero on all ranks to abort the solve).
 * Replaces: nothing in the reference (its parallelism is threads over parameters, src/interfaces.jl:210-222). */
typedef int (*abz_exchange_fn)(void* user, double* buf, int64_t per_rank);
int abz_iai_set_exchange(abz_series* s, abz_exchange_fn fn, void* user, int rank, int world);

/* Replaces: QuadGK.evalrule on a batch of panels (reached from src/algorithms.jl:227-233):
 * values [npanels][15][ncomp][2] in gk node order -> I_reim [npanels][ncomp][2], E [npanels]
 * with I = I_K * h, E = ||I_K - I_G|| * h (2-norm over components). */
int abz_gk15_nodes(double a, double b, double* x15);
int abz_gk15_batch(const double* ab, const double* values_reim, int64_t npanels, int ncomp,
                   double* I_reim, double* E);

#ifdef __cplusplus
}
#endif
#endif /* ABZHIP_H */
