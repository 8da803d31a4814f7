// Optimized tetrahedron method (gfx950 only): the integration weights w_b(k; E) per grid point and band of the rule of
// kernels_ltm_opt.hip, d = 3, written into a weight block laid out like that of kernels_ltm_nodew.hip.
//
// Kawamura, Gohda, Tsuneyuki, PRB 89, 094515 (2014) publish their method as such a set of weights.  The reference has no
// counterpart (src/dos_algorithms.jl:1-7 plans "LTM").
//
//  * Definition.  For every Kuhn simplex T (path t, cell i) and band b the effective corner energies are e'_m = sum_j P[m][j] e_b(p_j)
//    (ltm_opt_device.h; kernels_ltm_opt.hip has the derivation).  w'_m(T; E), m = 1..4, are the corner weights of the LINEAR rule on
//    (e'_1..e'_4), in path order, unit = one simplex: the closed forms in the head of kernels_ltm_nodew.hip, half-open regions
//    e'_1 <= E < e'_4 after sorting; a simplex with max e' <= E gives 1/4 to each corner under ABZ_LTM_STATES and nothing under
//    ABZ_LTM_DOS, a flat one nothing under ABZ_LTM_DOS.  An element takes the same projection, A'_m = sum_j P[m][j] A(p_j), so the
//    simplex's sum_m w'_m A'_m is sum_j (sum_m P[m][j] w'_m) A(p_j): the corner weights are scattered with P transposed onto the 20
//    points, and
//        w_b(k; E) = 1 / (6 npt^3) sum_t sum_{j = 1..20} sum_{m = 1..4} P[m][j] w'_m(T = (t, cell k - off_{t,j}); E),
//    off_{t,j} the offset of stencil point j of path t from the cell's corner 0, inside [-1, 2]^3, every index wrapped mod npt
//    (below npt = 4 a node receives from the same simplex more than once).  sum_k sum_b w A is then the N_A / g_A of
//    abz_rule_ltm_optimized for ANY A.  The columns of P have negative sums away from the corners: these weights are NOT confined
//    to [0, 1 / nk], and a node next to the Fermi surface can weigh negative (npt^3 w down to -0.12 has been seen).
//  * Two kernels per group of NE = 1 or 4 energies (by value, as in ltm_nodew_kernel), no atomics anywhere:
//    A. ltm_opt_cornerw_kernel<STATES, NE>: one cell per thread, its six simplices one after the other, blockIdx.y the band; the
//       stencil addressing is OptPath of ltm_opt_device.h (nothing indexed at run time, no scratch, a 32-bit line stride that the
//       host checks), the prologue optw_cell and the sort optw_sort of ltm_opt_nodew_device.h.  Per simplex 20 loads, the product,
//       the compare-exchange sort that carries each corner's path position along, the reciprocals once for the group.  It stores the four weights in PATH order for each energy into a workspace of 24 planes
//       [t 4 + m] per band and energy, cell-contiguous (a wave's store is a run); a simplex outside its window stores 0.0, or
//       0.25 when it lies wholly below E under STATES: the workspace needs no clearing.
//    B. ltm_opt_nodew_gather_kernel<NE> (ltm_opt_nodew_device.h, shared with kernels_ltm_green_opt_nodew.hip): one thread per (column of a padded grid line, band); it sums the 6 x 20 x (the non-zero of
//       4) terms P[m][j] C[t 4 + m][k - off_{t,j}] in ONE program order (t, then j, then m), multiplies by 1 / (6 npt^3) and
//       writes plane iE n + b of the weight block; padding columns +0.0.  Consecutive lanes are consecutive i_1: every load is a
//       shifted run of a line of the workspace.
//  * Workspace and slabs.  The workspace is scratch of the context, bounded by ABZ_LTM_OPTW_CHUNK_MB (default 256 MB).  Node planes
//    along axis 3 are taken in slabs of S planes; a slab needs the corner weights of the cells of the planes s - 2 .. s + S, wrapped:
//    S + 3 planes, the overlap is computed again.  S is as large as the cap allows and at least 1; where S + 3 planes hold the whole
//    grid there is one slab of npt planes whose plane indices wrap (this is every npt < 4, where wrapped planes coincide).  A
//    node's sum has the same terms in the same order whatever S is: the block has the same bits for every cap.  The planner
//    (optw_slab, optw_need) and the slab loop (optw_run_group) stand in ltm_opt_nodew_device.h; this file groups the energies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_opt_device.h"
#include "ltm_opt_nodew_device.h"

namespace abz {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// A: corner weights of every simplex of the workspace's cells
// ---------------------------------------------------------------------------------------------------------------------
template <bool STATES, int NE>
__global__ __launch_bounds__(256) void ltm_opt_cornerw_kernel(OptWArgs a) {
    const int64_t kk = (int64_t)blockIdx.x * 256 + threadIdx.x;  // cell of the workspace: column i1 of line i2 of its plane q
    if (kk >= a.wsplane) return;
    const OptWCell c = optw_cell(a, kk, NE);  // (a set is an energy)
    double En[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) En[i] = a.Es[i];
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        const OptPath path(t, c.j1, c.j2, c.j3);
        double x[OPT_NPT], e[4];
        path.load(c.Eb, c.tileE, x);
        opt_project(x, e);
        const OptWSorted s = optw_sort(e);
        const double e1 = s.e1, e2 = s.e2, e3 = s.e3, e4 = s.e4;
        bool inside = false;
#pragma unroll
        for (int i = 0; i < NE; ++i) inside = inside || (En[i] >= e1 && En[i] < e4);
        // an unselected region may have zero width: its reciprocal is then inf and never read
        double r21 = 0.0, r31 = 0.0, r41 = 0.0, r32 = 0.0, r42 = 0.0, r43 = 0.0;
        if (inside) {
            r21 = 1.0 / (e2 - e1);
            r31 = 1.0 / (e3 - e1);
            r41 = 1.0 / (e4 - e1);
            r32 = 1.0 / (e3 - e2);
            r42 = 1.0 / (e4 - e2);
            r43 = 1.0 / (e4 - e3);
        }
        double* __restrict__ const ot = c.out + (int64_t)(t * 4) * a.wsplane;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const double E = En[i];
            // outside the window: nothing, or the whole simplex (a flat one included)
            double w1 = STATES && !(E < e4) ? 0.25 : 0.0, w2 = w1, w3 = w1, w4 = w1;
            if (E >= e1 && E < e4) {
                if (E < e2) {
                    const double xx = E - e1, t2 = xx * r21, t3 = xx * r31, t4 = xx * r41;
                    const double q = STATES ? 0.25 * (t2 * t3 * t4) : t3 * t4 * r21;
                    w2 = q * t2;
                    w3 = q * t3;
                    w4 = q * t4;
                    w1 = (STATES ? 4.0 : 3.0) * q - (w2 + w3 + w4);
                } else if (E < e3) {
                    const double x1 = E - e1, x2 = E - e2;
                    const double t13 = x1 * r31, t14 = x1 * r41, t23 = x2 * r32, t24 = x2 * r42;
                    // shares of the vertices P13, P14, P23, P24 and of the corners 1, 2 themselves
                    double p13, p14, p23, p24, c1, c2;
                    if (STATES) {
                        const double v1 = 0.25 * (t13 * t14), v2 = 0.25 * (t14 * t23 * (1.0 - t13)), v3 = 0.25 * ((1.0 - t14) * t23 * t24);
                        p13 = v1 + v2;
                        p14 = v1 + v2 + v3;
                        p23 = v2 + v3;
                        p24 = v3;
                        c1 = v1;
                        c2 = p14;
                    } else {
                        const double ga = t13 * (1.0 - t23) * r41, gb = t23 * (1.0 - t24) * r41;
                        p13 = ga;
                        p14 = ga + gb;
                        p23 = p14;
                        p24 = gb;
                        c1 = 0.0;
                        c2 = 0.0;
                    }
                    w1 = c1 + p13 * (1.0 - t13) + p14 * (1.0 - t14);
                    w2 = c2 + p23 * (1.0 - t23) + p24 * (1.0 - t24);
                    w3 = p13 * t13 + p23 * t23;
                    w4 = p14 * t14 + p24 * t24;
                } else {
                    const double y = e4 - E, s1 = y * r41, s2 = y * r42, s3 = y * r43;
                    const double q = STATES ? 0.25 * (s1 * s2 * s3) : s1 * s2 * r43;
                    const double u1 = q * s1, u2 = q * s2, u3 = q * s3, u4 = (STATES ? 4.0 : 3.0) * q - (u1 + u2 + u3);
                    w1 = STATES ? 0.25 - u1 : u1;
                    w2 = STATES ? 0.25 - u2 : u2;
                    w3 = STATES ? 0.25 - u3 : u3;
                    w4 = STATES ? 0.25 - u4 : u4;
                }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) ot[(int64_t)(i * 24 + m) * a.wsplane] = optw_of_path(s, m, w1, w2, w3, w4);
        }
    }
}

// [states][NE == 4]
constexpr OptWFn OPTW_CORNER[2][2] = {
    {ltm_opt_cornerw_kernel<false, 1>, ltm_opt_cornerw_kernel<false, 4>},
    {ltm_opt_cornerw_kernel<true, 1>, ltm_opt_cornerw_kernel<true, 4>},
};
constexpr OptWFn OPTW_GATHER[2] = {ltm_opt_nodew_gather_kernel<1>, ltm_opt_nodew_gather_kernel<4>};

}  // namespace

// The block W (nE n planes, tiled like the eigenvalue planes E with pitch = row, padding columns included) <- the weights of the
// optimized rule at Es[i].  Launches only; groups of 4 energies, then single ones; per group the slabs one after the other.
int launch_ltm_node_weights_optimized(abz_ctx* ctx, int n, int npt, PlaneView E, PlaneView W, const double* Es_host, int nE, bool states) {
    if (E.tile > INT32_MAX || (int64_t)npt * npt > INT32_MAX) {
        set_error("abz_rule_ltm_node_weights_optimized: a stride of %lld doubles between grid lines does not fit the kernel's 32-bit factor",
                  (long long)E.tile);
        return ABZ_ERR_UNSUPPORTED;
    }
    OptWArgs a;
    a.E = E;
    a.W = W;
    a.npt = npt;
    a.n = n;
    a.weight = 1.0 / (6.0 * (double)npt * (double)npt * (double)npt);
    size_t need = 0;
    for (int ne : {1, 4})
        if (ne == 1 ? (nE % 4 != 0 || nE < 4) : nE >= 4) need = std::max(need, optw_need(npt, n, ne));
    int rc = ctx->scratch[1].reserve(need);
    if (rc) return rc;
    a.C = ctx->scratch[1].as<double>();
    ProfScope ps(ctx, ABZ_K_LTM);
    for (int i0 = 0; i0 < nE;) {
        const int ne = nE - i0 >= 4 ? 4 : 1;
        for (int i = 0; i < 4; ++i) a.Es[i] = Es_host[i0 + std::min(i, ne - 1)];
        a.plane0 = i0 * n;
        if ((rc = optw_run_group(ctx, a, ne, OPTW_CORNER[states][ne == 4], OPTW_GATHER[ne == 4]))) return rc;
        i0 += ne;
    }
    return ABZ_OK;
}

}  // namespace abz
