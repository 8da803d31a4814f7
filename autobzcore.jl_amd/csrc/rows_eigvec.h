// Eigenvectors in the row layout (NP = 8 / 16 / 32 lanes per node, lane r owning row r of a Hermitian matrix in registers):
// Householder tridiagonalisation with the reflectors kept, the eigenvector of the real tridiagonal by inverse iteration in the
// lane of its eigenvalue, and the back-transformation -- eigenvalue b (ascending) and column b of U end up in lane b
// (rows_eigh_columns).  Steps (2)-(5) of the fused GGR build (kernels_ggr_rows.hip, which describes them); shared with the
// orbital weights of the tetrahedron method (kernels_ltm_orb.hip).  Below them the Hermitian quadratic form u_b^H D u_b of a lane's
// column from a matrix parked in the node's LDS room (park_upper, quad_form): the GGR velocities and the band expectation
// values of kernels_ltm_expect.hip.  gfx950 only.
#pragma once
#include <utility>

#include "abz_internal.h"
#include "rows_device.h"

namespace abz {

namespace {

// a wave's LDS writes visible to its other lanes (the rooms are wave-private: no block barrier)
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Room of one node's kept reflectors / derivative rows in LDS (complex numbers; + 1: the nodes of a wave start on different banks)
template <int NP>
constexpr int REFL_STRIDE = NP * (NP - 1) / 2 + 1;  // v_K[i], i > K, at K NP - K (K + 1) / 2 + (i - K - 1)
template <int NP>
constexpr int DUP_STRIDE = NP * (NP + 1) / 2 + 1;   // D[R][c], R <= c, at c (c + 1) / 2 + R
template <int NP>
constexpr int PARK_STRIDE = DUP_STRIDE<NP>;

// what the Householder steps leave behind (rows_device.h: hh_step): the reflector components go to `park` (this node's room)
template <int NP>
struct HhKeep {
    double2* park;
    double beta = 0.0;        // lane K + 1: beta of step K
    double phr = 1.0, phi = 0.0;  // lane j: accumulated phase p_j of the subdiagonal (p_0 = 1, p_{K+1} = p_K e_K / |e_K|)
    double cr = 1.0, ci = 0.0;    // the running product (uniform inside the node)
    template <int NPX, int K>
    __device__ __forceinline__ void reflect(int r, double vr, double vi, double b, double x1r, double x1i, double a1sq, double sigma) {
        if (r > K && r < NPX) park[K * NPX - K * (K + 1) / 2 + (r - K - 1)] = make_double2(vr, vi);
        beta = (r == K + 1) ? b : beta;
        // e_K = -(x1 / |x1|) sqrt(sigma); x1 = 0: -sqrt(sigma); sigma = 0: no coupling, phase 1
        double ur = -1.0, ui = 0.0;
        if (a1sq > 0.0) {
            const double inv = a1sq >= 1e-280 ? rsqrt_nr(a1sq) : 1.0 / sqrt(a1sq);
            ur = -x1r * inv;
            ui = -x1i * inv;
        }
        if (!(sigma > 0.0)) {
            ur = 1.0;
            ui = 0.0;
        }
        const double nr = cr * ur - ci * ui, ni = cr * ui + ci * ur;
        cr = nr;
        ci = ni;
        phr = (r == K + 1) ? cr : phr;
        phi = (r == K + 1) ? ci : phi;
    }
    template <int NPX, int K>
    __device__ __forceinline__ void last(int r, double xr, double xi) {
        if constexpr (K + 1 < NPX) {
            const double x1r = group_bcast<NPX, K + 1>(xr), x1i = group_bcast<NPX, K + 1>(xi);
            const double a1sq = x1r * x1r + x1i * x1i;
            double ur = 1.0, ui = 0.0;
            if (a1sq > 0.0) {
                const double inv = a1sq >= 1e-280 ? rsqrt_nr(a1sq) : 1.0 / sqrt(a1sq);
                ur = x1r * inv;
                ui = x1i * inv;
            }
            const double nr = cr * ur - ci * ui, ni = cr * ui + ci * ur;
            cr = nr;
            ci = ni;
            phr = (r == K + 1) ? cr : phr;
            phi = (r == K + 1) ? ci : phi;
        }
    }
};

// ---- eigenvector of the real symmetric tridiagonal (d, |e|^2) for this lane's eigenvalue `lam`: everything in the lane's own
// registers, all indices compile-time.  Scaled to unit Gershgorin radius like the bisection.
template <int NP>
struct TriLU {
    double a[NP], b[NP], dd[NP], c[NP], ia[NP];  // U: diagonal, first and second superdiagonal; multipliers of L; 1 / pivots
    unsigned swapped = 0;                        // bit k: rows k, k + 1 were interchanged
};

// The loops below run over all NP rows without a condition on n: tri_eigvec pads the matrix with a decoupled block (zero
// coupling, diagonal far outside the spectrum) and the start vector with zeros, so rows >= n stay exactly zero.  (Guards
// `k < n` on these straight-line bodies were turned into selects by the compiler anyway: both sides computed, the uniform
// masks kept in dozens of SGPR pairs.)
template <int NP>
__device__ __forceinline__ void tri_factor(const double (&ds)[NP], const double (&off)[NP], double lam, TriLU<NP>& f) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        f.a[k] = ds[k] - lam;
        f.b[k] = off[k];
        f.c[k] = off[k];
        f.dd[k] = 0.0;
    }
    f.swapped = 0;
    double scale1 = fabs(f.a[0]) + fabs(f.b[0]);
#pragma unroll
    for (int k = 0; k + 1 < NP; ++k) {
        const double bk1 = (k + 2 < NP) ? f.b[k + 1] : 0.0;
        const double ak = f.a[k], ak1 = f.a[k + 1], ck = f.c[k], bk = f.b[k];
        const double scale2 = fabs(ck) + fabs(ak1) + fabs(bk1);
        // dlagtf: interchange when |c| / scale2 > |a| / scale1 (real rows: c is never zero, the couplings are floored; the
        // padding: c = 0, no interchange, multiplier 0)
        const bool sw = fabs(ck) * scale1 > fabs(ak) * scale2;
        const double piv = sw ? ck : ak;
        const double ip = rcp_nr(fabs(piv) < 1e-290 ? 1e-290 : piv);
        const double mult = (sw ? ak : ck) * ip;
        // no interchange: a[k+1] -= mult b[k].   interchange: a[k] = c, a[k+1] = b[k] - mult a[k+1], d[k] = b[k+1],
        // b[k+1] = -mult b[k+1], b[k] = old a[k+1]
        f.a[k] = piv;
        f.a[k + 1] = sw ? fma(-mult, ak1, bk) : fma(-mult, bk, ak1);
        f.b[k] = sw ? ak1 : bk;
        f.dd[k] = sw ? bk1 : 0.0;
        if (k + 2 < NP) f.b[k + 1] = sw ? -mult * bk1 : f.b[k + 1];
        f.c[k] = mult;
        f.swapped |= sw ? (1u << k) : 0u;
        scale1 = sw ? scale1 : scale2;
    }
    // reciprocal pivots; a pivot below eps (unit scale) is replaced by +-eps as dlagts does with job = -1
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const double ak = f.a[k];
        const double pk = fabs(ak) < 2.3e-16 ? (ak < 0.0 ? -2.3e-16 : 2.3e-16) : ak;
        f.ia[k] = rcp_nr(pk);
    }
}

// y <- inv(T - lam I) y, then y scaled to unit maximum norm
template <int NP>
__device__ __forceinline__ void tri_solve(const TriLU<NP>& f, double (&y)[NP]) {
#pragma unroll
    for (int k = 0; k + 1 < NP; ++k) {
        const bool sw = (f.swapped >> k) & 1u;
        const double yk = y[k], yk1 = y[k + 1];
        y[k] = sw ? yk1 : yk;
        y[k + 1] = sw ? fma(-f.c[k], yk1, yk) : fma(-f.c[k], yk, yk1);
    }
#pragma unroll
    for (int k = NP - 1; k >= 0; --k) {
        double t = y[k];
        if (k + 1 < NP) t = fma(-f.b[k], y[k + 1 < NP ? k + 1 : k], t);
        if (k + 2 < NP) t = fma(-f.dd[k], y[k + 2 < NP ? k + 2 : k], t);
        y[k] = t * f.ia[k];
    }
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) mx = fmax(mx, fabs(y[k]));
    const double s = (mx > 1e-290 && mx < 1e290) ? rcp_nr(mx) : 1.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) y[k] *= s;
}

template <int NP>
__device__ __forceinline__ void unit2(double (&y)[NP]) {
    double nn = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) nn = fma(y[k], y[k], nn);
    const double s = nn > 1e-290 ? rsqrt_nr(nn) : 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) y[k] *= s;
}

template <int NP>
__device__ __forceinline__ void tri_eigvec(int n, int r, int lane, const double (&d)[NP], const double (&e2)[NP], double lam, double (&z)[NP]) {
    double lo = d[0], hi = d[0], eprev = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (i < n) {
            const double en = (i + 1 < n) ? sqrt(e2[i]) : 0.0;
            lo = fmin(lo, d[i] - eprev - en);
            hi = fmax(hi, d[i] + eprev + en);
            eprev = en;
        }
    }
    const double span = fmax(fabs(lo), fabs(hi));
    const double sc = span > 0.0 ? 1.0 / span : 1.0;
    double ds[NP], off[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const double y = fmax(e2[i] * sc * sc, 4.9e-32);  // the floor of the bisection: the matrix it found the eigenvalues of
        // rows >= n: a decoupled block with its diagonal at 4 (the spectrum lies in [-1, 1])
        ds[i] = (i < n) ? d[i] * sc : 4.0;
        off[i] = (i + 1 < n) ? y * rsqrt_nr(y) : 0.0;
    }
    const double lams = lam * sc;
    // clusters: lane r is linked to lane r - 1 when their eigenvalues are within 1e-5 of the scale; pos = links below it
    const double lprev = __shfl(lams, lane > 0 ? lane - 1 : 0, 64);
    const bool link = r > 0 && r < n && (lams - lprev) <= 1e-5;
    const unsigned long long links = __builtin_amdgcn_ballot_w64(link);
    const unsigned long long below = (~links) & ((2ull << lane) - 1ull);  // (bit of the node's first lane is always set)
    const int pos = lane - (63 - __builtin_clzll(below));
    TriLU<NP> f;
    tri_factor<NP>(ds, off, lams + 2.3e-15 * (double)pos, f);
    // start vector: lane dependent, no zeros, no symmetry
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const unsigned h = (unsigned)(r * 40503 + i * 30011 + 12345) * 2654435761u;
        z[i] = (i < n) ? (double)((h >> 8) & 0xffffu) * (1.0 / 65536.0) + 0.25 : 0.0;
        z[i] = ((h >> 30) & 1u) ? -z[i] : z[i];
    }
    tri_solve<NP>(f, z);
    tri_solve<NP>(f, z);
    tri_solve<NP>(f, z);
    unit2<NP>(z);
    // cluster members, lowest first: Gram-Schmidt against the members below (final by then), two more solves each
    for (int p = 1; __builtin_amdgcn_ballot_w64(pos >= p) != 0ull; ++p) {  // wave-uniform; not entered without a cluster
        for (int it = 0; it < 3; ++it) {
            double y[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) y[i] = z[i];
            if (it > 0) tri_solve<NP>(f, y);
            for (int t = 1; t <= p; ++t) {  // (the member's vector is fetched twice rather than held: registers)
                double dot = 0.0;
                const int src = lane - t >= 0 ? lane - t : 0;
#pragma unroll
                for (int i = 0; i < NP; ++i) dot = fma(__shfl(z[i], src, 64), y[i], dot);
                dot = (t <= pos) ? dot : 0.0;
#pragma unroll
                for (int i = 0; i < NP; ++i) y[i] = fma(-dot, __shfl(z[i], src, 64), y[i]);
            }
            unit2<NP>(y);
            if (pos == p) {
#pragma unroll
                for (int i = 0; i < NP; ++i) z[i] = y[i];
            }
        }
    }
}

// y = P z (complex), then u = H_0 ... H_{n-3} y.  Lane b works on its own column; v_K comes back from the node's room in LDS
// (the same address for all lanes of a node: broadcast reads).
template <int NP, int K, int... I>
__device__ __forceinline__ void back_step(int n, const HhKeep<NP>& kp, double (&ur)[NP], double (&ui)[NP], std::integer_sequence<int, I...>) {
    if (K + 2 >= n) return;  // uniform: no reflector for this step
    const double beta = group_bcast<NP, K + 1>(kp.beta);
    const double2* __restrict__ vk = kp.park + (K * NP - K * (K + 1) / 2);
    double2 v[NP - K - 1];
    // w = v^H u = sum_i conj(v_i) u_i: two accumulator pairs (even / odd i) halve the dependent chains
    double wr[2] = {0.0, 0.0}, wi[2] = {0.0, 0.0};
    ((void)([&] {
         constexpr int i = K + 1 + I;  // (rows >= n: v = 0 was stored, u = 0)
         v[I] = vk[I];
         wr[I & 1] = fma(v[I].x, ur[i], wr[I & 1]);
         wr[I & 1] = fma(v[I].y, ui[i], wr[I & 1]);
         wi[I & 1] = fma(v[I].x, ui[i], wi[I & 1]);
         wi[I & 1] = fma(-v[I].y, ur[i], wi[I & 1]);
     }()),
     ...);
    const double wwr = (wr[0] + wr[1]) * beta, wwi = (wi[0] + wi[1]) * beta;
    ((void)([&] {
         constexpr int i = K + 1 + I;  // u_i -= w v_i
         ur[i] = fma(-wwr, v[I].x, ur[i]);
         ur[i] = fma(wwi, v[I].y, ur[i]);
         ui[i] = fma(-wwr, v[I].y, ui[i]);
         ui[i] = fma(-wwi, v[I].x, ui[i]);
     }()),
     ...);
}
template <int NP, int... KK>
__device__ __forceinline__ void back_steps(int n, const HhKeep<NP>& kp, double (&ur)[NP], double (&ui)[NP], std::integer_sequence<int, KK...>) {
    // K = NP - 3 - KK: the last reflector first
    (back_step<NP, NP - 3 - KK>(n, kp, ur, ui, std::make_integer_sequence<int, NP - (NP - 3 - KK) - 1>()), ...);
}
template <int NP, int... J>
__device__ __forceinline__ void phase_apply(int n, const HhKeep<NP>& kp, const double (&z)[NP], double (&ur)[NP], double (&ui)[NP],
                                            std::integer_sequence<int, J...>) {
    ((void)([&] {
         const double pr = group_bcast<NP, J>(kp.phr), pi = group_bcast<NP, J>(kp.phi);
         ur[J] = (J < n) ? pr * z[J] : 0.0;
         ui[J] = (J < n) ? pi * z[J] : 0.0;
     }()),
     ...);
}

// eigenvalue b (ascending) and column b of U in lane b, from the rows (ar, ai) of the Hermitian matrix (destroyed); `park`:
// this node's room in LDS
template <int NP>
__device__ __forceinline__ void rows_eigh_columns(int n, int r, int lane, double2* park, double (&ar)[NP], double (&ai)[NP], double& myeig,
                                                  double (&ur)[NP], double (&ui)[NP]) {
    HhKeep<NP> kp;
    kp.park = park;
    double z[NP];
    {
        double e2[NP], d[NP];
        hh_steps_keep<NP>(n, r, ar, ai, e2, kp, std::make_integer_sequence<int, NP>());
        diag_gather<NP>(ar, d, std::make_integer_sequence<int, NP>());
        myeig = tri_eigval_bisect<NP>(n, r, d, e2);
        tri_eigvec<NP>(n, r, lane, d, e2, myeig, z);
    }
    phase_apply<NP>(n, kp, z, ur, ui, std::make_integer_sequence<int, NP>());
    wave_sync_lds();  // the reflectors were written by other lanes of this wave
    if constexpr (NP >= 3) back_steps<NP>(n, kp, ur, ui, std::make_integer_sequence<int, NP - 2>());
}

// u^H D u for this lane's column u, D Hermitian: lane r parks the upper triangle of its row (D[r][c], c >= r) in the node's
// room, every lane reads D[R][c] back (broadcast reads), column c at a time
template <int NP>
__device__ __forceinline__ void park_upper(int n, int r, double2* park, const double (&dr)[NP], const double (&di)[NP]) {
#pragma unroll
    for (int c = 0; c < NP; ++c)
        if (c < n && r <= c) park[c * (c + 1) / 2 + r] = make_double2(dr[c], di[c]);
}
template <int NP, int C, int... RR>
__device__ __forceinline__ void quad_col(int n, const double2* __restrict__ park, const double (&ur)[NP], const double (&ui)[NP], double& diag,
                                         double (&offd)[2], std::integer_sequence<int, RR...>) {
    if (C >= n) return;  // uniform
    const double2* __restrict__ col = park + C * (C + 1) / 2;
    // u_C through an opaque move: the products conj(u_R) u_C do not depend on the direction, and the compiler hoisted all
    // n (n - 1) of them out of the loop over the directions -- through scratch memory (186 stores, 1.5 KB per lane)
    double ucr = ur[C], uci = ui[C];
    asm volatile("" : "+v"(ucr), "+v"(uci));
    diag = fma(col[C].x, fma(ucr, ucr, uci * uci), diag);
    ((void)([&] {
         constexpr int R = RR;  // R < C
         const double2 dv = col[R];
         const double tr = fma(ur[R], ucr, ui[R] * uci);   // conj(u_R) u_C
         const double ti = fma(ur[R], uci, -ui[R] * ucr);
         offd[R & 1] = fma(dv.x, tr, offd[R & 1]);
         offd[R & 1] = fma(-dv.y, ti, offd[R & 1]);
     }()),
     ...);
}
template <int NP, int... CC>
__device__ __forceinline__ double quad_form(int n, const double2* __restrict__ park, const double (&ur)[NP], const double (&ui)[NP],
                                            std::integer_sequence<int, CC...>) {
    double diag = 0.0, offd[2] = {0.0, 0.0};
    (quad_col<NP, CC>(n, park, ur, ui, diag, offd, std::make_integer_sequence<int, CC>()), ...);
    return fma(2.0, offd[0] + offd[1], diag);
}

}  // namespace

}  // namespace abz
