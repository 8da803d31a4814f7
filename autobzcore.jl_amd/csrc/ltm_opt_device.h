// What the files of the optimized tetrahedron method share (kernels_ltm_opt.hip, kernels_ltm_green_opt.hip and the two files of
// node weights through ltm_opt_nodew_device.h): the 20 stencil points of a Kuhn simplex in path coordinates, the projection
// 1260 P onto the 4 effective corner values and the form in which it is evaluated, the wrap of a stencil index, the stencil
// addressing of a path (OptPath), and what the two scans have in common: their sources, the shared part of their arguments, the
// effective elements of a simplex and the opening of their launchers.  kernels_ltm_opt.hip has the definition and the
// derivation; everything here is inlined into the kernels of the file that includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abz_internal.h"
#include "ltm_device.h"

namespace abz {

namespace {

// The 20 points in path coordinates: p = v1 + al e_a + be e_b + ga e_c.
constexpr int OPT_NPT = 20;
__device__ constexpr int OPT_PT[OPT_NPT][3] = {
    {0, 0, 0},    {1, 0, 0},   {1, 1, 0},   {1, 1, 1},                                                   // v1 .. v4
    {-1, 0, 0},   {1, -1, 0},  {1, 1, -1},  {2, 2, 2},                                                   // 2 v_i - v_j: (1,2) (2,3) (3,4) (4,1)
    {-1, -1, 0},  {1, -1, -1}, {2, 2, 0},   {1, 2, 2},                                                   // (1,3) (2,4) (3,1) (4,2)
    {-1, -1, -1}, {2, 0, 0},   {1, 2, 0},   {1, 1, 2},                                                   // (1,4) (2,1) (3,2) (4,3)
    {2, 1, 1},    {0, 1, 0},   {1, 0, 1},   {0, 0, -1},                                                  // v4 - v1 + v2, ...
};
// 1260 P
__device__ constexpr int OPT_K[4][OPT_NPT] = {
    {1440, 0, 30, 0, -38, 7, 17, -28, -56, 9, -46, 9, -38, -28, 17, 7, -18, -18, 12, -18},
    {0, 1440, 0, 30, -28, -38, 7, 17, 9, -56, 9, -46, 7, -38, -28, 17, -18, -18, -18, 12},
    {30, 0, 1440, 0, 17, -28, -38, 7, -46, 9, -56, 9, 17, 7, -38, -28, 12, -18, -18, -18},
    {0, 30, 0, 1440, 7, 17, -28, -38, 9, -46, 9, -56, -28, 17, 7, -38, -18, 12, -18, -18},
};
constexpr bool opt_rows_ok() {
    for (int m = 0; m < 4; ++m) {
        int s = 0;
        for (int j = 0; j < OPT_NPT; ++j) s += OPT_K[m][j];
        if (s != 1260) return false;
    }
    return true;
}
static_assert(opt_rows_ok(), "the rows of 1260 P sum to 1260");

// x'_m = x_m + sum_{j != m} P[m][j] (x_j - x_m)
__device__ __forceinline__ void opt_project(const double (&x)[OPT_NPT], double (&y)[4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < OPT_NPT; ++j)
            if (j != m && OPT_K[m][j] != 0) s = fma((double)OPT_K[m][j] / 1260.0, x[j] - x[m], s);
        y[m] = x[m] + s;
    }
}

// index i + o of a periodic axis of npt >= 1 points, o in -1 .. 2
__device__ __forceinline__ int opt_wrap(int i, int o, int npt) {
    int j = i + o;
    j += j < 0 ? npt : 0;
    j -= j >= npt ? npt : 0;
    j -= j >= npt ? npt : 0;  // npt = 1: i + 2 is two periods away
    return j;
}

// The wrapped indices i - 1 .. i + 2 of every axis of the cell (i1, i2, i3): a column (axis 1) or a line number (axis 2; axis 3 in
// units of npt lines).
__device__ __forceinline__ void opt_tables(int i1, int i2, int i3, int npt, int (&j1)[4], int (&j2)[4], int (&j3)[4]) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        j1[o] = opt_wrap(i1, o - 1, npt);
        j2[o] = opt_wrap(i2, o - 1, npt);
        j3[o] = opt_wrap(i3, o - 1, npt) * npt;
    }
}

// THE stencil addressing of path t = 0 .. 5: the permutation (X, Y, Z) of the axes, as in the queue of ltm_window_kernel (corners
// 0, e_X, e_X + e_Y, (1,1,1)), and what a step of o - 1 along the path's first, second and third axis adds to the column and to
// the line.  The tables are picked from the three index tables of a walk by compares on the permutation, and every point is
// three constant-index entries of them: nothing is indexed by a run-time value, nothing goes to scratch.  j1, j2: indices of
// the axes 1, 2; j3: of axis 3, times the lines of a plane -- opt_tables for a walk forward over the grid, the tables of
// ltm_opt_nodew_gather_kernel for its walk back over the workspace.
struct OptPath {
    int col[3][4], line[3][4];
    __device__ __forceinline__ OptPath(int t, const int (&j1)[4], const int (&j2)[4], const int (&j3)[4]) {
        const int X = t >> 1, Y = (X + 1 + (t & 1)) % 3, Z = 3 - X - Y;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            col[0][o] = X == 0 ? j1[o] : 0;
            col[1][o] = Y == 0 ? j1[o] : 0;
            col[2][o] = Z == 0 ? j1[o] : 0;
            line[0][o] = X == 1 ? j2[o] : (X == 2 ? j3[o] : 0);
            line[1][o] = Y == 1 ? j2[o] : (Y == 2 ? j3[o] : 0);
            line[2][o] = Z == 1 ? j2[o] : (Z == 2 ? j3[o] : 0);
        }
    }
    // point j of the stencil: its column and its line, inside the ranges of the index tables (on the grid 0 .. npt-1 and 0 .. npt^2-1)
    __device__ __forceinline__ int col_of(int j) const { return col[0][OPT_PT[j][0] + 1] + col[1][OPT_PT[j][1] + 1] + col[2][OPT_PT[j][2] + 1]; }
    __device__ __forceinline__ int line_of(int j) const { return line[0][OPT_PT[j][0] + 1] + line[1][OPT_PT[j][1] + 1] + line[2][OPT_PT[j][2] + 1]; }
    // x <- the 20 points of a band's planes.  `tile`, the stride between lines, is a 32-bit factor (the host checks it): line * tile is
    // then ONE 32 x 32 -> 64 bit multiply-add per point, where the 64 x 64 bit product took three quarter-rate multiplies and set
    // the scan's time
    __device__ __forceinline__ void load(const double* __restrict__ planes, int tile, double (&x)[OPT_NPT]) const {
#pragma unroll
        for (int j = 0; j < OPT_NPT; ++j) x[j] = planes[(int64_t)line_of(j) * tile + col_of(j)];
    }
};

// ---- the two scans (ltm_opt_kernel, ltm_green_opt_kernel) ---------------------------------------------------------------

// the source of the elements: A' = 1, A' = e', attached components
enum { OPT_ONE = 0, OPT_ENERGY = 1, OPT_ELEMS = 2 };

// what the arguments of both scan kernels begin with
struct OptScanArgs {
    PlaneView E, A;
    int64_t ncell;  // npt^3
    int64_t acomp;  // doubles from a band's plane of one component to its plane of the next: n * A.pitch
    int npt;
    int aplane0;    // first element plane of this launch: (its first component) * n
};

// the planes of band blockIdx.y: its eigenvalues and, under OPT_ELEMS, the first component of the launch
template <int SRC>
struct OptBand {
    const double* Eb;
    const double* Ab = nullptr;
    int tileE, tileA = 0;
    int64_t acomp = 0;
    __device__ __forceinline__ explicit OptBand(const OptScanArgs& a) : Eb(a.E.base + (int64_t)blockIdx.y * a.E.pitch), tileE((int)a.E.tile) {
        if constexpr (SRC == OPT_ELEMS) {
            Ab = a.A.base + (int64_t)(a.aplane0 + (int)blockIdx.y) * a.A.pitch;
            tileA = (int)a.A.tile;
            acomp = a.acomp;
        }
    }
};

// A[m] <- the effective elements of the path's simplex at its corner m: 1, the effective energies e, or the projection of the NC
// attached components (20 loads and one product each)
template <int SRC, int NC>
__device__ __forceinline__ void opt_elements(const OptPath& path, const OptBand<SRC>& b, const double (&e)[4], LtmVec<NC> (&A)[4]) {
    if constexpr (SRC == OPT_ELEMS) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double x[OPT_NPT], y[4];
            path.load(b.Ab + (int64_t)c * b.acomp, b.tileA, x);
            opt_project(x, y);
#pragma unroll
            for (int m = 0; m < 4; ++m) A[m].v[c] = y[m];
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) A[m].v[0] = SRC == OPT_ENERGY ? e[m] : 1.0;
    }
}

// The opening of both scan launchers.  A == nullptr: one component, A = 1 (`energy` false) or A = e (`energy` true).  Refuses a
// line stride beyond the kernels' 32-bit factor in the name of `who`; fills a, the source and the carve-up of the cells into
// nblocks blocks per band, nrows rows of partial sums.
inline int opt_scan_open(const char* who, int n, int npt, PlaneView E, const PlaneView* A, bool energy, int& ncomp, OptScanArgs& a, int& src,
                         int64_t& nblocks, int64_t& nrows) {
    src = A ? OPT_ELEMS : (energy ? OPT_ENERGY : OPT_ONE);
    if (!A) ncomp = 1;
    if (E.tile > INT32_MAX || (A && A->tile > INT32_MAX)) {
        set_error("%s: a stride of %lld doubles between grid lines does not fit the kernel's 32-bit factor", who,
                  (long long)std::max(E.tile, A ? A->tile : 0));
        return ABZ_ERR_UNSUPPORTED;
    }
    a.E = E;
    a.npt = npt;
    a.ncell = (int64_t)npt * npt * npt;
    if (A) {
        a.A = *A;
        a.acomp = (int64_t)n * A->pitch;
    }
    nblocks = std::min<int64_t>(cdiv64(a.ncell, 256), std::max(64, std::min(2048, 8192 / n)));
    nrows = nblocks * n;
    return ABZ_OK;
}

}  // namespace

}  // namespace abz
