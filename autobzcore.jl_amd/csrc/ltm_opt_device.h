// What the files of the optimized tetrahedron method share (kernels_ltm_opt.hip, kernels_ltm_green_opt.hip): the 20 stencil
// points of a Kuhn simplex in path coordinates, the projection 1260 P onto the 4 effective corner values, the form in which it is
// evaluated and the wrap of a stencil index.  kernels_ltm_opt.hip has the definition and the derivation; everything here is
// inlined into the kernels of the file that includes it.
#pragma once

#include <hip/hip_runtime.h>

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

}  // namespace

}  // namespace abz
