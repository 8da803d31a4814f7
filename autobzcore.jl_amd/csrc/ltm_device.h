// What the tetrahedron files share (kernels_ltm.hip, kernels_ltm_green.hip, kernels_ltm_nodew.hip): the mesh's constants, the
// cell geometry of a whole periodic grid and the element load of a corner.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace abz {

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr int ltm_nsimplex(int d) { return d == 3 ? 6 : (d == 2 ? 2 : 1); }  // simplices per cell

// dynamic LDS of the plain g scan at 1024 energies: 5 x 1024 x 8 B + queue and counts; every scan stays within it
constexpr size_t LTM_LDS_MAX = sizeof(double) * 5 * 1024 + sizeof(uint32_t) * (256 + 8);

// Cell k of a walk over npt^D cells -> its indices (i1 fastest; i3 = 0 below D = 3).  32-bit divisions wherever k allows them.
// By value: with three int& results the 2-d slab window kernels compile to other code (profiles/ltm_green_refactor_vs_parent.txt).
struct LtmCell {
    int i1, i2, i3;
};
template <int D>
__device__ __forceinline__ LtmCell ltm_cell(int64_t k, int npt) {
    const int64_t line = k <= 0xffffffffll ? (int64_t)((uint32_t)k / (uint32_t)npt) : k / npt;
    const int i1 = (int)(k - line * npt);
    const int i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
    const int i2 = (int)line - i3 * npt;
    return {i1, i2, i3};
}

// THE whole-grid geometry: corner `bits` (bit j: +1 along variable j+1) of cell (i1, i2, i3), which become the corner's own
// indices, every one wrapped mod npt.  The corner is column i1 of line i3 npt + i2 of a band's planes.
template <int D>
__device__ __forceinline__ void ltm_wrap(int& i1, int& i2, int& i3, int bits, int npt) {
    if ((bits & 1) && ++i1 == npt) i1 = 0;
    if (D >= 2 && (bits & 2) && ++i2 == npt) i2 = 0;
    if (D == 3 && (bits & 4) && ++i3 == npt) i3 = 0;
}

// the elements a corner carries besides its energy
template <int NC>
struct LtmVec {
    double v[NC];
};

// the NC components of the corner whose first one lies at p, `acomp` doubles apart
template <int NC>
__device__ __forceinline__ LtmVec<NC> ltm_load(const double* __restrict__ p, int64_t acomp) {
    LtmVec<NC> r;
#pragma unroll
    for (int c = 0; c < NC; ++c) r.v[c] = p[(int64_t)c * acomp];
    return r;
}

}  // namespace abz
