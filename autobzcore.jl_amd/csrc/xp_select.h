// Helpers of the kernels that turn operator planes into matrix elements of the tetrahedron method (kernels_ltm_expect.hip,
// kernels_ltm_pairs.hip): the plane of an upper-triangle entry in either H layout, and reads / writes of a small register array at a
// uniform run-time index.  gfx950 only.
#pragma once
#include <utility>

#include "abz_internal.h"

namespace abz {

namespace {

// plane of Re X[a][b], a <= b (Im: the next one; the diagonal of the compact layout has none)
__device__ __forceinline__ int xp_plane(const PlaneView& v, int n, int a, int b) { return v.compact ? b * b + 2 * a : 2 * (a + n * b); }

// q[i] of the register array and q[k] = v, i and k uniform: select chains over values that were read first (with the element
// read inside the conditional expression the chain became a chain of addresses and one load at a run-time offset: the array
// left the registers)
template <int K, int... M>
__device__ __forceinline__ double xp_pick(const double (&q)[K], int i, std::integer_sequence<int, M...>) {
    double v = q[0];
    ((void)([&] {
         const double x = q[M + 1];
         v = (i == M + 1) ? x : v;
     }()),
     ...);
    return v;
}
template <int K>
__device__ __forceinline__ double xp_pick(const double (&q)[K], int i) {
    return xp_pick(q, i, std::make_integer_sequence<int, K - 1>());
}
template <int K, int... M>
__device__ __forceinline__ void xp_put(double (&q)[K], int k, double v, std::integer_sequence<int, M...>) {
    ((void)([&] {
         const double old = q[M];
         q[M] = (k == M) ? v : old;
     }()),
     ...);
}
template <int K>
__device__ __forceinline__ void xp_put(double (&q)[K], int k, double v) {
    xp_put(q, k, v, std::make_integer_sequence<int, K>());
}

}  // namespace

}  // namespace abz
