// Images of grid points under a set of integer symmetry matrices acting on grid indices mod npt: shared by the orbit
// tables of symmetric rules (kernels_symptr.hip) and the orbit map of unfolded tetrahedron rules (kernels_ltm.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace abz {

struct SymArgs {
    int npt, d, nsyms;
    int small;  // every |S v| < 2^31: 32-bit arithmetic (a 64-bit modulo costs ~4x more)
    int perm;   // every matrix is a signed permutation (cubic / inversion groups in the lattice basis): no modulo at all
    int group;  // the set is closed under multiplication (a group): orbit size = nsyms / |stabiliser|
    int64_t N;
    int S[48 * 9];  // up to 48 symmetries of a 3-d lattice, row-major
};

__device__ __forceinline__ int64_t sym_image(const SymArgs& a, const int* v, int s) {
    int64_t img = 0, mul = 1;
    if (a.perm) {  // row r has one entry +-1, in column c: the image coordinate is v[c] or (npt - v[c]) mod npt
        for (int r = 0; r < a.d; ++r) {
            int t = 0;
            for (int c = 0; c < a.d; ++c) {
                const int e = a.S[(s * a.d + r) * a.d + c];
                t = e > 0 ? v[c] : (e < 0 ? (v[c] == 0 ? 0 : a.npt - v[c]) : t);
            }
            img += (int64_t)t * mul;
            mul *= a.npt;
        }
        return img;
    }
    for (int r = 0; r < a.d; ++r) {
        int64_t t;
        if (a.small) {
            int t32 = 0;
            for (int c = 0; c < a.d; ++c) t32 += a.S[(s * a.d + r) * a.d + c] * v[c];
            t32 %= a.npt;
            if (t32 < 0) t32 += a.npt;
            t = t32;
        } else {
            t = 0;
            for (int c = 0; c < a.d; ++c) t += (int64_t)a.S[(s * a.d + r) * a.d + c] * v[c];
            t %= a.npt;
            if (t < 0) t += a.npt;
        }
        img += t * mul;
        mul *= a.npt;
    }
    return img;
}

// the arguments of nsyms <= 48 matrices of a d <= 3 dimensional lattice (callers check both); `group` is left 0
inline void sym_args_init(SymArgs& a, int npt, int d, const int32_t* syms, int nsyms) {
    a.npt = npt;
    a.d = d;
    a.nsyms = nsyms;
    a.N = 1;
    for (int j = 0; j < d; ++j) a.N *= npt;
    int64_t smax = 1;
    for (int i = 0; i < nsyms * d * d; ++i) {
        a.S[i] = syms[i];
        smax = std::max<int64_t>(smax, std::llabs((long long)syms[i]));
    }
    a.small = (smax * d * (int64_t)npt < ((int64_t)1 << 30)) ? 1 : 0;
    a.perm = 1;
    a.group = 0;
    for (int sidx = 0; sidx < nsyms && a.perm; ++sidx)
        for (int r = 0; r < d && a.perm; ++r) {
            int nz = 0;
            for (int c = 0; c < d; ++c) {
                const int e = syms[(sidx * d + r) * d + c];
                if (e != 0) nz += (e == 1 || e == -1) ? 1 : 2;
            }
            if (nz != 1) a.perm = 0;
        }
}

}  // namespace abz
