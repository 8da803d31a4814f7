// LtmBlock: a device block of `sets` sets of planes that a rule keeps beside its eigenvalue planes (attached elements, the
// real and the complex integration weights of the tetrahedron method).  Nothing of HIP is needed here: a plain host
// compiler builds and tests the type (tests/c/ltm_block_main.cpp).
#pragma once
#include "dev_buf.h"
#include "plane_view.h"

namespace abz {

// double [ntiles][sets * planes_per_set planes][row]: the tiling of the eigenvalue planes it was made like -- same rows, same
// lines -- with all its planes in every tile, pitch = row.  Set i holds planes i * planes_per_set and on.  Move-only through
// its DevBuf; what is moved from owns nothing (buf.p == nullptr).  A new block is built in a local LtmBlock and moved into
// the rule once it is complete: the move lets the resident one go.
struct LtmBlock {
    DevBuf buf;
    PlaneView view;  // of buf
    int sets = 0;

    static size_t bytes(const PlaneView& like, int64_t ntiles, int planes) {
        return sizeof(double) * (size_t)ntiles * (size_t)planes * (size_t)like.row;
    }
    // bytes of the resident block, 0 when there is none
    size_t bytes(int64_t ntiles, int planes_per_set) const { return buf.p ? bytes(view, ntiles, sets * planes_per_set) : 0; }
    // a fresh block; a failure leaves this one empty
    int alloc(PlaneView like, int64_t ntiles, int planes_per_set, int nsets) {
        drop();
        const int planes = nsets * planes_per_set;
        const int rc = buf.alloc(bytes(like, ntiles, planes));
        if (rc) return rc;
        view = like;
        view.base = buf.as<double>();
        view.tile = (int64_t)planes * like.row;
        view.pitch = like.row;
        view.compact = 0;
        sets = nsets;
        return 0;
    }
    // the planes_per_set planes of set i
    PlaneView set_view(int i, int planes_per_set) const {
        PlaneView v = view;
        v.base += (int64_t)i * planes_per_set * v.pitch;
        return v;
    }
    void drop() {
        buf.release();
        view = PlaneView();
        sets = 0;
    }
};

}  // namespace abz
