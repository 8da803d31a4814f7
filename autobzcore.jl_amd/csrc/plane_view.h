// PlaneView: the addressing of rule values.  Nothing of HIP is needed here (tests/c/ltm_block_main.cpp).
#pragma once
#include <cstdint>

namespace abz {

// Tiled planar addressing of rule values: nodes are grouped in tiles of `line_len` consecutive nodes
// (a grid line, or 64 nodes of an irregular list); a tile stores all its planes back to back, each
// plane row `pitch` doubles long (pitch >= line_len, multiple of 16 = 128 B).  Element (node k,
// plane p) = base[(k / line_len) * tile + p * pitch + k % line_len].  One wave writes one tile: a
// single contiguous ~27 KB HBM region instead of 21 streams 27 MB apart (1.7x the write bandwidth,
// tools/micro/wtest.hip).
// The same formula carries the PADDED PLANAR layout of full-grid rules (ABZ_RULE_PLANAR): tile = row (the stride from one
// grid line to the next inside a plane), pitch = nlines * row (the stride from one plane to the next), so every plane is one
// dense array of padded rows and all resident waves write it as one front (tools/micro/placement.hip).  `row` is the padded
// row length either way (columns line_len .. row-1 of a row are padding).
struct PlaneView {
    double* base = nullptr;  // first plane of this array inside tile 0
    int64_t tile = 0;        // doubles from one line (tile) to the next
    int pitch = 0;           // doubles from one plane to the next
    int line_len = 1;
    int row = 0;             // padded row length (multiple of 16 doubles = 128 B)
    int compact = 0;         // H planes of a Hermitian rule stored as the upper triangle only (ABZ_WANT_H_COMPACT): = n
};

}  // namespace abz
