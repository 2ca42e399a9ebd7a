// lnerf_hashgrid_cell.h -- the cell arithmetic of the hash grid (include/lnerf.h "Multiresolution hash
// grid"), shared by lnerf_hashgrid.hip and lnerf_hashgrid_sorted.hip so that both form the same
// cells, entry indices and weights. Device code only; float64 throughout; build with
// -ffp-contract=off.
#ifndef LNERF_HASHGRID_CELL_H
#define LNERF_HASHGRID_CELL_H

#include "lnerf_hashgrid.h"

namespace lnerf {

// One axis of a point at one level: u = clamp((p - lo) / ext, 0, 1) with a NaN taken as 0,
// pos = u (res - 1), cell i = min(floor(pos), res - 2) in 0..res-2 and weight w = pos - i in [0, 1].
// live: the clamp left u as it was (the coordinate is inside the box, its edges included); only
// then does the output depend on the coordinate.
__device__ __forceinline__ void hg_axis(float p, double lo, double ext, int res, int& i, double& w, bool& live) {
    const double u_raw = ((double)p - lo) / ext;
    live = u_raw >= 0.0 && u_raw <= 1.0;
    const double u = u_raw > 0.0 ? (u_raw < 1.0 ? u_raw : 1.0) : 0.0;
    const double pos = u * (double)(res - 1);
    int c = (int)floor(pos);
    c = c < res - 2 ? c : res - 2;
    i = c;
    w = pos - (double)c;
}

struct HgCell {
    int i[3];
    double w[3];
    bool live[3];
};

__device__ __forceinline__ HgCell hg_cell(const HgParams& g, int res, const float* __restrict__ p3) {
    HgCell c;
#pragma unroll
    for (int a = 0; a < 3; ++a) hg_axis(p3[a], g.lo[a], g.ext[a], res, c.i[a], c.w[a], c.live[a]);
    return c;
}

// corner k: bit a of k is the offset along axis a
__device__ __forceinline__ unsigned hg_index(const HgCell& c, int k, int res, int dense, unsigned mask) {
    const unsigned gx = (unsigned)(c.i[0] + (k & 1)), gy = (unsigned)(c.i[1] + ((k >> 1) & 1)),
                   gz = (unsigned)(c.i[2] + ((k >> 2) & 1));
    return dense ? gx + (unsigned)res * (gy + (unsigned)res * gz)
                 : ((gx ^ (gy * 2654435761u) ^ (gz * 805459861u)) & mask);
}

__device__ __forceinline__ double hg_weight(const HgCell& c, int k) {
    const double wx = (k & 1) ? c.w[0] : 1.0 - c.w[0];
    const double wy = (k & 2) ? c.w[1] : 1.0 - c.w[1];
    const double wz = (k & 4) ? c.w[2] : 1.0 - c.w[2];
    return wx * wy * wz;
}

}  // namespace lnerf
#endif
