// lnerf_occgrid.h -- what lnerf_api.cpp and lnerf_occgrid.hip share: the validated, kernel-side
// form of an lnerf_occgrid (include/lnerf.h "Occupancy grid") and the launchers.
#ifndef LNERF_OCCGRID_H
#define LNERF_OCCGRID_H

#include <hip/hip_runtime.h>

#include "lnerf.h"

namespace lnerf {

struct OccParams {
    int res, shift;          // cells per axis = 1 << shift
    long long cells;         // res^3, a multiple of 64
    double lo[3], ext[3];    // the box: lo and (double)hi - (double)lo
};

// The callers have validated every argument (n >= 1, the pointers each kernel reads and writes
// non-NULL, the sampler's M a multiple of 64 in 64..1024 and 1 <= S <= 1024).
void k_occgrid_cell_points(const OccParams& g, const int* cells, long long n, const float* u, float* points,
                           hipStream_t s);
void k_occgrid_update(const OccParams& g, float* density, const int* cells, long long n, const float* sigma,
                      int sigma_stride, float decay, hipStream_t s);
// doubles of stream-ordered scratch lnerf_occgrid_threshold needs (the stage-1 partial sums, then thr)
int occgrid_threshold_scratch(const OccParams& g);
void k_occgrid_threshold(const OccParams& g, const float* density, float threshold, int flags, unsigned* bits,
                         double* mean, long long* occupied, double* scratch, hipStream_t s);
void k_sample_occupancy(const OccParams& g, const unsigned* bits, const float* rays, int n, int S, int steps,
                        float near_t, float far_t, const float* u, int flags, float* sample_t, float* dists,
                        int* n_occ, hipStream_t s);

}  // namespace lnerf
#endif
