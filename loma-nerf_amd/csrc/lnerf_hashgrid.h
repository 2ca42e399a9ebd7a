// lnerf_hashgrid.h -- what lnerf_api.cpp and lnerf_hashgrid.hip share: the validated, kernel-side
// form of an lnerf_hashgrid (include/lnerf.h "Multiresolution hash grid") and the launchers.
#ifndef LNERF_HASHGRID_H
#define LNERF_HASHGRID_H

#include <hip/hip_runtime.h>

#include "lnerf.h"

namespace lnerf {

// LDS floats a workgroup of the d_table kernel owns: a dense level of at most this many values
// (entries * F) is summed there and flushed once (lnerf_hashgrid.hip).
constexpr int kHgLdsFloats = 8192;

struct HgLevel {
    long long offset;   // the level's first entry
    int res;            // grid points per axis
    int dense;          // 1: index g_x + res (g_y + res g_z); 0: the hash, masked to T - 1
    int lds_blocks;     // d_table kernel: > 0 = workgroups that sum this level in LDS; 0 = the merge path
    int pad;
};

struct HgParams {
    int levels, features;
    unsigned mask;                            // T - 1
    double lo[3], ext[3];                     // the box: lo and (double)hi - (double)lo
    HgLevel lv[LNERF_HASHGRID_MAX_LEVELS];
};

// The callers have validated every argument (R >= 1, F in {1, 2, 4, 8}, the pointers each kernel
// reads and writes non-NULL and aligned).
void k_hashgrid_encode(const HgParams& g, const float* table, const float* points, long long R, float* encoded,
                       hipStream_t s);
// g.lv[l].lds_blocks is filled here (it depends on R).
void k_hashgrid_grad_table(HgParams g, const float* points, long long R, const float* d_encoded, const float* scale,
                           float* d_table, hipStream_t s);
void k_hashgrid_grad_points(const HgParams& g, const float* table, const float* points, long long R,
                            const float* d_encoded, const float* scale, float* d_points, hipStream_t s);

// lnerf_hashgrid_sorted.hip: d_table under LNERF_HASHGRID_REPRODUCIBLE. R <= 2^28; d_table aligned
// like the table and, without `accumulate`, zeroed by the caller. `scratch` holds the bytes
// k_hashgrid_sorted_scratch_bytes gives for the same g and R; the work is enqueued on s, level by
// level. Either returns the first HIP error it meets (what was enqueued before it still runs).
hipError_t k_hashgrid_sorted_scratch_bytes(const HgParams& g, long long R, hipStream_t s, size_t* bytes);
hipError_t k_hashgrid_grad_table_sorted(const HgParams& g, const float* points, long long R, const float* d_encoded,
                                        const float* scale, bool accumulate, float* d_table, void* scratch,
                                        hipStream_t s);

}  // namespace lnerf
#endif
