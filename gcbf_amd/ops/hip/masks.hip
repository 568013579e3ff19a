// Fused batched safety-mask kernels for CDNA4/gfx950.
//
// Computes the reference's per-agent safe / unsafe / collision masks
// (reference gcbf/env/simple_car.py:306-387, dubins_car.py:818-923,
// simple_drone.py:379-465) in ONE pass over the (B, n_agents, N) pairwise
// geometry — the reference loops graphs in Python and launches dozens of
// broadcast kernels per call.  One wave per agent row; lanes stride the
// sender dimension and reduce with ballots.
//
// Env kinds (mask geometry):
//   0 car2d:   P=2, cone dir = velocity (vx,vy)/|v|, warn 4r, safe thr 4r
//   1 dubins:  P=2, cone dir = heading (cosθ, sinθ), warn 3r, safe thr 3r
//   2 drone3d: P=3, cone dir = (vx/|v|, vy/|v|, vz)  [vz quirk], warn 4r,
//              safe thr 4r, unsafe-collision diag 2r+1
#include <hip/hip_runtime.h>
#include <cfloat>

#include "masks_common.h"

extern "C" __global__ void fused_masks(
        const float* __restrict__ states,  // (B*N, S)
        bool* __restrict__ safe,           // (B*n_rec,) or null
        bool* __restrict__ unsafe,         // (B*n_rec,) or null
        bool* __restrict__ collision,      // (B*n_rec,) or null
        int B, int N, int n_rec, int S, float r, int kind) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (row >= B * n_rec) return;
    const int b = row / n_rec, i = row % n_rec;
    bool w_all_safe, w_any_uns, w_any_coll;
    mask_row(states + (size_t)b * N * S, i, lane, N, S, r, kind,
             &w_all_safe, &w_any_uns, &w_any_coll);
    if (lane == 0) {
        if (safe) safe[row] = w_all_safe;
        if (unsafe) unsafe[row] = w_any_uns;
        if (collision) collision[row] = w_any_coll;
    }
}

extern "C" void launch_fused_masks(const float* states, bool* safe,
                                   bool* unsafe, bool* collision, int B,
                                   int N, int n_rec, int S, float r, int kind,
                                   hipStream_t stream) {
    const int rows = B * n_rec;
    const int blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(fused_masks, dim3(blocks),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream,
                       states, safe, unsafe, collision, B, N, n_rec, S, r,
                       kind);
}
