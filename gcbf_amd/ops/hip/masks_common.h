// Per-wave body of the fused safety-mask kernel, shared by masks.hip (one
// wave per agent row over a grid) and rollout_tail.hip (rows looped inside
// one workgroup).  Both call mask_row, so the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "env_step_common.h"  // WAVE, ROWS_PER_BLOCK

#define ENV_CAR 0
#define ENV_DUBINS 1
#define ENV_DRONE 2

// Masks of agent row i against the N nodes of one graph.  ``states`` points
// at the graph's first row.  Every lane of the wave must call with the same
// i; the three results are wave-uniform.
__device__ inline void mask_row(const float* states, int i, int lane, int N,
                                int S, float r, int kind, bool* w_all_safe,
                                bool* w_any_uns, bool* w_any_coll) {
    const int P = (kind == ENV_DRONE) ? 3 : 2;

    const float* si = states + (size_t)i * S;

    // per-row cone direction
    float dir0 = 0.f, dir1 = 0.f, dir2 = 0.f;
    if (kind == ENV_CAR) {
        const float v = sqrtf(si[2] * si[2] + si[3] * si[3]) + 1e-5f;
        dir0 = si[2] / v;
        dir1 = si[3] / v;
    } else if (kind == ENV_DUBINS) {
        dir0 = cosf(si[2]);
        dir1 = sinf(si[2]);
    } else {
        const float v = sqrtf(si[3] * si[3] + si[4] * si[4] +
                              si[5] * si[5]) + 1e-5f;
        dir0 = si[3] / v;
        dir1 = si[4] / v;
        dir2 = si[5];  // reference quirk: vz not normalized
    }

    const float safe_thr = (kind == ENV_DUBINS) ? 3.f * r : 4.f * r;
    const float warn = (kind == ENV_DUBINS) ? 3.f * r : 4.f * r;
    // diagonal offsets per mask (match the reference's +eye*(c+1) exactly)
    const float diag_safe = 4.f * r + 1.f;
    const float diag_unsafe = (kind == ENV_DRONE) ? 2.f * r + 1.f
                                                  : 4.f * r + 1.f;
    const float diag_coll = 2.f * r + 1.f;

    bool all_safe = true;
    bool any_unsafe = false;
    bool any_coll = false;

    for (int j = lane; j < N; j += WAVE) {
        const float* sj = states + (size_t)j * S;
        float pd[3] = {0.f, 0.f, 0.f};
        float d2 = 0.f;
        for (int c = 0; c < P; ++c) {
            pd[c] = si[c] - sj[c];
            d2 += pd[c] * pd[c];
        }
        const float d = sqrtf(d2);
        const float dself = (i == j) ? 1.f : 0.f;  // i==j only when j<n_rec

        const float d_safe = d + dself * diag_safe;
        const float d_uns = d + dself * diag_unsafe;
        const float d_coll = d + dself * diag_coll;

        all_safe &= (d_safe > safe_thr);
        any_coll |= (d_coll < 2.f * r);

        // heading/velocity cone (unsafe direction)
        bool cone = false;
        {
            const float inv = 1.f / (d + 1e-4f);
            // pos_vec = -(pd)/(|pd|+1e-4) : direction i -> j
            const float inner = -(pd[0] * dir0 + pd[1] * dir1 +
                                  pd[2] * dir2) * inv;
            const float ratio = 2.f * r / (d_uns + 1e-7f);
            // ratio > 1 -> asin NaN -> comparison false (matches torch)
            const float thr = cosf(asinf(ratio));
            cone = (inner > thr) && (d_uns < warn);
        }
        any_unsafe |= (d_uns < 2.f * r) || cone;
    }

    *w_all_safe = __all(all_safe);
    *w_any_uns = __any(any_unsafe);
    *w_any_coll = __any(any_coll);
}
