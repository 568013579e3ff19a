// Episode-reset rejection sampling for CDNA4/gfx950.
//
// Greedy sequential rejection sampling over a pre-drawn candidate stream,
// the device form of env/utils.py:rejection_sample_positions (reference
// gcbf/env/simple_car.py:97-121): walk the candidates in order and accept
// one iff it is farther than min_sep from the origin (the reference tests
// against a zero-initialised buffer, so the origin is always "occupied"),
// from every point accepted so far, and farther than avoid_dist from every
// avoid point.  All decisions compare squared fp32 distances
// (d2 <= thr*thr rejects), no sqrt.
//
// One 64-lane wavefront per problem (grid = B, block = 64).  Accepted points
// live in LDS.  The stream is consumed in chunks of 64 candidates, one per
// lane:
//   1. every lane tests its candidate against the origin, the accepted list
//      as of the start of the chunk (LDS broadcast reads) and the avoid set;
//   2. the chunk is resolved in stream order with a wave ballot: the lowest
//      passing lane is accepted and its point broadcast; every higher
//      passing lane tests against it and clears itself on conflict; repeat.
//      A lane is only ever tested against lanes that were ACCEPTED, so a
//      candidate that conflicts with an earlier but rejected candidate is
//      still accepted, exactly like the sequential loop.
// Consumption stops the moment count == n (used = index of the last consumed
// candidate + 1); if the pool runs out first, used = C and count < n.  pts
// and count are in/out, so a caller can resume with a fresh pool.
// No atomics; deterministic.
#include <hip/hip_runtime.h>

#define WAVE 64

template <int DIM>
__device__ __forceinline__ float dist2(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        const float d = a[k] - b[k];
        s += d * d;
    }
    return s;
}

template <int DIM>
__global__ __launch_bounds__(WAVE) void reset_sample_kernel(
        const float* __restrict__ cand,     // (B, C, DIM)
        const float* __restrict__ min_sep,  // (B,)
        const float* __restrict__ avoid,    // (B, A, DIM)
        float avoid_dist,
        float* __restrict__ pts,            // (B, n, DIM) in/out
        int* __restrict__ count,            // (B,) in/out
        int* __restrict__ used,             // (B,)
        int C, int A, int n) {
    extern __shared__ float acc[];          // n * DIM accepted points
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const float* cand_b = cand + (size_t)b * C * DIM;
    const float* avoid_b = avoid + (size_t)b * A * DIM;
    float* pts_b = pts + (size_t)b * n * DIM;

    const float sep = min_sep[b];
    const float sep2 = sep * sep;
    const float av2 = avoid_dist * avoid_dist;

    // resume: points accepted by earlier pools
    const int cnt0 = min(max(count[b], 0), n);
    for (int i = lane; i < cnt0 * DIM; i += WAVE) acc[i] = pts_b[i];
    __syncthreads();

    int cnt = cnt0;
    int used_v = 0;
    for (int c0 = 0; c0 < C && cnt < n; c0 += WAVE) {
        const int c = c0 + lane;
        float p[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) p[k] = 0.f;
        bool pass = c < C;  // the last chunk may be partial
        if (pass) {
#pragma unroll
            for (int k = 0; k < DIM; ++k) p[k] = cand_b[(size_t)c * DIM + k];
            float zero[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) zero[k] = 0.f;
            pass = dist2<DIM>(zero, p) > sep2;
            for (int j = 0; j < cnt; ++j)
                pass = pass && (dist2<DIM>(&acc[j * DIM], p) > sep2);
            for (int a = 0; a < A; ++a)
                pass = pass && (dist2<DIM>(&avoid_b[(size_t)a * DIM], p) > av2);
        }

        // in-order resolution of the chunk (all lanes active here)
        int last = -1;
        unsigned long long m = __ballot(pass);
        while (m != 0ull && cnt < n) {
            const int l = __ffsll((long long)m) - 1;  // lowest passing lane
            float q[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) q[k] = __shfl(p[k], l, WAVE);
            if (lane == l) {
#pragma unroll
                for (int k = 0; k < DIM; ++k) acc[cnt * DIM + k] = p[k];
                pass = false;  // consumed
            } else if (pass && lane > l) {
                pass = dist2<DIM>(q, p) > sep2;
            }
            ++cnt;
            last = l;
            m = __ballot(pass);
        }
        used_v = (cnt == n) ? c0 + last + 1 : min(c0 + WAVE, C);
        __syncthreads();  // acc writes visible to the next chunk's pre-test
    }

    for (int i = cnt0 * DIM + lane; i < cnt * DIM; i += WAVE)
        pts_b[i] = acc[i];
    if (lane == 0) {
        count[b] = cnt;
        used[b] = used_v;
    }
}

extern "C" void launch_reset_sample(const float* cand, const float* min_sep,
                                    const float* avoid, float avoid_dist,
                                    float* pts, int* count, int* used, int B,
                                    int C, int A, int n, int dim,
                                    hipStream_t stream) {
    const size_t lds = (size_t)n * dim * sizeof(float);
    if (dim == 2)
        hipLaunchKernelGGL(reset_sample_kernel<2>, dim3(B), dim3(WAVE), lds,
                           stream, cand, min_sep, avoid, avoid_dist, pts,
                           count, used, C, A, n);
    else
        hipLaunchKernelGGL(reset_sample_kernel<3>, dim3(B), dim3(WAVE), lds,
                           stream, cand, min_sep, avoid, avoid_dist, pts,
                           count, used, C, A, n);
}
