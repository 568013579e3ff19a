// Per-wave bodies of the radius-graph builder, shared by graph_build.hip
// (count / fill / pad kernels over a grid) and rollout_tail.hip (the same
// rows looped inside one workgroup).  Both call these functions, so the two
// cannot drift apart.  Positions are read with an explicit row stride so a
// caller can point ``pos`` at the leading columns of the state matrix.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

#include "env_step_common.h"  // WAVE, ROWS_PER_BLOCK

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v = fminf(v, __shfl_down(v, off, WAVE));
    return __shfl(v, 0, WAVE);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return __shfl(v, 0, WAVE);
}

// adjusted pairwise distance: self-edge pushed out of range like the
// reference's +eye*(r+1) trick
__device__ __forceinline__ float row_dist(const float* pos, int P, int stride,
                                          int gbase, int i, int j,
                                          float big) {
    const float* pi = pos + (size_t)(gbase + i) * stride;
    const float* pj = pos + (size_t)(gbase + j) * stride;
    float d2 = 0.f;
#pragma unroll 3
    for (int c = 0; c < P; ++c) {
        const float t = pi[c] - pj[c];
        d2 += t * t;
    }
    float d = sqrtf(d2);
    if (i == j) d += big;
    return d;
}

// k-th smallest adjusted distance in the row (duplicates counted), matching
// torch.topk(k, largest=False).values[-1]
__device__ __forceinline__ float kth_smallest(const float* pos, int P,
                                              int stride, int gbase, int i,
                                              int N, float big, int k,
                                              int lane) {
    float kth = -FLT_MAX;
    int remaining = k;
    while (remaining > 0) {
        float lmin = FLT_MAX;
        for (int j = lane; j < N; j += WAVE) {
            const float d = row_dist(pos, P, stride, gbase, i, j, big);
            if (d > kth) lmin = fminf(lmin, d);
        }
        const float m = wave_min(lmin);
        int cnt = 0;
        for (int j = lane; j < N; j += WAVE)
            cnt += (row_dist(pos, P, stride, gbase, i, j, big) == m);
        remaining -= wave_sum_i(cnt);
        kth = m;
    }
    return kth;
}

// neighbour-cap threshold of receiver row i (FLT_MAX: no cap)
__device__ __forceinline__ float row_kth(const float* pos, int P, int stride,
                                         int gbase, int i, int N, float big,
                                         int topk, int lane) {
    float kth = FLT_MAX;
    if (topk > 0 && topk < N)
        kth = kth_smallest(pos, P, stride, gbase, i, N, big, topk, lane);
    return kth;
}

// edge count of receiver row i under a given cap threshold ``kth`` (from
// row_kth; wave-uniform)
__device__ __forceinline__ int count_row_thr(const float* pos, int P,
                                             int stride, int gbase, int i,
                                             int N, float r, float kth,
                                             int lane) {
    const float big = r + 1.f;
    int cnt = 0;
    for (int j = lane; j < N; j += WAVE) {
        const float d = row_dist(pos, P, stride, gbase, i, j, big);
        cnt += (d < r && d <= kth);
    }
    return wave_sum_i(cnt);
}

// edge count of receiver row i (wave-uniform)
__device__ __forceinline__ int count_row(const float* pos, int P, int stride,
                                         int gbase, int i, int N, float r,
                                         int topk, int lane) {
    const float kth = row_kth(pos, P, stride, gbase, i, N, r + 1.f, topk,
                              lane);
    return count_row_thr(pos, P, stride, gbase, i, N, r, kth, lane);
}

// edge_attr kinds
#define ATTR_DIFF 0    // states[src] - states[dst], S dims
#define ATTR_DUBINS 1  // [x,y,th,v cos th,v sin th] diff, 5 dims

__device__ __forceinline__ void write_attr(float* attr, const float* states,
                                           int S, int kind, long src,
                                           long dst) {
    const float* ss = states + (size_t)src * S;
    const float* sd = states + (size_t)dst * S;
    if (kind == ATTR_DIFF) {
        for (int c = 0; c < S; ++c) attr[c] = ss[c] - sd[c];
    } else {  // ATTR_DUBINS: S == 4 -> 5 attr dims
        attr[0] = ss[0] - sd[0];
        attr[1] = ss[1] - sd[1];
        attr[2] = ss[2] - sd[2];
        attr[3] = ss[3] * cosf(ss[2]) - sd[3] * cosf(sd[2]);
        attr[4] = ss[3] * sinf(ss[2]) - sd[3] * sinf(sd[2]);
    }
}

// ordered, ballot-compacted fill of receiver row i starting at edge ``base``
// under a given cap threshold ``kth`` (from row_kth)
__device__ __forceinline__ void fill_row_thr(const float* pos, int stride,
                                             const float* states, int base,
                                             long* edge_index,
                                             float* edge_attr, long E_total,
                                             int gbase, int i, int N, int P,
                                             int S, int A, float r, float kth,
                                             int attr_kind, int lane) {
    const float big = r + 1.f;

    for (int j0 = 0; j0 < N; j0 += WAVE) {
        const int j = j0 + lane;
        bool pred = false;
        if (j < N) {
            const float d = row_dist(pos, P, stride, gbase, i, j, big);
            pred = (d < r && d <= kth);
        }
        const unsigned long long mask = __ballot(pred);
        if (pred) {
            const int off = base + __popcll(mask & ((1ull << lane) - 1ull));
            // guard: with a soft capacity (padded engine buffers) the edge
            // count can exceed E_total — skip writes; the host detects the
            // overflow from the published count and redoes the step eagerly
            if (off < E_total) {
                const long src = gbase + j;
                const long dst = gbase + i;
                edge_index[off] = src;
                edge_index[E_total + off] = dst;
                write_attr(edge_attr + (size_t)off * A, states, S, attr_kind,
                           src, dst);
            }
        }
        base += __popcll(mask);
    }
}

// ordered, ballot-compacted fill of receiver row i starting at edge ``base``
__device__ __forceinline__ void fill_row(const float* pos, int stride,
                                         const float* states, int base,
                                         long* edge_index, float* edge_attr,
                                         long E_total, int gbase, int i,
                                         int N, int P, int S, int A, float r,
                                         int topk, int attr_kind, int lane) {
    const float kth = row_kth(pos, P, stride, gbase, i, N, r + 1.f, topk,
                              lane);
    fill_row_thr(pos, stride, states, base, edge_index, edge_attr, E_total,
                 gbase, i, N, P, S, A, r, kth, attr_kind, lane);
}

// entry idx < E_max of the padded edge list holding E real edges: real
// edges get seg = dst, pad entries src = dst = 0, seg = N_total, attr = 0
__device__ __forceinline__ void pad_entry(long idx, long E, long* edge_index,
                                          long* seg, float* edge_attr,
                                          long E_max, long N_total, int A) {
    if (idx < E) {
        seg[idx] = edge_index[E_max + idx];  // dst
    } else {
        edge_index[idx] = 0;
        edge_index[E_max + idx] = 0;
        seg[idx] = N_total;
        for (int c = 0; c < A; ++c) edge_attr[idx * A + c] = 0.f;
    }
}
