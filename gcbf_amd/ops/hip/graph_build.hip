// Fused batched radius-graph construction for CDNA4/gfx950.
//
// Replaces the reference's dense builder + Python top-k loop + edge_attr
// gather (reference gcbf/env/dubins_car.py:724-746) with two kernels:
//   count: one wave per receiver row (b, i) — pairwise distances, optional
//          k-nearest threshold, per-row edge count;
//   fill:  same decomposition — ordered compaction via wave ballots writes
//          edge_index AND edge_attr in one pass (edge ordering is row-major
//          over (graph, dst, src), matching torch.nonzero semantics).
//
// Host side does one cumsum between the two (torch.cumsum on device).
#include <hip/hip_runtime.h>
#include <cfloat>

#include "graph_build_common.h"

extern "C" __global__ void radius_count(
        const float* __restrict__ pos,   // (B*N, P)
        int* __restrict__ counts,        // (B*n_rec,)
        int B, int N, int n_rec, int P, float r, int topk) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (row >= B * n_rec) return;
    const int b = row / n_rec, i = row % n_rec;
    const int gbase = b * N;
    const int cnt = count_row(pos, P, P, gbase, i, N, r, topk, lane);
    if (lane == 0) counts[row] = cnt;
}

extern "C" __global__ void radius_fill(
        const float* __restrict__ pos,     // (B*N, P)
        const float* __restrict__ states,  // (B*N, S)
        const int* __restrict__ offsets,   // (B*n_rec,) exclusive scan
        long* __restrict__ edge_index,     // (2, E): [src row | dst row]
        float* __restrict__ edge_attr,     // (E, A)
        long E_total,
        int B, int N, int n_rec, int P, int S, int A,
        float r, int topk, int attr_kind) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (row >= B * n_rec) return;
    const int b = row / n_rec, i = row % n_rec;
    const int gbase = b * N;
    fill_row(pos, P, states, offsets[row], edge_index, edge_attr, E_total,
             gbase, i, N, P, S, A, r, topk, attr_kind, lane);
}

// Pad a built edge list out to a fixed capacity so every consumer shape is
// static (hipGraph capture of the rollout loop).  Real edges [0, E) get
// seg = dst (for CSR segment ops); pad entries get src = dst = 0 (a valid
// gather index) and seg = N_total (a sentinel past the last node, so CSR
// segments skip them), edge_attr = 0.  Also publishes E to a device scalar.
extern "C" __global__ void pad_edges(
        const int* __restrict__ offsets,   // (rows,) exclusive scan
        const int* __restrict__ counts,    // (rows,)
        long* __restrict__ edge_index,     // (2, E_max)
        long* __restrict__ seg,            // (E_max,)
        float* __restrict__ edge_attr,     // (E_max, A)
        int* __restrict__ e_count,         // (1,) out
        int rows, long E_max, long N_total, int A) {
    const long E = (long)offsets[rows - 1] + counts[rows - 1];
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) *e_count = (int)E;
    if (idx >= E_max) return;
    pad_entry(idx, E, edge_index, seg, edge_attr, E_max, N_total, A);
}

extern "C" void launch_pad_edges(const int* offsets, const int* counts,
                                 long* edge_index, long* seg,
                                 float* edge_attr, int* e_count, int rows,
                                 long E_max, long N_total, int A,
                                 hipStream_t stream) {
    const int threads = 256;
    const int blocks = (int)((E_max + threads - 1) / threads);
    hipLaunchKernelGGL(pad_edges, dim3(blocks > 0 ? blocks : 1),
                       dim3(threads), 0, stream, offsets, counts, edge_index,
                       seg, edge_attr, e_count, rows, E_max, N_total, A);
}

// ------------------------------------------------------------- launchers
extern "C" void launch_radius_count(const float* pos, int* counts, int B,
                                    int N, int n_rec, int P, float r,
                                    int topk, hipStream_t stream) {
    const int rows = B * n_rec;
    const int blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(radius_count, dim3(blocks),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream,
                       pos, counts, B, N, n_rec, P, r, topk);
}

extern "C" void launch_radius_fill(const float* pos, const float* states,
                                   const int* offsets, long* edge_index,
                                   float* edge_attr, long E_total, int B,
                                   int N, int n_rec, int P, int S, int A,
                                   float r, int topk, int attr_kind,
                                   hipStream_t stream) {
    const int rows = B * n_rec;
    const int blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(radius_fill, dim3(blocks),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream,
                       pos, states, offsets, edge_index, edge_attr, E_total,
                       B, N, n_rec, P, S, A, r, topk, attr_kind);
}
