// Segment (per-destination) attention aggregation kernels for CDNA4/gfx950.
//
// Replaces the reference's torch_scatter-based PyG AttentionalAggregation
// (reference gcbf/nn/gnn.py:17-19): scatter-softmax of a per-edge gate over
// incoming edges of each node, then the softmax-weighted sum of per-edge
// messages.  Edge lists are destination-sorted (CSR via `ptr`), so each
// segment is contiguous: no atomics, deterministic reduction order, bitwise
// reproducible across runs.
//
// Decomposition: one 256-thread workgroup (4 waves of 64) per destination
// node.  The per-edge att / dot-product scratch is staged through the output
// buffers themselves (same-workgroup global RAW after __syncthreads is
// coherent), so no degree-dependent LDS: any segment size works and
// occupancy stays high.
#include <hip/hip_runtime.h>
#include <cfloat>

#include "segops_common.h"

#define BLOCK SEG_BLOCK
#define WAVE SEG_WAVE

// ---------------------------------------------------------------- forward
extern "C" __global__ void seg_attn_fwd(
        const float* __restrict__ msg,    // (E, D)
        const float* __restrict__ gate,   // (E,)
        const int* __restrict__ ptr,      // (N+1,)
        float* __restrict__ att,          // (E,)  out
        float* __restrict__ out,          // (N, D) out
        int N, int D) {
    const int n = blockIdx.x;
    if (n >= N) return;
    __shared__ __attribute__((aligned(16))) float red[4];
    // body shared with mlp_glue.hip (segops_common.h)
    seg_attn_row(msg, gate, ptr[n], ptr[n + 1], att, out + (size_t)n * D, D,
                 red);
}

// ---------------------------------------------------------------- backward
// dmsg[e] = att[e] * g_n ;  s_e = <msg_e, g_n> ;
// dgate[e] = att[e] * (s_e - sum_{e' in n} att_e' s_e')
// s_e is staged in dgate itself between the two passes.
extern "C" __global__ void seg_attn_bwd(
        const float* __restrict__ grad_out,  // (N, D)
        const float* __restrict__ msg,       // (E, D)
        const float* __restrict__ att,       // (E,)
        const int* __restrict__ ptr,         // (N+1,)
        float* __restrict__ dmsg,            // (E, D) out
        float* __restrict__ dgate,           // (E,)  out
        int N, int D) {
    const int n = blockIdx.x;
    if (n >= N) return;
    __shared__ __attribute__((aligned(16))) float red[4];
    // body shared with mlp_glue.hip (segops_common.h)
    seg_attn_bwd_row<true>(grad_out + (size_t)n * D, msg, att, ptr[n],
                           ptr[n + 1], dmsg, dgate, dgate, D, red);
}

// ------------------------------------------------------------- launchers
extern "C" void launch_seg_attn_fwd(const float* msg, const float* gate,
                                    const int* ptr, float* att, float* out,
                                    int N, int D, hipStream_t stream) {
    hipLaunchKernelGGL(seg_attn_fwd, dim3(N), dim3(BLOCK), 0, stream,
                       msg, gate, ptr, att, out, N, D);
}

extern "C" void launch_seg_attn_bwd(const float* grad_out, const float* msg,
                                    const float* att, const int* ptr,
                                    float* dmsg, float* dgate, int N, int D,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(seg_attn_bwd, dim3(N), dim3(BLOCK), 0, stream,
                       grad_out, msg, att, ptr, dmsg, dgate, N, D);
}
