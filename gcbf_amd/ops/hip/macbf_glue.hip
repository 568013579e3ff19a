// Glue of the no-grad MACBF actor over padded edge buffers (CDNA4/gfx950):
// the segment max between φ and γ, written straight into γ's padded bf16
// GEMM input.
//
//   segmax_rows_kernel   max over {e: seg[e] == node(r)} of msg[e] -> bf16 rows
//
// It replaces arange + searchsorted + int32 cast (the CSR pointer), the
// bf16 -> fp32 cast of φ's output, seg_max_fwd (segmax.hip), the row select,
// the zero pad and the fp32 -> bf16 cast by one launch.  The comparison is
// seg_max_fwd's: scan the segment in order from -FLT_MAX with ``v > m``, so
// the first maximal edge wins, a NaN never wins, and a segment with no
// winner (empty, or nothing above -FLT_MAX) gives 0.  A max selects one of
// its inputs, so the bf16 bits of the winner are stored as they were read:
// the result equals the fp32 composition bit for bit.
//
// A plain grid launch on the caller's stream (records under graph capture):
// no LDS, no barrier, no atomics, no cross-workgroup communication, no
// inline assembly, plain vector stores.
#include <hip/hip_runtime.h>

#include "segops_common.h"

// first index in seg[0:E) (non-decreasing) whose value is >= key
__device__ __forceinline__ int seg_first_ge(const long* __restrict__ seg,
                                            int E, long key) {
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per output row r; lanes own feature columns.  r < n_rows:
// the row of node idx[r], or of node r without an index; r >= n_rows, or a
// node outside [0, num_nodes): zeros.  Sentinel entries (seg == num_nodes)
// sort after every real segment and are never read, so msg rows past the
// real edges may hold anything.
__global__ void __launch_bounds__(SEG_BLOCK) segmax_rows_kernel(
        const unsigned short* __restrict__ msg,  // (>=E, D) bf16
        const long* __restrict__ seg,            // (E,) dst-sorted
        const long* __restrict__ idx,            // (n_rows,) or null
        unsigned short* __restrict__ out,        // (rows, D) bf16
        int E, int D, int n_rows, int num_nodes) {
    const int r = blockIdx.x;
    unsigned short* out_row = out + (size_t)r * D;
    const long node = r >= n_rows ? -1 : (idx != nullptr ? idx[r] : (long)r);
    int lo = 0, hi = 0;
    if (node >= 0 && node < num_nodes) {
        lo = seg_first_ge(seg, E, node);
        hi = seg_first_ge(seg, E, node + 1);
    }
    for (int d = threadIdx.x; d < D; d += SEG_BLOCK) {
        float m = -FLT_MAX;
        unsigned short best = 0;
        for (int e = lo; e < hi; ++e) {
            const unsigned short b = msg[(size_t)e * D + d];
            const float v = bf16_up(b);
            if (v > m) {
                m = v;
                best = b;
            }
        }
        out_row[d] = best;
    }
}

extern "C" void launch_segmax_rows_bf16(const void* msg, const long* seg,
                                        const long* idx, void* out, int E,
                                        int D, int n_rows, int num_nodes,
                                        int rows, hipStream_t stream) {
    hipLaunchKernelGGL(segmax_rows_kernel, dim3(rows), dim3(SEG_BLOCK), 0,
                       stream, (const unsigned short*)msg, seg, idx,
                       (unsigned short*)out, E, D, n_rows, num_nodes);
}
