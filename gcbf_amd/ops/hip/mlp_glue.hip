// Glue between the library GEMMs of the no-grad actor forward, and the bf16
// weight-mirror refresh (CDNA4/gfx950).
//
// The captured actor spends more launches between its 13 GEMMs than on
// them: gathers, cats, zero pads, fp32<->bf16 casts, slices, a CSR pointer
// build.  None of that changes a value the result depends on.  The kernels
// here write the padded bf16 GEMM inputs directly:
//
//   edge_inputs_kernel    [x[dst], x[src], edge_attr] -> bf16 (rows_padded, W)
//   attn_gamma_in_kernel  softmax-weighted message sum ++ x[r] -> bf16 rows
//   rows_cat_pad_kernel   [a_bf16, b_fp32] -> bf16 (rows_padded, Da+Db)
//   refresh_mirrors_kernel  every fp32 master of a module -> its bf16 mirror
//
// All are plain grid launches on the caller's stream (they record under
// graph capture): no atomics, no cross-workgroup communication, no inline
// assembly, plain vector stores.  fp32 -> bf16 is round-to-nearest-even
// (bf16_rne, segops_common.h), the conversion of torch's .bfloat16(); the
// attention arithmetic is seg_attn_row, the body seg_attn_fwd runs.
#include <hip/hip_runtime.h>

#include "segops_common.h"

#define GLUE_BLOCK 256

// ------------------------------------------------------------ edge inputs
// out[e] = [x[dst_e], x[src_e], edge_attr[e]] for e < E, zero rows after.
// An edge whose src or dst is outside [0, N) contributes zeros for that part.
__global__ void edge_inputs_kernel(
        const float* __restrict__ x,        // (N, nd)
        const long* __restrict__ ei,        // (2, E): src row, dst row
        const float* __restrict__ ea,       // (E, ed)
        unsigned short* __restrict__ out,   // (rows, 2*nd+ed) bf16
        int N, int nd, int ed, long E, long rows) {
    const int W = 2 * nd + ed;
    const long total = rows * W;
    for (long i = blockIdx.x * (long)GLUE_BLOCK + threadIdx.x; i < total;
         i += (long)gridDim.x * GLUE_BLOCK) {
        const long e = i / W;
        const int c = (int)(i - e * W);
        float v = 0.f;
        if (e < E) {
            if (c < 2 * nd) {
                const long node = c < nd ? ei[E + e] : ei[e];
                if (node >= 0 && node < N)
                    v = x[node * nd + (c < nd ? c : c - nd)];
            } else {
                v = ea[e * ed + (c - 2 * nd)];
            }
        }
        out[i] = bf16_rne(v);
    }
}

// ------------------------------------------------- aggregation -> γ input
// first index in seg[0:E) (non-decreasing) whose value is >= key
__device__ __forceinline__ int seg_lower_bound(const long* __restrict__ seg,
                                               int E, long key) {
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per output row r.  r < n_rows: [Σ_e att_e msg_e, x[r]] over
// the edges with seg == r; r >= n_rows: zeros.  Sentinel entries (seg ==
// num_nodes > r) sort after every real segment and are never touched.
template <typename GateT>
__global__ void __launch_bounds__(SEG_BLOCK) attn_gamma_in_kernel(
        const unsigned short* __restrict__ msg,  // (>=E, D) bf16
        const GateT* __restrict__ gate,          // (>=E,)
        const long* __restrict__ seg,            // (E,) dst-sorted
        const float* __restrict__ x,             // (>=n_rows, nd)
        float* __restrict__ att,                 // (E,) scratch
        unsigned short* __restrict__ out,        // (rows, D+nd) bf16
        int E, int D, int nd, int n_rows) {
    const int r = blockIdx.x;
    const int W = D + nd;
    unsigned short* out_row = out + (size_t)r * W;
    if (r >= n_rows) {
        for (int d = threadIdx.x; d < W; d += SEG_BLOCK) out_row[d] = 0;
        return;
    }
    __shared__ __attribute__((aligned(16))) float red[4];
    const int lo = seg_lower_bound(seg, E, r);
    const int hi = seg_lower_bound(seg, E, (long)r + 1);
    seg_attn_row(msg, gate, lo, hi, att, out_row, D, red);
    for (int j = threadIdx.x; j < nd; j += SEG_BLOCK)
        out_row[D + j] = bf16_rne(x[(size_t)r * nd + j]);
}

// ------------------------------------------------------- cat + pad + cast
__global__ void rows_cat_pad_kernel(
        const unsigned short* __restrict__ a,   // (>=n_rows, Da) bf16
        const float* __restrict__ b,            // (>=n_rows, Db) fp32
        unsigned short* __restrict__ out,       // (rows, Da+Db) bf16
        int Da, int Db, long n_rows, long rows) {
    const int W = Da + Db;
    const long total = rows * W;
    for (long i = blockIdx.x * (long)GLUE_BLOCK + threadIdx.x; i < total;
         i += (long)gridDim.x * GLUE_BLOCK) {
        const long r = i / W;
        const int c = (int)(i - r * W);
        unsigned short v = 0;
        if (r < n_rows)
            v = c < Da ? a[r * Da + c] : bf16_rne(b[r * Db + (c - Da)]);
        out[i] = v;
    }
}

// --------------------------------------------------------- mirror refresh
// table (n, 8) int64, one row per Linear:
//   [fp32 weight (rows, K), bf16 mirror (rows, K64), rows, K, K64,
//    fp32 bias (rows,) or 0, bf16 bias mirror, fp32 bias copy]
// blockIdx.y selects the layer, blockIdx.x strides over groups of four
// mirror columns (K64 % 64 == 0), pad columns [K, K64) are written as zero.
#define MIRROR_FIELDS 8

__global__ void refresh_mirrors_kernel(const long long* __restrict__ table) {
    const long long* t = table + (size_t)blockIdx.y * MIRROR_FIELDS;
    const float* __restrict__ w = reinterpret_cast<const float*>(t[0]);
    unsigned short* __restrict__ wb = reinterpret_cast<unsigned short*>(t[1]);
    const long rows = t[2];
    const int K = (int)t[3], K64 = (int)t[4];
    const float* __restrict__ b = reinterpret_cast<const float*>(t[5]);
    unsigned short* __restrict__ bb = reinterpret_cast<unsigned short*>(t[6]);
    float* __restrict__ b32 = reinterpret_cast<float*>(t[7]);

    const int G = K64 >> 2;
    const long groups = rows * G;
    const bool vec = (K & 3) == 0;
    const long stride = (long)gridDim.x * GLUE_BLOCK;
    const long first = blockIdx.x * (long)GLUE_BLOCK + threadIdx.x;
    for (long i = first; i < groups; i += stride) {
        const long row = i / G;
        const int k = (int)(i - row * G) << 2;
        const float* src = w + row * K;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec) {
            if (k < K) v = *reinterpret_cast<const float4*>(src + k);
        } else {
            if (k + 0 < K) v.x = src[k + 0];
            if (k + 1 < K) v.y = src[k + 1];
            if (k + 2 < K) v.z = src[k + 2];
            if (k + 3 < K) v.w = src[k + 3];
        }
        uint2 o;
        o.x = (unsigned int)bf16_rne(v.x) | ((unsigned int)bf16_rne(v.y) << 16);
        o.y = (unsigned int)bf16_rne(v.z) | ((unsigned int)bf16_rne(v.w) << 16);
        *reinterpret_cast<uint2*>(wb + row * K64 + k) = o;
    }
    if (b != nullptr) {
        for (long i = first; i < rows; i += stride) {
            const float v = b[i];
            bb[i] = bf16_rne(v);
            b32[i] = v;
        }
    }
}

// ------------------------------------------------------------- launchers
static inline int glue_blocks(long total) {
    long nb = (total + GLUE_BLOCK - 1) / GLUE_BLOCK;
    if (nb < 1) nb = 1;
    return (int)(nb > 4096 ? 4096 : nb);
}

extern "C" void launch_edge_inputs_bf16(const float* x, const long* ei,
                                        const float* ea, void* out, int N,
                                        int nd, int ed, long E, long rows,
                                        hipStream_t stream) {
    hipLaunchKernelGGL(edge_inputs_kernel,
                       dim3(glue_blocks(rows * (2 * nd + ed))),
                       dim3(GLUE_BLOCK), 0, stream, x, ei, ea,
                       (unsigned short*)out, N, nd, ed, E, rows);
}

extern "C" void launch_attn_gamma_in(const void* msg, const void* gate,
                                     int gate_is_bf16, const long* seg,
                                     const float* x, float* att, void* out,
                                     int E, int D, int nd, int n_rows,
                                     int rows, hipStream_t stream) {
    if (gate_is_bf16)
        hipLaunchKernelGGL(attn_gamma_in_kernel<unsigned short>, dim3(rows),
                           dim3(SEG_BLOCK), 0, stream,
                           (const unsigned short*)msg,
                           (const unsigned short*)gate, seg, x, att,
                           (unsigned short*)out, E, D, nd, n_rows);
    else
        hipLaunchKernelGGL(attn_gamma_in_kernel<float>, dim3(rows),
                           dim3(SEG_BLOCK), 0, stream,
                           (const unsigned short*)msg, (const float*)gate,
                           seg, x, att, (unsigned short*)out, E, D, nd,
                           n_rows);
}

extern "C" void launch_rows_cat_pad_bf16(const void* a, const float* b,
                                         void* out, int Da, int Db,
                                         long n_rows, long rows,
                                         hipStream_t stream) {
    hipLaunchKernelGGL(rows_cat_pad_kernel,
                       dim3(glue_blocks(rows * (Da + Db))), dim3(GLUE_BLOCK),
                       0, stream, (const unsigned short*)a, b,
                       (unsigned short*)out, Da, Db, n_rows, rows);
}

extern "C" void launch_refresh_mirrors(const long long* table, int n_layers,
                                       long max_groups, hipStream_t stream) {
    int bx = glue_blocks(max_groups);
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(refresh_mirrors_kernel, dim3(bx, n_layers),
                       dim3(GLUE_BLOCK), 0, stream, table);
}
