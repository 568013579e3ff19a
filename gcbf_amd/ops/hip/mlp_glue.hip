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
// The update's grad-mode forwards use the same three and, for backward,
//
//   edge_inputs_bwd_kernel         edge_attr columns of dIn -> fp32
//   attn_gamma_in_bwd_gate_kernel  gradient of the gate (seg_attn_bwd_row)
//   attn_gamma_in_bwd_msg_kernel   bf16(att * g + gate MLP's msg gradient)
//   rows_cat_bwd_kernel            first Da columns of the real rows
//
// which write the zero pad rows of their outputs themselves.
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

// d_edge_attr[e, j] = float(dIn[e, 2*nd + j]) for e < E: what the cast, the
// row slice and the cat hand back to edge_attr (x takes no gradient).
__global__ void edge_inputs_bwd_kernel(
        const unsigned short* __restrict__ din,  // (>=E, 2*nd+ed) bf16
        float* __restrict__ dea,                 // (E, ed)
        int nd, int ed, long E) {
    const int W = 2 * nd + ed;
    const long total = E * ed;
    for (long i = blockIdx.x * (long)GLUE_BLOCK + threadIdx.x; i < total;
         i += (long)gridDim.x * GLUE_BLOCK) {
        const long e = i / ed;
        const int j = (int)(i - e * ed);
        dea[i] = bf16_up(din[e * W + 2 * nd + j]);
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

// One workgroup per output row r.  r < n_rows: [Σ_e att_e msg_e, x[node]]
// over the edges with seg == node, where node = idx[r], or r without an
// index; r >= n_rows, or a node outside [0, num_nodes): zeros.  Sentinel
// entries (seg == num_nodes) sort after every real segment and are never
// touched.  att keeps the normalised weight of every edge of a row's node.
template <typename GateT>
__global__ void __launch_bounds__(SEG_BLOCK) attn_gamma_in_kernel(
        const unsigned short* __restrict__ msg,  // (>=E, D) bf16
        const GateT* __restrict__ gate,          // (>=E,)
        const long* __restrict__ seg,            // (E,) dst-sorted
        const float* __restrict__ x,             // (>=num_nodes, nd)
        const long* __restrict__ idx,            // (n_rows,) or null
        float* __restrict__ att,                 // (E,) out
        unsigned short* __restrict__ out,        // (rows, D+nd) bf16
        int E, int D, int nd, int n_rows, int num_nodes) {
    const int r = blockIdx.x;
    const int W = D + nd;
    unsigned short* out_row = out + (size_t)r * W;
    const long node = r >= n_rows ? -1 : (idx != nullptr ? idx[r] : (long)r);
    if (node < 0 || node >= num_nodes) {
        for (int d = threadIdx.x; d < W; d += SEG_BLOCK) out_row[d] = 0;
        return;
    }
    __shared__ __attribute__((aligned(16))) float red[4];
    const int lo = seg_lower_bound(seg, E, node);
    const int hi = seg_lower_bound(seg, E, node + 1);
    seg_attn_row(msg, gate, lo, hi, att, out_row, D, red);
    for (int j = threadIdx.x; j < nd; j += SEG_BLOCK)
        out_row[D + j] = bf16_rne(x[(size_t)node * nd + j]);
}

// Backward, in two launches because the gate MLP's backward runs between
// them: it turns dgate into the gradient dmsg_gate that the second needs.
// One workgroup per output row r < n_rows, as in the forward.  Each also
// owns the edge slots between the previous row's segment and its own, and
// the last one every slot after its segment, so both kernels write every
// row of their output (idx must be strictly increasing).  The last row's
// workgroup thus writes up to a bucket of pad slots on its own: at most 255
// rows of D elements, nothing next to the GEMMs around it.  `rows` counts the
// edge slots of the padded outputs, rows >= E.
struct GlueSpan { int gap, lo, hi, end, real; bool ok; };

__device__ __forceinline__ GlueSpan glue_span(
        const long* __restrict__ seg, const long* __restrict__ idx, int E,
        int r, int n_rows, int num_nodes, int rows) {
    GlueSpan s;
    const long node = idx != nullptr ? idx[r] : (long)r;
    s.ok = node >= 0 && node < num_nodes;
    s.gap = 0;
    if (r > 0) {
        const long prev = idx != nullptr ? idx[r - 1] : (long)r - 1;
        s.gap = seg_lower_bound(seg, E, prev + 1);
    }
    s.lo = s.ok ? seg_lower_bound(seg, E, node) : s.gap;
    s.hi = s.ok ? seg_lower_bound(seg, E, node + 1) : s.gap;
    if (s.lo < s.gap) s.lo = s.gap;       // unsorted idx: stay in our slots
    if (s.hi < s.lo) s.hi = s.lo;
    // first sentinel slot; the last row owns [hi, rows)
    s.real = seg_lower_bound(seg, E, (long)num_nodes);
    s.end = r == n_rows - 1 ? rows : s.hi;
    return s;
}

// dgate[e] = bf16(att_e * (s_e - Σ att s)) on the edges of the row's node,
// 0 on every other slot.
__global__ void __launch_bounds__(SEG_BLOCK) attn_gamma_in_bwd_gate_kernel(
        const unsigned short* __restrict__ dout,  // (>=n_rows, D+nd) bf16
        const unsigned short* __restrict__ msg,   // (rows, D) bf16
        const float* __restrict__ att,            // (E,)
        const long* __restrict__ seg,             // (E,)
        const long* __restrict__ idx,             // (n_rows,) or null
        float* __restrict__ stage,                // (E,) scratch
        unsigned short* __restrict__ dgate,       // (rows,) bf16 out
        int E, int D, int nd, int n_rows, int num_nodes, int rows) {
    const int r = blockIdx.x;
    const GlueSpan s = glue_span(seg, idx, E, r, n_rows, num_nodes, rows);
    for (int e = s.gap + threadIdx.x; e < s.lo; e += SEG_BLOCK) dgate[e] = 0;
    for (int e = s.hi + threadIdx.x; e < s.end; e += SEG_BLOCK) dgate[e] = 0;
    __shared__ __attribute__((aligned(16))) float red[4];
    seg_attn_bwd_row<false>(dout + (size_t)r * (D + nd), msg, att, s.lo, s.hi,
                            (float*)nullptr, stage, dgate, D, red);
}

// dmsg[e] = bf16(att_e * g + float(dmsg_gate[e])) on the edges of the row's
// node: both contributions meet in fp32 and are rounded once, as where they
// met at a φ with fp32 output (plain last layer).  A φ with bf16 output
// (spectral-normed last layer) met them in bf16, after att_e * g had been
// rounded to bf16 on its own: round_prod.  Real edges of nodes no row
// selects keep dmsg_gate: the gate kernel wrote dgate = 0 there, so their
// att * g term is zero as it was eagerly (eagerly 0 + dmsg_gate turned a
// -0 into +0, here it stays -0; equal as numbers and in every GEMM).
// Sentinel and pad slots are 0.
__global__ void __launch_bounds__(SEG_BLOCK) attn_gamma_in_bwd_msg_kernel(
        const unsigned short* __restrict__ dout,       // (>=n_rows, D+nd)
        const float* __restrict__ att,                 // (E,)
        const long* __restrict__ seg,                  // (E,)
        const long* __restrict__ idx,                  // (n_rows,) or null
        const unsigned short* __restrict__ dmsg_gate,  // (rows, D) bf16
        unsigned short* __restrict__ dmsg,             // (rows, D) bf16 out
        int E, int D, int nd, int n_rows, int num_nodes, int rows,
        int round_prod) {
    const int r = blockIdx.x;
    const GlueSpan s = glue_span(seg, idx, E, r, n_rows, num_nodes, rows);
    const unsigned short* g = dout + (size_t)r * (D + nd);
    const long first = (long)s.gap * D, last = (long)s.end * D;
    for (long i = first + threadIdx.x; i < last; i += SEG_BLOCK) {
        const int e = (int)(i / D);
        unsigned short v = 0;
        if (e >= s.lo && e < s.hi) {
            // the product is rounded on its own before the sum, as where
            // seg_attn_bwd stores it: no contraction into an fma here
#pragma clang fp contract(off)
            const int d = (int)(i - (long)e * D);
            float p = att[e] * bf16_up(g[d]);
            if (round_prod) p = bf16_up(bf16_rne(p));
            v = bf16_rne(p + bf16_up(dmsg_gate[i]));
        } else if (e < s.real) {
            v = dmsg_gate[i];
        }
        dmsg[i] = v;
    }
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

// da[r] = dIn[r, 0:Da] for r < n_rows, zero rows after (b takes no gradient)
__global__ void rows_cat_bwd_kernel(
        const unsigned short* __restrict__ din,  // (rows, Da+Db) bf16
        unsigned short* __restrict__ da,         // (rows, Da) bf16
        int Da, int Db, long n_rows, long rows) {
    const long total = rows * Da;
    for (long i = blockIdx.x * (long)GLUE_BLOCK + threadIdx.x; i < total;
         i += (long)gridDim.x * GLUE_BLOCK) {
        const long r = i / Da;
        const int c = (int)(i - r * Da);
        da[i] = r < n_rows ? din[r * (Da + Db) + c] : (unsigned short)0;
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

extern "C" void launch_edge_inputs_bwd(const void* din, float* dea, int nd,
                                       int ed, long E, hipStream_t stream) {
    hipLaunchKernelGGL(edge_inputs_bwd_kernel, dim3(glue_blocks(E * ed)),
                       dim3(GLUE_BLOCK), 0, stream,
                       (const unsigned short*)din, dea, nd, ed, E);
}

extern "C" void launch_attn_gamma_in(const void* msg, const void* gate,
                                     int gate_is_bf16, const long* seg,
                                     const float* x, const long* idx,
                                     float* att, void* out, int E, int D,
                                     int nd, int n_rows, int num_nodes,
                                     int rows, hipStream_t stream) {
    if (gate_is_bf16)
        hipLaunchKernelGGL(attn_gamma_in_kernel<unsigned short>, dim3(rows),
                           dim3(SEG_BLOCK), 0, stream,
                           (const unsigned short*)msg,
                           (const unsigned short*)gate, seg, x, idx, att,
                           (unsigned short*)out, E, D, nd, n_rows,
                           num_nodes);
    else
        hipLaunchKernelGGL(attn_gamma_in_kernel<float>, dim3(rows),
                           dim3(SEG_BLOCK), 0, stream,
                           (const unsigned short*)msg, (const float*)gate,
                           seg, x, idx, att, (unsigned short*)out, E, D, nd,
                           n_rows, num_nodes);
}

extern "C" void launch_attn_gamma_in_bwd_gate(
        const void* dout, const void* msg, const float* att, const long* seg,
        const long* idx, float* stage, void* dgate, int E, int D, int nd,
        int n_rows, int num_nodes, int rows, hipStream_t stream) {
    hipLaunchKernelGGL(attn_gamma_in_bwd_gate_kernel, dim3(n_rows),
                       dim3(SEG_BLOCK), 0, stream,
                       (const unsigned short*)dout,
                       (const unsigned short*)msg, att, seg, idx, stage,
                       (unsigned short*)dgate, E, D, nd, n_rows, num_nodes,
                       rows);
}

extern "C" void launch_attn_gamma_in_bwd_msg(
        const void* dout, const float* att, const long* seg, const long* idx,
        const void* dmsg_gate, void* dmsg, int E, int D, int nd, int n_rows,
        int num_nodes, int rows, int round_prod, hipStream_t stream) {
    hipLaunchKernelGGL(attn_gamma_in_bwd_msg_kernel, dim3(n_rows),
                       dim3(SEG_BLOCK), 0, stream,
                       (const unsigned short*)dout, att, seg, idx,
                       (const unsigned short*)dmsg_gate,
                       (unsigned short*)dmsg, E, D, nd, n_rows, num_nodes,
                       rows, round_prod);
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

extern "C" void launch_rows_cat_bwd(const void* din, void* da, int Da, int Db,
                                    long n_rows, long rows,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(rows_cat_bwd_kernel, dim3(glue_blocks(rows * Da)),
                       dim3(GLUE_BLOCK), 0, stream,
                       (const unsigned short*)din, (unsigned short*)da, Da,
                       Db, n_rows, rows);
}

extern "C" void launch_refresh_mirrors(const long long* table, int n_layers,
                                       long max_groups, hipStream_t stream) {
    int bx = glue_blocks(max_groups);
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(refresh_mirrors_kernel, dim3(bx, n_layers),
                       dim3(GLUE_BLOCK), 0, stream, table);
}
