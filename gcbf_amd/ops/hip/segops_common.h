// Per-segment bodies of the CSR attention aggregation, shared by
// seg_attn_fwd / seg_attn_bwd (segops.hip, fp32 in / fp32 out) and the
// attn_gamma_in kernels (mlp_glue.hip, bf16 messages in / bf16 rows out),
// forward (seg_attn_row) and backward (seg_attn_bwd_row).  One 256-thread
// workgroup owns one destination node; the arithmetic is fp32 in one fixed
// order (max, exp, sum, normalise, weighted sum), so both callers produce
// the same fp32 accumulators bit for bit.  Loads upcast (exact), the store
// converts at the very end.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

#define SEG_BLOCK 256
#define SEG_WAVE 64

// fp32 -> bf16 bits, round to nearest even, NaN -> 0x7FC0 (the conversion
// torch's .bfloat16() performs)
__device__ __forceinline__ unsigned short bf16_rne(float f) {
    const unsigned int u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float bf16_up(unsigned short b) {
    return __uint_as_float(((unsigned int)b) << 16);
}

// element access by storage type: float is fp32, unsigned short is bf16 bits
__device__ __forceinline__ float seg_ld(const float* p, size_t i) {
    return p[i];
}
__device__ __forceinline__ float seg_ld(const unsigned short* p, size_t i) {
    return bf16_up(p[i]);
}
// four consecutive elements starting at element 4*i4 of a row whose start
// is aligned to four elements
__device__ __forceinline__ float4 seg_ld4(const float* row, int i4) {
    return reinterpret_cast<const float4*>(row)[i4];
}
__device__ __forceinline__ float4 seg_ld4(const unsigned short* row, int i4) {
    const uint2 v = reinterpret_cast<const uint2*>(row)[i4];
    return make_float4(__uint_as_float(v.x << 16),
                       __uint_as_float(v.x & 0xffff0000u),
                       __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xffff0000u));
}
__device__ __forceinline__ void seg_st(float* p, int i, float v) { p[i] = v; }
__device__ __forceinline__ void seg_st(unsigned short* p, int i, float v) {
    p[i] = bf16_rne(v);
}
// out_row needs no alignment beyond its element type for the bf16 store
__device__ __forceinline__ void seg_st4(float* row, int i4, float4 v) {
    reinterpret_cast<float4*>(row)[i4] = v;
}
__device__ __forceinline__ void seg_st4(unsigned short* row, int i4,
                                        float4 v) {
    row[4 * i4 + 0] = bf16_rne(v.x);
    row[4 * i4 + 1] = bf16_rne(v.y);
    row[4 * i4 + 2] = bf16_rne(v.z);
    row[4 * i4 + 3] = bf16_rne(v.w);
}

// like seg_ld4 for a row with no alignment beyond its element type (a bf16
// row of an odd-width matrix); fp32 rows of D % 4 == 0 are always aligned
__device__ __forceinline__ float4 seg_ld4_any(const float* row, int i4) {
    return reinterpret_cast<const float4*>(row)[i4];
}
__device__ __forceinline__ float4 seg_ld4_any(const unsigned short* row,
                                              int i4) {
    return make_float4(bf16_up(row[4 * i4 + 0]), bf16_up(row[4 * i4 + 1]),
                       bf16_up(row[4 * i4 + 2]), bf16_up(row[4 * i4 + 3]));
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
    for (int off = SEG_WAVE / 2; off > 0; off >>= 1)
        v += __shfl_down(v, off, SEG_WAVE);
    return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
    for (int off = SEG_WAVE / 2; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_down(v, off, SEG_WAVE));
    return v;
}

__device__ __forceinline__ float block_reduce_sum(float v, float* red,
                                                  int wid, int lane) {
    v = wave_reduce_sum(v);
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// out_row[0:D] = sum over edges e in [lo, hi) of softmax(gate)[e] * msg[e].
// Called by every thread of a SEG_BLOCK-thread workgroup with the same
// (lo, hi); `att` (E,) fp32 is the per-edge staging buffer (same-workgroup
// global RAW after __syncthreads), `red` four floats of LDS.  An empty
// segment writes zeros.  msg rows are D elements apart and, when D % 4 == 0,
// read four at a time.
template <typename MsgT, typename GateT, typename OutT>
__device__ __forceinline__ void seg_attn_row(
        const MsgT* __restrict__ msg, const GateT* __restrict__ gate,
        int lo, int hi, float* __restrict__ att, OutT* __restrict__ out_row,
        int D, float* red) {
    const int deg = hi - lo;
    const int tid = threadIdx.x;
    const int wid = tid / SEG_WAVE, lane = tid % SEG_WAVE;

    if (deg == 0) {
        for (int d = tid; d < D; d += SEG_BLOCK) seg_st(out_row, d, 0.f);
        return;
    }

    // 1) segment max of gate
    float m = -FLT_MAX;
    for (int e = tid; e < deg; e += SEG_BLOCK)
        m = fmaxf(m, seg_ld(gate, lo + e));
    m = wave_reduce_max(m);
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));

    // 2) exp, stage into att, segment sum
    float s = 0.f;
    for (int e = tid; e < deg; e += SEG_BLOCK) {
        const float x = __expf(seg_ld(gate, lo + e) - m);
        att[lo + e] = x;
        s += x;
    }
    s = block_reduce_sum(s, red, wid, lane);
    const float inv = 1.f / (s + 1e-16f);

    // 3) normalize in place
    for (int e = tid; e < deg; e += SEG_BLOCK) att[lo + e] *= inv;
    __syncthreads();

    // 4) out[:] = sum_e att[e] * msg[e][:]  (lanes own feature columns)
    if ((D & 3) == 0) {
        const int D4 = D >> 2;
        for (int d4 = tid; d4 < D4; d4 += SEG_BLOCK) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int e = 0; e < deg; ++e) {
                const float w = att[lo + e];
                const float4 v = seg_ld4(msg + (size_t)(lo + e) * D, d4);
                acc.x += w * v.x; acc.y += w * v.y;
                acc.z += w * v.z; acc.w += w * v.w;
            }
            seg_st4(out_row, d4, acc);
        }
    } else {
        for (int d = tid; d < D; d += SEG_BLOCK) {
            float acc = 0.f;
            for (int e = 0; e < deg; ++e)
                acc += att[lo + e] * seg_ld(msg, (size_t)(lo + e) * D + d);
            seg_st(out_row, d, acc);
        }
    }
}

// Backward of seg_attn_row for the edges e in [lo, hi) of one destination,
// given the gradient row g (D) of its output:
//   dmsg[e] = att[e] * g ;  s_e = <msg_e, g> ;
//   dgate[e] = att[e] * (s_e - sum_{e' in [lo, hi)} att[e'] s_e')
// Shared by seg_attn_bwd (segops.hip: fp32 everywhere, s_e staged in dgate
// itself, so `stage` and `dgate` may be the same buffer) and
// attn_gamma_in_bwd_gate_kernel (mlp_glue.hip: bf16 g and msg, bf16 dgate,
// fp32 stage, no dmsg).  Called by every thread of a SEG_BLOCK-thread
// workgroup; an empty segment writes nothing.  WriteDmsg=false skips the
// dmsg store and ignores `dmsg`.
template <bool WriteDmsg, typename GradT, typename MsgT, typename DmsgT,
          typename DgateT>
__device__ __forceinline__ void seg_attn_bwd_row(
        const GradT* __restrict__ g, const MsgT* __restrict__ msg,
        const float* __restrict__ att, int lo, int hi, DmsgT* dmsg,
        float* stage, DgateT* dgate, int D, float* red) {
    const int deg = hi - lo;
    if (deg == 0) return;
    const int tid = threadIdx.x;
    const int wid = tid / SEG_WAVE, lane = tid % SEG_WAVE;
    const int n_waves = SEG_BLOCK / SEG_WAVE;

    // pass 1: per-edge dmsg write + dot product (one wave per edge)
    const bool vec4 = (D & 3) == 0;
    for (int e = wid; e < deg; e += n_waves) {
        const float ae = att[lo + e];
        const MsgT* me = msg + (size_t)(lo + e) * D;
        DmsgT* dme = WriteDmsg ? dmsg + (size_t)(lo + e) * D : nullptr;
        float dot = 0.f;
        if (vec4) {
            const int D4 = D >> 2;
            for (int d4 = lane; d4 < D4; d4 += SEG_WAVE) {
                const float4 gv = seg_ld4_any(g, d4);
                const float4 mv = seg_ld4(me, d4);
                if (WriteDmsg) {
                    float4 dv;
                    dv.x = ae * gv.x; dv.y = ae * gv.y;
                    dv.z = ae * gv.z; dv.w = ae * gv.w;
                    seg_st4(dme, d4, dv);
                }
                dot += mv.x * gv.x + mv.y * gv.y + mv.z * gv.z + mv.w * gv.w;
            }
        } else {
            for (int d = lane; d < D; d += SEG_WAVE) {
                const float gv = seg_ld(g, d);
                if (WriteDmsg) seg_st(dme, d, ae * gv);
                dot += seg_ld(me, d) * gv;
            }
        }
        dot = wave_reduce_sum(dot);
        if (lane == 0) stage[lo + e] = dot;   // stage s_e
    }
    __syncthreads();

    // seg = sum_e att_e * s_e
    float part = 0.f;
    for (int e = tid; e < deg; e += SEG_BLOCK)
        part += att[lo + e] * stage[lo + e];
    const float seg = block_reduce_sum(part, red, wid, lane);

    // pass 2: dgate (overwrites the staged s_e where stage == dgate)
    for (int e = tid; e < deg; e += SEG_BLOCK)
        seg_st(dgate, lo + e, att[lo + e] * (stage[lo + e] - seg));
}
