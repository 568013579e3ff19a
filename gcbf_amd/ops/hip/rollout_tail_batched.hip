// Everything a captured rollout step does after the actor, for B scenes of
// one static layout, in TWO launches of B workgroups (CDNA4/gfx950): one
// workgroup per scene, scene b = blockIdx.x.
//
// tail_batched_step<KIND>
//   0  stage scene b's action in LDS, selecting 0.f where explore[b] != 0
//   A  unsafe_any   mask_row        (masks_common.h)        on states_in
//   -- barrier: staged action visible
//   B  env step     <env>_step_row  (env_step_common.h)     states_in -> out
//   -- barrier: this workgroup's global writes of states_out become visible
//      to this workgroup (same-workgroup RAW, as rollout_tail.hip relies on)
//   C  count        row_kth + count_row_thr (graph_build_common.h) on
//      states_out, gbase = b*N, into counts[b*n_rec + row]; with a live
//      neighbour cap (0 < topk < N) the row's threshold goes to
//      thr[b*n_rec + row]
//   -- barrier
//   F  flags[b] = {scene_edge_count, all(reach), unsafe_any}  (one lane)
//
// tail_batched_fill
//   wave 0: base_b = sum of flags[b'][0] for b' < b, total E = sum over all
//           scenes (B <= 64: one wave trip); exclusive scan of the scene's
//           row counts into LDS
//   -- barrier
//   D  fill         fill_row_thr  from base_b + offset[row] into the ONE
//      globally compacted padded edge list (all pads after all real edges,
//      which the CSR consumers' searchsorted over seg needs); the cap
//      threshold is read back from thr, not searched for again
//   -- barrier: seg reads the dst row that this workgroup's fill wrote
//   E  seg of this scene's real edges; the pad range [E, E_cap) is split
//      evenly over the B workgroups (pad_entry)
//   workgroup 0 publishes E to e_count
//
// The hand-over between the two kernels (states_out, counts, thr, flags)
// goes through global memory and stream order only.  thr is touched only
// while the cap is live; without one (topk = -1, or topk >= N) both kernels
// use FLT_MAX and the pointer may be null.  The per-wave bodies are the
// ones the stand-alone kernels call; no arithmetic is re-derived here, so
// every output is bit-equal to the kernel sequence
//   fused_masks -> env_step_batched -> build_graph_padded(batch=B, topk).
//
// Barrier discipline as in rollout_tail.hip: every __syncthreads() sits at
// the top level of the kernel body, outside every loop and branch; there is
// no return before the last one; the row loops contain no barrier.  No
// atomics, no communication between workgroups within a launch.
#include <hip/hip_runtime.h>

#include "env_step_common.h"
#include "graph_build_common.h"
#include "masks_common.h"

// per-scene bounds: the LDS bounds of rollout_tail.hip; B: one wave trip
#define TB_MAX_ROWS 128
#define TB_MAX_NODES 256
#define TB_MAX_WAVES 16
#define TB_MAX_SCENES 64
#define TB_MAX_ACT 3

template <int KIND>
__global__ void __launch_bounds__(1024) tail_batched_step(
        const float* __restrict__ states_in,  // (B, N, S) at t
        const float* __restrict__ goal,       // (B, n, G)
        const float* __restrict__ action,     // (B, n, A)
        const int* __restrict__ explore,      // (B,) != 0: action read as 0
        const float* __restrict__ K,          // LQR gain or null (dubins)
        float* states_out,                    // (B, N, S) out, re-read below
        float* __restrict__ u_ref_next, float* __restrict__ reward,
        bool* __restrict__ reach, bool* __restrict__ collision,
        int* __restrict__ counts,             // (B*n_rec,) out
        float* __restrict__ thr,              // (B*n_rec,) out, cap live only
        int* __restrict__ flags,              // (B, 3) out
        int N, int n, int n_rec, int S, int G, int A, int P, float dt,
        float r_agent, float sl, float d2g, float act_lim, float r_comm,
        int topk) {
    __shared__ float s_action[TB_MAX_NODES * TB_MAX_ACT];
    __shared__ int s_counts[TB_MAX_ROWS];
    __shared__ int s_unsafe[TB_MAX_WAVES];
    __shared__ int s_reach[TB_MAX_WAVES];

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int n_waves = blockDim.x / WAVE;
    const size_t b = blockIdx.x;

    // scene b's rows, offset once in size_t
    const float* sc_in = states_in + b * (size_t)N * S;
    float* sc_out = states_out + b * (size_t)N * S;
    const float* sc_goal = goal + b * (size_t)n * G;
    const float* sc_action = action + b * (size_t)n * A;
    float* sc_uref = u_ref_next + b * (size_t)n * A;
    float* sc_reward = reward + b * (size_t)n;
    bool* sc_reach = reach + b * (size_t)n;
    bool* sc_coll = collision + b * (size_t)n;

    // ---- 0: exploration gate (a select, never a multiply: a NaN or inf
    // action of an exploring scene must not reach the step)
    const bool zeroed = explore[b] != 0;
    for (int idx = threadIdx.x; idx < n * A; idx += blockDim.x)
        s_action[idx] = zeroed ? 0.f : sc_action[idx];

    // ---- A: unsafe mask of the CURRENT states
    bool unsafe_acc = false;
    for (int row = wave; row < n_rec; row += n_waves) {
        bool all_safe, any_uns, any_coll;
        mask_row(sc_in, row, lane, N, S, r_agent, KIND, &all_safe, &any_uns,
                 &any_coll);
        unsafe_acc |= any_uns;
    }
    __syncthreads();  // 0: gated action in LDS

    // ---- B: env step, states_in -> states_out
    bool reach_acc = true;
    const int step_rows = (KIND == ENV_CAR) ? N : n;
    for (int i = wave; i < step_rows; i += n_waves) {
        bool reach_i;
        if (KIND == ENV_DUBINS)
            reach_i = dubins_step_row(sc_in, sc_goal, s_action, sc_out,
                                      sc_uref, sc_reward, sc_reach, sc_coll,
                                      i, lane, N, n, dt, r_agent, sl, d2g,
                                      act_lim);
        else if (KIND == ENV_CAR)
            reach_i = car_step_row(sc_in, sc_goal, s_action, K, sc_out,
                                   sc_uref, sc_reward, sc_reach, sc_coll, i,
                                   lane, N, dt, r_agent, sl, d2g, act_lim);
        else
            reach_i = drone_step_row(sc_in, sc_goal, s_action, K, sc_out,
                                     sc_uref, sc_reward, sc_reach, sc_coll,
                                     i, lane, N, n, dt, r_agent, sl, d2g,
                                     act_lim);
        reach_acc &= reach_i;
    }
    if (lane == 0) {
        s_unsafe[wave] = unsafe_acc;
        s_reach[wave] = reach_acc;
    }
    __syncthreads();  // 1: states_out written, per-wave flags in LDS

    // ---- C: per-receiver edge counts on the NEW states; positions are the
    // leading P columns of states_out (row stride S), rows of scene b.  The
    // cap threshold (up to 2k sweeps of the row) is found here once and
    // handed to the fill kernel
    const int gbase = (int)b * N;
    const bool capped = topk > 0 && topk < N;
    for (int row = wave; row < n_rec; row += n_waves) {
        const float kth = row_kth(states_out, P, S, gbase, row, N,
                                  r_comm + 1.f, topk, lane);
        const int cnt = count_row_thr(states_out, P, S, gbase, row, N,
                                      r_comm, kth, lane);
        if (lane == 0) {
            s_counts[row] = cnt;
            counts[b * (size_t)n_rec + row] = cnt;
            if (capped) thr[b * (size_t)n_rec + row] = kth;
        }
    }
    __syncthreads();  // 2: counts in LDS

    // ---- F: flags (integer sum, order-free)
    if (wave == 0) {
        int part = 0;
        for (int idx = lane; idx < n_rec; idx += WAVE) part += s_counts[idx];
        const int total = wave_sum_i(part);
        if (lane == 0) {
            bool uns = false, rch = true;
            for (int w = 0; w < n_waves; ++w) {
                uns |= (s_unsafe[w] != 0);
                rch &= (s_reach[w] != 0);
            }
            flags[b * 3 + 0] = total;
            flags[b * 3 + 1] = rch ? 1 : 0;
            flags[b * 3 + 2] = uns ? 1 : 0;
        }
    }
}

__global__ void __launch_bounds__(1024) tail_batched_fill(
        const float* states_out,              // (B, N, S) new states
        const int* __restrict__ counts,       // (B*n_rec,)
        const float* __restrict__ thr,        // (B*n_rec,), cap live only
        const int* __restrict__ flags,        // (B, 3)
        long* edge_index,                     // (2, E_cap) out
        long* seg,                            // (E_cap,) out
        float* edge_attr,                     // (E_cap, A_attr) out
        int* __restrict__ e_count,            // (1,) out
        int B, int N, int n_rec, int S, int P, float r_comm, int topk,
        int attr_kind, int A_attr, long E_cap) {
    __shared__ int s_offsets[TB_MAX_ROWS];
    __shared__ int s_base;
    __shared__ int s_scene;
    __shared__ int s_total;

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int n_waves = blockDim.x / WAVE;
    const int b = blockIdx.x;

    if (wave == 0) {
        // scene bases: B <= 64, one lane per scene
        const int v = (lane < B) ? flags[lane * 3] : 0;
        const int base = wave_sum_i(lane < b ? v : 0);
        const int total = wave_sum_i(v);

        // exclusive scan of the scene's row counts, 64 rows per trip
        int carry = 0;
        for (int r0 = 0; r0 < n_rec; r0 += WAVE) {
            const int idx = r0 + lane;
            const int c = (idx < n_rec) ? counts[(size_t)b * n_rec + idx] : 0;
            int incl = c;
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const int t = __shfl_up(incl, off, WAVE);
                if (lane >= off) incl += t;
            }
            if (idx < n_rec) s_offsets[idx] = carry + incl - c;
            carry += __shfl(incl, WAVE - 1, WAVE);
        }
        if (lane == 0) {
            s_base = base;
            s_scene = carry;
            s_total = total;
        }
    }
    __syncthreads();  // 1: base, offsets and total in LDS

    // ---- D: ordered fill of this scene's edges at base_b + offset[row]
    const int base_b = s_base;
    const bool capped = topk > 0 && topk < N;
    for (int row = wave; row < n_rec; row += n_waves) {
        const float kth = capped ? thr[(size_t)b * n_rec + row] : FLT_MAX;
        fill_row_thr(states_out, S, states_out, base_b + s_offsets[row],
                     edge_index, edge_attr, E_cap, b * N, row, N, P, S,
                     A_attr, r_comm, kth, attr_kind, lane);
    }
    __syncthreads();  // 2: real edges written (seg reads their dst row)

    // ---- E: seg ids of this scene's real edges
    const long E = (long)s_total;
    const long N_total = (long)B * N;
    long real_end = (long)base_b + s_scene;
    if (real_end > E_cap) real_end = E_cap;
    for (long idx = (long)base_b + threadIdx.x; idx < real_end;
         idx += blockDim.x)
        pad_entry(idx, E, edge_index, seg, edge_attr, E_cap, N_total, A_attr);

    // pad entries [E, E_cap), an even share per workgroup
    const long pad_lo = E < E_cap ? E : E_cap;
    const long chunk = (E_cap - pad_lo + B - 1) / B;
    const long lo = pad_lo + (long)b * chunk;
    long hi = lo + chunk;
    if (hi > E_cap) hi = E_cap;
    for (long idx = lo + threadIdx.x; idx < hi; idx += blockDim.x)
        pad_entry(idx, E, edge_index, seg, edge_attr, E_cap, N_total, A_attr);

    if (b == 0 && threadIdx.x == 0) e_count[0] = (int)E;
}

extern "C" int rollout_tail_batched_max_rows() { return TB_MAX_ROWS; }
extern "C" int rollout_tail_batched_max_nodes() { return TB_MAX_NODES; }
extern "C" int rollout_tail_batched_max_scenes() { return TB_MAX_SCENES; }

// kind: ENV_CAR / ENV_DUBINS / ENV_DRONE (masks_common.h); threads: 256,
// 512 or 1024.  Both grids are B workgroups.  topk: neighbour cap, -1 none;
// thr: (B*n_rec,) workspace, needed only where 0 < topk < N.
extern "C" void launch_rollout_tail_batched(
        int kind, const float* states_in, const float* goal,
        const float* action, const int* explore, const float* K,
        float* states_out, float* u_ref_next, float* reward, bool* reach,
        bool* collision, int* counts, float* thr, long* edge_index, long* seg,
        float* edge_attr, int* flags, int* e_count, int B, int N, int n,
        int n_rec, int S, int G, int A, int P, float dt, float r_agent,
        float sl, float d2g, float act_lim, float r_comm, int attr_kind,
        int A_attr, long E_cap, int topk, int threads, hipStream_t stream) {
#define TB_LAUNCH(KIND)                                                    \
    hipLaunchKernelGGL(tail_batched_step<KIND>, dim3(B), dim3(threads), 0, \
                       stream, states_in, goal, action, explore, K,        \
                       states_out, u_ref_next, reward, reach, collision,   \
                       counts, thr, flags, N, n, n_rec, S, G, A, P, dt,    \
                       r_agent, sl, d2g, act_lim, r_comm, topk)
    if (kind == ENV_DUBINS) TB_LAUNCH(ENV_DUBINS);
    else if (kind == ENV_CAR) TB_LAUNCH(ENV_CAR);
    else TB_LAUNCH(ENV_DRONE);
#undef TB_LAUNCH
    hipLaunchKernelGGL(tail_batched_fill, dim3(B), dim3(threads), 0, stream,
                       states_out, counts, thr, flags, edge_index, seg,
                       edge_attr, e_count, B, N, n_rec, S, P, r_comm, topk,
                       attr_kind, A_attr, E_cap);
}
