// Everything a captured rollout step does after the actor, in ONE launch of
// ONE workgroup (CDNA4/gfx950):
//
//   A  unsafe_any   mask_row        (masks_common.h)        on states_in
//   B  env step     <env>_step_row  (env_step_common.h)     states_in -> out
//   -- barrier: this workgroup's global writes of states_out become visible
//      to this workgroup (same-workgroup RAW, as segops.hip relies on)
//   C  count        count_row       (graph_build_common.h)  on states_out
//   -- barrier -- exclusive scan of the per-row counts in LDS (wave 0)
//   -- barrier
//   D  fill         fill_row                                on states_out
//   -- barrier: pad reads the dst row that fill wrote
//   E  pad          pad_entry
//   F  flags = [edge_count, all(reach), unsafe_any]   (one lane, plain stores)
//
// At rollout sizes (16 agents, a 16x16 pair scan, <= 240 edges) each of
// these was a launch of its own whose work did not fill its dispatch slot.
// The per-wave bodies are the ones the stand-alone kernels call: where
// those map "one wave per row" over a grid, this kernel loops
// ``for (row = wave; row < rows; row += n_waves)``.  No arithmetic is
// re-derived here, so every output is bit-equal to the kernel sequence.
// ``topk`` is the neighbour cap count_row / fill_row take (k nearest senders
// per receiver, ties kept; -1: none); the cap's k-th-distance scan lives in
// registers, so the LDS bound below does not depend on it.
//
// Barrier discipline: every __syncthreads() sits at the top level of the
// kernel body, outside every loop and branch; there is no return before the
// last one; the row loops contain no barrier.  No atomics, no
// cross-workgroup communication.
#include <hip/hip_runtime.h>

#include "env_step_common.h"
#include "graph_build_common.h"
#include "masks_common.h"

// size bound of the single-workgroup path (docs/KERNELS.md, rollout_tail)
#define TAIL_MAX_ROWS 128
#define TAIL_MAX_NODES 256
#define TAIL_MAX_WAVES 16

template <int KIND>
__global__ void __launch_bounds__(1024) rollout_tail_kernel(
        const float* __restrict__ states_in,  // (N, S) at t
        const float* __restrict__ goal,
        const float* __restrict__ action,     // (n, A)
        const float* __restrict__ K,          // LQR gain or null (dubins)
        float* states_out,                    // (N, S) out, re-read below
        float* __restrict__ u_ref_next, float* __restrict__ reward,
        bool* __restrict__ reach, bool* __restrict__ collision,
        long* edge_index,                     // (2, E_max) out
        long* seg,                            // (E_max,) out
        float* edge_attr,                     // (E_max, A_attr) out
        int* __restrict__ flags,              // (3,) out
        int N, int n, int n_rec, int S, int P, float dt, float r_agent,
        float sl, float d2g, float act_lim, float r_comm, int attr_kind,
        int A_attr, long E_max, int topk) {
    __shared__ int s_counts[TAIL_MAX_ROWS];
    __shared__ int s_offsets[TAIL_MAX_ROWS];
    __shared__ int s_unsafe[TAIL_MAX_WAVES];
    __shared__ int s_reach[TAIL_MAX_WAVES];
    __shared__ int s_total;

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int n_waves = blockDim.x / WAVE;

    // ---- A: unsafe mask of the CURRENT states
    bool unsafe_acc = false;
    for (int row = wave; row < n_rec; row += n_waves) {
        bool all_safe, any_uns, any_coll;
        mask_row(states_in, row, lane, N, S, r_agent, KIND, &all_safe,
                 &any_uns, &any_coll);
        unsafe_acc |= any_uns;
    }

    // ---- B: env step, states_in -> states_out
    bool reach_acc = true;
    const int step_rows = (KIND == ENV_CAR) ? N : n;
    for (int i = wave; i < step_rows; i += n_waves) {
        bool reach_i;
        if (KIND == ENV_DUBINS)
            reach_i = dubins_step_row(states_in, goal, action, states_out,
                                      u_ref_next, reward, reach, collision,
                                      i, lane, N, n, dt, r_agent, sl, d2g,
                                      act_lim);
        else if (KIND == ENV_CAR)
            reach_i = car_step_row(states_in, goal, action, K, states_out,
                                   u_ref_next, reward, reach, collision, i,
                                   lane, N, dt, r_agent, sl, d2g, act_lim);
        else
            reach_i = drone_step_row(states_in, goal, action, K, states_out,
                                     u_ref_next, reward, reach, collision,
                                     i, lane, N, n, dt, r_agent, sl, d2g,
                                     act_lim);
        reach_acc &= reach_i;
    }
    if (lane == 0) {
        s_unsafe[wave] = unsafe_acc;
        s_reach[wave] = reach_acc;
    }
    __syncthreads();  // 1: states_out written, per-wave flags in LDS

    // ---- C: per-receiver edge counts on the NEW states; positions are
    // the leading P columns of states_out (row stride S)
    for (int row = wave; row < n_rec; row += n_waves) {
        const int cnt = count_row(states_out, P, S, 0, row, N, r_comm, topk,
                                  lane);
        if (lane == 0) s_counts[row] = cnt;
    }
    __syncthreads();  // 2: counts in LDS

    // exclusive scan by wave 0, 64 rows per trip (integer, order-free)
    if (wave == 0) {
        int carry = 0;
        for (int base = 0; base < n_rec; base += WAVE) {
            const int idx = base + lane;
            const int v = (idx < n_rec) ? s_counts[idx] : 0;
            int incl = v;
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const int t = __shfl_up(incl, off, WAVE);
                if (lane >= off) incl += t;
            }
            if (idx < n_rec) s_offsets[idx] = carry + incl - v;
            carry += __shfl(incl, WAVE - 1, WAVE);
        }
        if (lane == 0) s_total = carry;
    }
    __syncthreads();  // 3: offsets and total in LDS

    // ---- D: ordered fill of edge_index / edge_attr
    for (int row = wave; row < n_rec; row += n_waves)
        fill_row(states_out, S, states_out, s_offsets[row], edge_index,
                 edge_attr, E_max, 0, row, N, P, S, A_attr, r_comm, topk,
                 attr_kind, lane);
    __syncthreads();  // 4: real edges written (pad reads their dst row)

    // ---- E: seg ids of the real edges, pad entries up to E_max
    const long E = (long)s_total;
    for (long idx = threadIdx.x; idx < E_max; idx += blockDim.x)
        pad_entry(idx, E, edge_index, seg, edge_attr, E_max, (long)N, A_attr);

    // ---- F: flags
    if (threadIdx.x == 0) {
        bool uns = false, rch = true;
        for (int w = 0; w < n_waves; ++w) {
            uns |= (s_unsafe[w] != 0);
            rch &= (s_reach[w] != 0);
        }
        flags[0] = (int)E;
        flags[1] = rch ? 1 : 0;
        flags[2] = uns ? 1 : 0;
    }
}

extern "C" int rollout_tail_max_rows() { return TAIL_MAX_ROWS; }
extern "C" int rollout_tail_max_nodes() { return TAIL_MAX_NODES; }

// kind: ENV_CAR / ENV_DUBINS / ENV_DRONE (masks_common.h); topk: neighbour
// cap of graph_build_common.h (-1: none); threads: 256, 512 or 1024.  Grid
// is always one workgroup.
extern "C" void launch_rollout_tail(
        int kind, const float* states_in, const float* goal,
        const float* action, const float* K, float* states_out,
        float* u_ref_next, float* reward, bool* reach, bool* collision,
        long* edge_index, long* seg, float* edge_attr, int* flags, int N,
        int n, int n_rec, int S, int P, float dt, float r_agent, float sl,
        float d2g, float act_lim, float r_comm, int attr_kind, int A_attr,
        long E_max, int topk, int threads, hipStream_t stream) {
#define TAIL_LAUNCH(KIND)                                                  \
    hipLaunchKernelGGL(rollout_tail_kernel<KIND>, dim3(1), dim3(threads),  \
                       0, stream, states_in, goal, action, K, states_out,  \
                       u_ref_next, reward, reach, collision, edge_index,   \
                       seg, edge_attr, flags, N, n, n_rec, S, P, dt,       \
                       r_agent, sl, d2g, act_lim, r_comm, attr_kind,       \
                       A_attr, E_max, topk)
    if (kind == ENV_DUBINS) TAIL_LAUNCH(ENV_DUBINS);
    else if (kind == ENV_CAR) TAIL_LAUNCH(ENV_CAR);
    else TAIL_LAUNCH(ENV_DRONE);
#undef TAIL_LAUNCH
}
