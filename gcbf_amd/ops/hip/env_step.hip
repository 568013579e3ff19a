// Fused single-graph environment step kernels for CDNA4/gfx950.
//
// One launch per env.step() replaces the reference's ~40 small ATen calls
// (u_ref PID/LQR, action clamp, dynamics, Euler, reach/collision tests,
// reward assembly — reference gcbf/env/dubins_car.py:522-615,
// simple_car.py:146-176, simple_drone.py:191-234).  It also emits the NEXT
// step's u_ref (the trainer attaches u_ref to the new graph immediately, so
// fusing it here makes that attach free).
//
// Key structural fact exploited: in all three envs the position update is
// action-independent (positions integrate the CURRENT velocity/heading), so
// each agent-wave can reconstruct every neighbor's t+1 position on the fly
// for the pairwise collision test — the whole step is one kernel.
//
// Decomposition: one 64-lane wave per agent; obstacles are integrated
// round-robin by the waves after their agent work.
#include <hip/hip_runtime.h>
#include <cfloat>

#include "env_step_common.h"

// ---------------------------------------------------------------- DubinsCar
// per-env device helpers (u_ref, t+1 positions): env_step_common.h
extern "C" __global__ void dubins_step(
        const float* __restrict__ states,   // (N, 4) at t
        const float* __restrict__ goal,     // (n, 4)
        const float* __restrict__ action,   // (n, 2) residual
        float* __restrict__ new_states,     // (N, 4) out
        float* __restrict__ u_ref_next,     // (n, 2) out (for t+1 graph)
        float* __restrict__ reward,         // (n,)  out
        bool* __restrict__ reach,           // (n,)  out (at t+1)
        bool* __restrict__ collision,       // (n,)  out (at t+1)
        int N, int n, float dt, float r_car, float sl, float d2g,
        float act_lim) {
    const int i = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;

    dubins_step_row(states, goal, action, new_states, u_ref_next, reward,
                    reach, collision, i, lane, N, n, dt, r_car, sl, d2g,
                    act_lim);
}

// ---------------------------------------------------------------- SimpleCar
extern "C" __global__ void car_step(
        const float* __restrict__ states,   // (N, 4)
        const float* __restrict__ goal,     // (N, 2)
        const float* __restrict__ action,   // (N, 2)
        const float* __restrict__ K,        // (2, 4)
        float* __restrict__ new_states, float* __restrict__ u_ref_next,
        float* __restrict__ reward, bool* __restrict__ reach,
        bool* __restrict__ collision,
        int N, float dt, float r_car, float sl, float d2g, float act_lim) {
    const int i = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= N) return;

    car_step_row(states, goal, action, K, new_states, u_ref_next, reward,
                 reach, collision, i, lane, N, dt, r_car, sl, d2g, act_lim);
}

// --------------------------------------------------------------- SimpleDrone
extern "C" __global__ void drone_step(
        const float* __restrict__ states,   // (N, 6)
        const float* __restrict__ goal,     // (n, 6)
        const float* __restrict__ action,   // (n, 3)
        const float* __restrict__ K,        // (3, 6)
        float* __restrict__ new_states, float* __restrict__ u_ref_next,
        float* __restrict__ reward, bool* __restrict__ reach,
        bool* __restrict__ collision,
        int N, int n, float dt, float r_drone, float sl, float d2g,
        float act_lim) {
    const int i = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;

    drone_step_row(states, goal, action, K, new_states, u_ref_next, reward,
                   reach, collision, i, lane, N, n, dt, r_drone, sl, d2g,
                   act_lim);
}

// ------------------------------------------------------------- launchers
extern "C" void launch_dubins_step(const float* states, const float* goal,
                                   const float* action, float* new_states,
                                   float* u_ref_next, float* reward,
                                   bool* reach, bool* collision, int N, int n,
                                   float dt, float r, float sl, float d2g,
                                   float act_lim, hipStream_t stream) {
    const int blocks = (n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(dubins_step, dim3(blocks),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream, states, goal,
                       action, new_states, u_ref_next, reward, reach,
                       collision, N, n, dt, r, sl, d2g, act_lim);
}

extern "C" void launch_car_step(const float* states, const float* goal,
                                const float* action, const float* K,
                                float* new_states, float* u_ref_next,
                                float* reward, bool* reach, bool* collision,
                                int N, float dt, float r, float sl, float d2g,
                                float act_lim, hipStream_t stream) {
    const int blocks = (N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(car_step, dim3(blocks), dim3(ROWS_PER_BLOCK * WAVE),
                       0, stream, states, goal, action, K, new_states,
                       u_ref_next, reward, reach, collision, N, dt, r, sl,
                       d2g, act_lim);
}

extern "C" void launch_drone_step(const float* states, const float* goal,
                                  const float* action, const float* K,
                                  float* new_states, float* u_ref_next,
                                  float* reward, bool* reach,
                                  bool* collision, int N, int n, float dt,
                                  float r, float sl, float d2g,
                                  float act_lim, hipStream_t stream) {
    const int blocks = (n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(drone_step, dim3(blocks), dim3(ROWS_PER_BLOCK * WAVE),
                       0, stream, states, goal, action, K, new_states,
                       u_ref_next, reward, reach, collision, N, n, dt, r, sl,
                       d2g, act_lim);
}
