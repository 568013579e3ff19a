// Batched environment step kernels for CDNA4/gfx950: B scenes of identical
// shape per launch, each stepped exactly as env_step.hip steps one.
//
// Decomposition: as in env_step.hip one 64-lane wave per agent and four
// agents per 256-thread workgroup; the grid is (ceil(n/4), B), so a
// workgroup never straddles two scenes and the last one of each scene may
// be partial.  Every access to a scene goes through that scene's base
// pointers, offset once in size_t.  Obstacle rows are integrated
// round-robin by the scene's own agent waves.
//
// active[b] != 0: the five per-agent outputs are what the single-scene
// kernel computes for scene b alone (same device helpers from
// env_step_common.h, same order of operations; the Dubins action cost sums
// that scene's n agents).  active[b] == 0: the scene is parked — all N
// state rows are copied bit for bit, u_ref_next is the u_ref of the
// unchanged state, reward 0, collision false, reach the test at the
// current state.
//
// reach_all[b] = AND of scene b's reach row.  Positions integrate
// independently of the action, so the wave of agent 0 evaluates every
// agent's t+1 reach inside the pair scan it already does and reduces with
// a wave vote: no atomics, no cross-workgroup traffic, no second launch.
#include <hip/hip_runtime.h>

#include "env_step_common.h"

// ---------------------------------------------------------------- DubinsCar
extern "C" __global__ void dubins_step_batched(
        const float* __restrict__ states,   // (B, N, 4) at t
        const float* __restrict__ goal,     // (B, n, 4)
        const float* __restrict__ action,   // (B, n, 2) residual
        const int* __restrict__ active,     // (B,)
        float* __restrict__ new_states,     // (B, N, 4) out
        float* __restrict__ u_ref_next,     // (B, n, 2) out
        float* __restrict__ reward,         // (B, n) out
        bool* __restrict__ reach,           // (B, n) out
        bool* __restrict__ collision,       // (B, n) out
        bool* __restrict__ reach_all,       // (B,)   out
        int N, int n, float dt, float r_car, float sl, float d2g,
        float act_lim) {
    const int i = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;
    const size_t b = blockIdx.y;
    states += b * (size_t)N * 4;
    new_states += b * (size_t)N * 4;
    goal += b * (size_t)n * 4;
    action += b * (size_t)n * 2;
    u_ref_next += b * (size_t)n * 2;
    reward += b * (size_t)n;
    reach += b * (size_t)n;
    collision += b * (size_t)n;
    const bool act = active[b] != 0;
    const bool lead = i == 0;   // this wave also reduces reach_all

    const float* si = states + (size_t)i * 4;
    const float* gi = goal + (size_t)i * 4;
    const float pdx = si[0] - gi[0], pdy = si[1] - gi[1];
    const bool prev_reach = sqrtf(pdx * pdx + pdy * pdy) < d2g;

    if (!act) {
        bool all_reach = prev_reach;
        if (lead) {
            for (int j = lane; j < n; j += WAVE) {
                const float dx = states[(size_t)j * 4] - goal[(size_t)j * 4],
                            dy = states[(size_t)j * 4 + 1]
                                 - goal[(size_t)j * 4 + 1];
                all_reach &= sqrtf(dx * dx + dy * dy) < d2g;
            }
            all_reach = __all(all_reach);
        }
        if (lane == 0) {
            for (int c = 0; c < 4; ++c) new_states[i * 4 + c] = si[c];
            float urn[2];
            dubins_u_ref(si, gi, sl, urn);
            u_ref_next[i * 2 + 0] = urn[0];
            u_ref_next[i * 2 + 1] = urn[1];
            reward[i] = 0.f;
            reach[i] = prev_reach;
            collision[i] = false;
            if (lead) reach_all[b] = all_reach;
            for (int o = n + i; o < N; o += n)
                for (int c = 0; c < 4; ++c)
                    new_states[o * 4 + c] = states[o * 4 + c];
        }
        return;
    }

    // u_ref at t (bitwise-identical to the previous launch's u_ref_next)
    float ur[2];
    dubins_u_ref(si, gi, sl, ur);
    float u0 = fminf(fmaxf(action[i * 2 + 0] + ur[0], -act_lim), act_lim);
    float u1 = fminf(fmaxf(action[i * 2 + 1] + ur[1], -act_lim), act_lim);

    // dynamics (+ freeze) + Euler
    float ns[4];
    if (prev_reach) {
        ns[0] = si[0]; ns[1] = si[1]; ns[2] = si[2]; ns[3] = si[3];
    } else {
        const float vc = fminf(si[3], sl);
        ns[0] = si[0] + vc * cosf(si[2]) * dt;
        ns[1] = si[1] + vc * sinf(si[2]) * dt;
        ns[2] = si[2] + u0 * 10.f * dt;
        ns[3] = si[3] + u1 * dt;
    }
    if (lane == 0) {
        for (int c = 0; c < 4; ++c) new_states[i * 4 + c] = ns[c];
    }

    // reach at t+1
    const float ndx = ns[0] - gi[0], ndy = ns[1] - gi[1];
    const bool reach_i = sqrtf(ndx * ndx + ndy * ndy) < d2g;

    // pairwise collision at t+1 (reconstruct every j's next position); the
    // lead wave also tests every other agent's t+1 reach
    bool any_coll = false;
    bool all_reach = reach_i;
    for (int j = lane; j < N; j += WAVE) {
        if (j == i) continue;
        float pjx, pjy;
        dubins_next_pos(states + (size_t)j * 4, goal + (size_t)j * 4, j, n,
                        sl, d2g, dt, &pjx, &pjy);
        const float dx = ns[0] - pjx, dy = ns[1] - pjy;
        any_coll |= sqrtf(dx * dx + dy * dy) < 2.f * r_car;
        if (lead && j < n) {
            const float rx = pjx - goal[(size_t)j * 4],
                        ry = pjy - goal[(size_t)j * 4 + 1];
            all_reach &= sqrtf(rx * rx + ry * ry) < d2g;
        }
    }
    any_coll = __any(any_coll);
    if (lead) all_reach = __all(all_reach);

    // scalar action-norm penalty: sum over the scene's agents
    // (deterministic: each wave reduces the same full list)
    float asum = 0.f;
    for (int k = lane; k < n; k += WAVE) {
        const float a0 = action[k * 2 + 0], a1 = action[k * 2 + 1];
        asum += sqrtf(a0 * a0 + a1 * a1);
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        asum += __shfl_down(asum, off, WAVE);
    asum = __shfl(asum, 0, WAVE);

    if (lane == 0) {
        reach[i] = reach_i;
        collision[i] = any_coll;
        reward[i] = ((float)reach_i - (float)prev_reach) * 10.f
                    - (float)any_coll * 0.1f - 1e-4f - 0.01f * asum;
        // u_ref for t+1 from the new state
        float urn[2];
        dubins_u_ref(ns, gi, sl, urn);
        u_ref_next[i * 2 + 0] = urn[0];
        u_ref_next[i * 2 + 1] = urn[1];
        if (lead) reach_all[b] = all_reach;
    }

    // obstacles: integrated round-robin by agent wave i (constant drift)
    for (int o = n + i; o < N; o += n) {
        if (lane == 0) {
            const float* so = states + (size_t)o * 4;
            const float vc = fminf(so[3], sl);
            new_states[o * 4 + 0] = so[0] + vc * cosf(so[2]) * dt;
            new_states[o * 4 + 1] = so[1] + vc * sinf(so[2]) * dt;
            new_states[o * 4 + 2] = so[2];
            new_states[o * 4 + 3] = so[3];
        }
    }
}

// ---------------------------------------------------------------- SimpleCar
extern "C" __global__ void car_step_batched(
        const float* __restrict__ states,   // (B, N, 4)
        const float* __restrict__ goal,     // (B, N, 2)
        const float* __restrict__ action,   // (B, N, 2)
        const int* __restrict__ active,     // (B,)
        const float* __restrict__ K,        // (2, 4), shared by all scenes
        float* __restrict__ new_states, float* __restrict__ u_ref_next,
        float* __restrict__ reward, bool* __restrict__ reach,
        bool* __restrict__ collision, bool* __restrict__ reach_all,
        int N, float dt, float r_car, float sl, float d2g, float act_lim) {
    const int i = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= N) return;
    const size_t b = blockIdx.y;
    states += b * (size_t)N * 4;
    new_states += b * (size_t)N * 4;
    goal += b * (size_t)N * 2;
    action += b * (size_t)N * 2;
    u_ref_next += b * (size_t)N * 2;
    reward += b * (size_t)N;
    reach += b * (size_t)N;
    collision += b * (size_t)N;
    const bool act = active[b] != 0;
    const bool lead = i == 0;

    const float* si = states + (size_t)i * 4;
    const float* gi = goal + (size_t)i * 2;
    const float pdx = si[0] - gi[0], pdy = si[1] - gi[1];
    const bool prev_reach = sqrtf(pdx * pdx + pdy * pdy) < d2g;

    if (!act) {
        bool all_reach = prev_reach;
        if (lead) {
            for (int j = lane; j < N; j += WAVE) {
                const float dx = states[(size_t)j * 4] - goal[(size_t)j * 2],
                            dy = states[(size_t)j * 4 + 1]
                                 - goal[(size_t)j * 2 + 1];
                all_reach &= sqrtf(dx * dx + dy * dy) < d2g;
            }
            all_reach = __all(all_reach);
        }
        if (lane == 0) {
            for (int c = 0; c < 4; ++c) new_states[i * 4 + c] = si[c];
            float urn[2];
            car_u_ref(si, gi, K, sl, urn);
            u_ref_next[i * 2] = urn[0];
            u_ref_next[i * 2 + 1] = urn[1];
            reward[i] = 0.f;
            reach[i] = prev_reach;
            collision[i] = false;
            if (lead) reach_all[b] = all_reach;
        }
        return;
    }

    float ur[2];
    car_u_ref(si, gi, K, sl, ur);
    const float u0 = fminf(fmaxf(action[i * 2] + ur[0], -act_lim), act_lim);
    const float u1 = fminf(fmaxf(action[i * 2 + 1] + ur[1], -act_lim),
                           act_lim);

    float ns[4];
    ns[0] = si[0] + si[2] * dt;
    ns[1] = si[1] + si[3] * dt;
    ns[2] = si[2] + u0 * dt;
    ns[3] = si[3] + u1 * dt;
    if (lane == 0)
        for (int c = 0; c < 4; ++c) new_states[i * 4 + c] = ns[c];

    const float ndx = ns[0] - gi[0], ndy = ns[1] - gi[1];
    const bool reach_i = sqrtf(ndx * ndx + ndy * ndy) < d2g;

    bool any_coll = false;
    bool all_reach = reach_i;
    for (int j = lane; j < N; j += WAVE) {
        if (j == i) continue;
        const float* sj = states + (size_t)j * 4;
        const float pjx = sj[0] + sj[2] * dt, pjy = sj[1] + sj[3] * dt;
        const float dx = ns[0] - pjx, dy = ns[1] - pjy;
        any_coll |= sqrtf(dx * dx + dy * dy) < 2.f * r_car;
        if (lead) {
            const float rx = pjx - goal[(size_t)j * 2],
                        ry = pjy - goal[(size_t)j * 2 + 1];
            all_reach &= sqrtf(rx * rx + ry * ry) < d2g;
        }
    }
    any_coll = __any(any_coll);
    if (lead) all_reach = __all(all_reach);

    if (lane == 0) {
        const float a0 = action[i * 2], a1 = action[i * 2 + 1];
        reach[i] = reach_i;
        collision[i] = any_coll;
        reward[i] = ((float)reach_i - (float)prev_reach) * 4.f
                    - (float)any_coll * 2.f - 0.01f
                    - 1e-4f * sqrtf(a0 * a0 + a1 * a1);
        float urn[2];
        car_u_ref(ns, gi, K, sl, urn);
        u_ref_next[i * 2] = urn[0];
        u_ref_next[i * 2 + 1] = urn[1];
        if (lead) reach_all[b] = all_reach;
    }
}

// --------------------------------------------------------------- SimpleDrone
extern "C" __global__ void drone_step_batched(
        const float* __restrict__ states,   // (B, N, 6)
        const float* __restrict__ goal,     // (B, n, 6)
        const float* __restrict__ action,   // (B, n, 3)
        const int* __restrict__ active,     // (B,)
        const float* __restrict__ K,        // (3, 6), shared by all scenes
        float* __restrict__ new_states, float* __restrict__ u_ref_next,
        float* __restrict__ reward, bool* __restrict__ reach,
        bool* __restrict__ collision, bool* __restrict__ reach_all,
        int N, int n, float dt, float r_drone, float sl, float d2g,
        float act_lim) {
    const int i = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;
    const size_t b = blockIdx.y;
    states += b * (size_t)N * 6;
    new_states += b * (size_t)N * 6;
    goal += b * (size_t)n * 6;
    action += b * (size_t)n * 3;
    u_ref_next += b * (size_t)n * 3;
    reward += b * (size_t)n;
    reach += b * (size_t)n;
    collision += b * (size_t)n;
    const bool act = active[b] != 0;
    const bool lead = i == 0;

    const float* si = states + (size_t)i * 6;
    const float* gi = goal + (size_t)i * 6;
    const float pdx = si[0] - gi[0], pdy = si[1] - gi[1],
                pdz = si[2] - gi[2];
    const bool prev_reach = sqrtf(pdx * pdx + pdy * pdy + pdz * pdz) < d2g;

    if (!act) {
        bool all_reach = prev_reach;
        if (lead) {
            for (int j = lane; j < n; j += WAVE) {
                const float* sj = states + (size_t)j * 6;
                const float* gj = goal + (size_t)j * 6;
                const float dx = sj[0] - gj[0], dy = sj[1] - gj[1],
                            dz = sj[2] - gj[2];
                all_reach &= sqrtf(dx * dx + dy * dy + dz * dz) < d2g;
            }
            all_reach = __all(all_reach);
        }
        if (lane == 0) {
            for (int c = 0; c < 6; ++c) new_states[i * 6 + c] = si[c];
            float urn[3];
            drone_u_ref(si, gi, K, sl, urn);
#pragma unroll
            for (int c = 0; c < 3; ++c) u_ref_next[i * 3 + c] = urn[c];
            reward[i] = 0.f;
            reach[i] = prev_reach;
            collision[i] = false;
            if (lead) reach_all[b] = all_reach;
            for (int o = n + i; o < N; o += n)
                for (int c = 0; c < 6; ++c)
                    new_states[o * 6 + c] = states[o * 6 + c];
        }
        return;
    }

    float ur[3];
    drone_u_ref(si, gi, K, sl, ur);
    float u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        u[c] = fminf(fmaxf(action[i * 3 + c] + ur[c], -act_lim), act_lim);

    float ns[6];
    if (prev_reach) {
#pragma unroll
        for (int c = 0; c < 6; ++c) ns[c] = si[c];
    } else {
        // xdot = A x + B u
        ns[0] = si[0] + si[3] * dt;
        ns[1] = si[1] + si[4] * dt;
        ns[2] = si[2] + si[5] * dt;
        ns[3] = si[3] + (-1.1f * si[3] + 1.1f * u[0]) * dt;
        ns[4] = si[4] + (-1.1f * si[4] + 1.1f * u[1]) * dt;
        ns[5] = si[5] + (-6.0f * si[5] + 6.0f * u[2]) * dt;
    }
    if (lane == 0)
        for (int c = 0; c < 6; ++c) new_states[i * 6 + c] = ns[c];

    const float ndx = ns[0] - gi[0], ndy = ns[1] - gi[1],
                ndz = ns[2] - gi[2];
    const bool reach_i = sqrtf(ndx * ndx + ndy * ndy + ndz * ndz) < d2g;

    bool any_coll = false;
    bool all_reach = reach_i;
    for (int j = lane; j < N; j += WAVE) {
        if (j == i) continue;
        const float* sj = states + (size_t)j * 6;
        float pjx = sj[0], pjy = sj[1], pjz = sj[2];
        if (j < n) {
            const float* gj = goal + (size_t)j * 6;
            const float dx = sj[0] - gj[0], dy = sj[1] - gj[1],
                        dz = sj[2] - gj[2];
            if (sqrtf(dx * dx + dy * dy + dz * dz) >= d2g) {
                pjx += sj[3] * dt;
                pjy += sj[4] * dt;
                pjz += sj[5] * dt;
            }
            if (lead) {
                const float rx = pjx - gj[0], ry = pjy - gj[1],
                            rz = pjz - gj[2];
                all_reach &= sqrtf(rx * rx + ry * ry + rz * rz) < d2g;
            }
        }  // obstacles static
        const float dx = ns[0] - pjx, dy = ns[1] - pjy, dz = ns[2] - pjz;
        any_coll |= sqrtf(dx * dx + dy * dy + dz * dz) < 2.f * r_drone;
    }
    any_coll = __any(any_coll);
    if (lead) all_reach = __all(all_reach);

    if (lane == 0) {
        const float a0 = action[i * 3], a1 = action[i * 3 + 1],
                    a2 = action[i * 3 + 2];
        reach[i] = reach_i;
        collision[i] = any_coll;
        reward[i] = ((float)reach_i - (float)prev_reach) * 10.f
                    - (float)any_coll - 0.01f
                    - 1e-3f * sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
        float urn[3];
        drone_u_ref(ns, gi, K, sl, urn);
#pragma unroll
        for (int c = 0; c < 3; ++c) u_ref_next[i * 3 + c] = urn[c];
        if (lead) reach_all[b] = all_reach;
    }

    // obstacles are static: copy rows round-robin
    for (int o = n + i; o < N; o += n) {
        if (lane == 0)
            for (int c = 0; c < 6; ++c)
                new_states[o * 6 + c] = states[o * 6 + c];
    }
}

// ------------------------------------------------------------- launchers
static inline dim3 scene_grid(int n, int B) {
    return dim3((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, B);
}

extern "C" void launch_dubins_step_batched(
        const float* states, const float* goal, const float* action,
        const int* active, float* new_states, float* u_ref_next,
        float* reward, bool* reach, bool* collision, bool* reach_all, int B,
        int N, int n, float dt, float r, float sl, float d2g, float act_lim,
        hipStream_t stream) {
    hipLaunchKernelGGL(dubins_step_batched, scene_grid(n, B),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream, states, goal,
                       action, active, new_states, u_ref_next, reward, reach,
                       collision, reach_all, N, n, dt, r, sl, d2g, act_lim);
}

extern "C" void launch_car_step_batched(
        const float* states, const float* goal, const float* action,
        const int* active, const float* K, float* new_states,
        float* u_ref_next, float* reward, bool* reach, bool* collision,
        bool* reach_all, int B, int N, float dt, float r, float sl,
        float d2g, float act_lim, hipStream_t stream) {
    hipLaunchKernelGGL(car_step_batched, scene_grid(N, B),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream, states, goal,
                       action, active, K, new_states, u_ref_next, reward,
                       reach, collision, reach_all, N, dt, r, sl, d2g,
                       act_lim);
}

extern "C" void launch_drone_step_batched(
        const float* states, const float* goal, const float* action,
        const int* active, const float* K, float* new_states,
        float* u_ref_next, float* reward, bool* reach, bool* collision,
        bool* reach_all, int B, int N, int n, float dt, float r, float sl,
        float d2g, float act_lim, hipStream_t stream) {
    hipLaunchKernelGGL(drone_step_batched, scene_grid(n, B),
                       dim3(ROWS_PER_BLOCK * WAVE), 0, stream, states, goal,
                       action, active, K, new_states, u_ref_next, reward,
                       reach, collision, reach_all, N, n, dt, r, sl, d2g,
                       act_lim);
}
