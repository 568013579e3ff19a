// Per-env device helpers shared by env_step.hip (one scene per launch) and
// env_step_batched.hip (B scenes per launch): reference controllers and the
// t+1 position reconstruction.  Both kernel families call these, in the same
// order, so they cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#define WAVE 64
#define ROWS_PER_BLOCK 4

#define PI_F 3.14159265358979323846f
#define TWO_PI_F 6.28318530717958647692f

__device__ __forceinline__ float pmod2pi(float x) {
    // python-style modulo: result in [0, 2*pi)
    float r = fmodf(x, TWO_PI_F);
    if (r < 0.f) r += TWO_PI_F;
    return r;
}

__device__ __forceinline__ float signf(float x) {
    return (x > 0.f) - (x < 0.f);
}

// ---------------------------------------------------------------- DubinsCar
// states [x, y, th, v]; action [omega/10, a]; obstacles move at constant
// heading/speed.  PID reference controller (reference dubins_car.py:764-816).
__device__ inline void dubins_u_ref(const float* s, const float* g, float sl,
                                    float* out) {
    const float dx = s[0] - g[0], dy = s[1] - g[1];
    const float dist = sqrtf(dx * dx + dy * dy);
    const float k_omega = 0.2f, k_v = 0.3f, k_a = 0.6f;

    float arg = -dx / (dist + 1e-4f);
    arg = fminf(fmaxf(arg, -1.f), 1.f);
    const float theta_t = pmod2pi(acosf(arg) * signf(-dy));
    const float theta = pmod2pi(s[2]);
    const float td = theta_t - theta;
    const float c = cosf(theta), sn = sinf(theta);
    float inner = (-dx) * c + (-dy) * sn;
    inner = fminf(fmaxf(inner / (dist + 1e-4f), -1.f), 1.f);
    const float tb = acosf(inner);

    const bool anti = (td < PI_F) && (td >= 0.f);
    const bool clock = (td > -PI_F) && (td <= 0.f);
    const float sgn = (theta <= PI_F) ? (anti ? 1.f : -1.f)
                                      : (clock ? -1.f : 1.f);
    out[0] = fminf(fmaxf(sgn * k_omega * tb, -5.f), 5.f);

    float a = -k_a * s[3] + k_v * dist;
    if (s[3] > sl) a = fminf(a, 0.f);
    if (s[3] < -sl) a = fmaxf(a, 0.f);
    out[1] = a;
}

// t+1 position of node j (agents freeze on reach; obstacles drift)
__device__ inline void dubins_next_pos(const float* s, const float* goal,
                                       int j, int n, float sl, float d2g,
                                       float dt, float* px, float* py) {
    float x = s[0], y = s[1];
    bool frozen = false;
    if (j < n) {
        const float gx = goal[0], gy = goal[1];
        const float dx = x - gx, dy = y - gy;
        frozen = sqrtf(dx * dx + dy * dy) < d2g;
    }
    if (!frozen) {
        const float vc = fminf(s[3], sl);
        x += vc * cosf(s[2]) * dt;
        y += vc * sinf(s[2]) * dt;
    }
    *px = x;
    *py = y;
}

// ---------------------------------------------------------------- SimpleCar
// states [x, y, vx, vy]; action [ax, ay]; LQR u_ref = -K (x - goal) with an
// over-speed penalty (reference simple_car.py:270-304).  No obstacles.
__device__ inline void car_u_ref(const float* s, const float* g2,
                                 const float* K,  // (2, 4) row-major
                                 float sl, float* out) {
    float d[4] = {s[0] - g2[0], s[1] - g2[1], s[2], s[3]};
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        a0 -= K[c] * d[c];
        a1 -= K[4 + c] * d[c];
    }
    const float v = sqrtf(s[2] * s[2] + s[3] * s[3]);
    if (v - sl > 0.f) {
        const float scale = (v - sl) * 50.f / v;
        a0 -= scale * s[2];
        a1 -= scale * s[3];
    }
    out[0] = a0;
    out[1] = a1;
}

// --------------------------------------------------------------- SimpleDrone
// states [x,y,z,vx,vy,vz]; xdot = A x + B u with diagonal damping
// (A: pos<-vel identity, vel damping -1.1/-1.1/-6; B: 1.1/1.1/6);
// LQR u_ref with over-speed penalty *10 (reference simple_drone.py:85-120,
// 349-377).  Obstacles static; agents freeze on reach.
__device__ inline void drone_u_ref(const float* s, const float* g,
                                   const float* K,  // (3, 6) row-major
                                   float sl, float* out) {
    float d[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = s[c] - g[c];
    float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int c = 0; c < 6; ++c) a[u] -= K[u * 6 + c] * d[c];
    const float v = sqrtf(s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
    if (v - sl > 0.f) {
        const float scale = (v - sl) * 10.f / v;
        a[0] -= scale * s[3];
        a[1] -= scale * s[4];
        a[2] -= scale * s[5];
    }
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2];
}
