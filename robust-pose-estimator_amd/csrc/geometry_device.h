// Device helpers shared by the fused geometry stage (geometry.hip) and its backward (geometry_backward.hip): K^-1, rays, depth from
// disparity, sampling positions and the bilinear taps.  One definition, so the backward's taps ARE the forward's taps.
#pragma once
#include "rpe_common.h"
#include "sampling.h"

struct Kinv3 { float m[9]; };

// 3x3 inverse by adjugate, evaluated in f64 and rounded once (torch.linalg.inv is LU in f32: ~1 ulp apart).
__device__ __forceinline__ Kinv3 invert_k(const float* K) {
    double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    double det = a * A + b * B + c * C;
    double r = 1.0 / det;
    Kinv3 o;
    o.m[0] = (float)(A * r); o.m[1] = (float)(-(b * i - c * h) * r); o.m[2] = (float)((b * f - c * e) * r);
    o.m[3] = (float)(B * r); o.m[4] = (float)((a * i - c * g) * r);  o.m[5] = (float)(-(a * f - c * d) * r);
    o.m[6] = (float)(C * r); o.m[7] = (float)(-(a * h - b * g) * r); o.m[8] = (float)((a * e - b * d) * r);
    return o;
}

// un-normalised grid_sample position of flow_utils.py:9-11 for pixel index idx displaced by flow
__device__ __forceinline__ float sample_pos(float flow, int idx, int size) {
    return rt_pos(rn_add(flow, (float)idx), size);
}

__device__ __forceinline__ float depth_from_disp(float b, float sfx, bool& valid) {
    float d = rn_div(b, -sfx);                 // pose_net.py:73
    valid = (d > 0.0f) && (d <= 1.0f);            // :74
    return valid ? d : 1.0f;                      // :75
}

// back-projected ray K^-1 [x+.5, y+.5, 1]
__device__ __forceinline__ void ray(const Kinv3& Ki, int x, int y, float& rx, float& ry, float& rz) {
    float px = (float)x + 0.5f, py = (float)y + 0.5f;
    rx = Ki.m[0] * px + Ki.m[1] * py + Ki.m[2];
    ry = Ki.m[3] * px + Ki.m[4] * py + Ki.m[5];
    rz = Ki.m[6] * px + Ki.m[7] * py + Ki.m[8];
}

struct Taps { int x0, y0; float nw, ne, sw, se; };

__device__ __forceinline__ Taps bilinear_taps(float ix, float iy) {
    Taps t;
    float fx0, fy0;
    t.x0 = safe_floor(ix, fx0); t.y0 = safe_floor(iy, fy0);
    float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    t.nw = (fx1 - ix) * (fy1 - iy);
    t.ne = (ix - fx0) * (fy1 - iy);
    t.sw = (fx1 - ix) * (iy - fy0);
    t.se = (ix - fx0) * (iy - fy0);
    return t;
}

__device__ __forceinline__ bool inb(int x, int y, int w, int h) { return x >= 0 && x < w && y >= 0 && y < h; }
