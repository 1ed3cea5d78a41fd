// Host-side arithmetic of the TinyUNet training route (csrc/unet_train.hip): map sizes, the order and offsets of the parameter
// tensors in the gradient blob, and the workspace plan.  Plain C++ (no HIP), so a stand-alone host program can exercise it.
//
// Parameter order (UT_NPARAM = 36 tensors, torch's own layouts; rpe_unet_train_forward takes the pointers in this order and
// rpe_unet_train_backward writes the gradients back to back in it), widths 16/32/64:
//   encoder stage i = 0..2 (cin_i -> c_i), index 6 i + :  0 conv1.weight (c_i,cin_i,3,3) | 1 conv1.bias | 2 norm.weight | 3 norm.bias |
//                                                         4 conv2.weight (c_i,c_i,3,3) | 5 conv2.bias
//   decoder stage j = 0..1 (c -> c/2), index 18 + 8 j + : 0 upconv.weight (c,c/2,2,2) | 1 upconv.bias | 2 conv1.weight (c/2,c,3,3) |
//                                                         3 conv1.bias | 4 norm.weight | 5 norm.bias | 6 conv2.weight (c/2,c/2,3,3) | 7 conv2.bias
//   head, index 34 + :                                    0 weight (1,16,1,1) | 1 bias
// Norm order (UT_NNORM = 5): the encoder stages' norms, then the decoder stages'.
#pragma once
#include <stddef.h>

#define UT_NPARAM 36
#define UT_NNORM 5

static const int UT_WIDTHS[3] = {16, 32, 64};

struct UtGeo { int h[3], w[3], hs[3], ws[3]; int uh[2], uw[2], dh[2], dw[2]; };   // encoder conv1 / conv2 (skip) sizes; decoder sizes

// false below the 44x44 grid the valid convolutions need (the same walk as the inference chain's)
static inline bool ut_geo(int h8, int w8, UtGeo& g) {
    int h = h8, w = w8;
    for (int i = 0; i < 3; ++i) {
        g.h[i] = h - 2; g.w[i] = w - 2; g.hs[i] = h - 4; g.ws[i] = w - 4;
        if (g.hs[i] < 2 || g.ws[i] < 2) return false;
        h = g.hs[i] / 2; w = g.ws[i] / 2;
    }
    int ch = g.hs[2], cw = g.ws[2];
    for (int j = 0; j < 2; ++j) {
        g.uh[j] = 2 * ch; g.uw[j] = 2 * cw;
        if (g.uh[j] > g.hs[1 - j] || g.uw[j] > g.ws[1 - j]) return false;
        g.dh[j] = g.uh[j] - 4; g.dw[j] = g.uw[j] - 4;
        if (g.dh[j] < 1 || g.dw[j] < 1) return false;
        ch = g.dh[j]; cw = g.dw[j];
    }
    return true;
}

// floats of parameter tensor k of a TinyUNet(cin); 0 for an index outside [0, UT_NPARAM)
static inline size_t ut_param_floats(int cin, int k) {
    if (k < 0 || k >= UT_NPARAM) return 0;
    if (k < 18) {
        const int i = k / 6, c = UT_WIDTHS[i], ci = i ? UT_WIDTHS[i - 1] : cin;
        switch (k % 6) { case 0: return (size_t)c * ci * 9; case 4: return (size_t)c * c * 9; default: return (size_t)c; }
    }
    if (k < 34) {
        const int j = (k - 18) / 8, c = UT_WIDTHS[2 - j], c2 = c / 2;
        switch ((k - 18) % 8) { case 0: return (size_t)c * c2 * 4; case 2: return (size_t)c2 * c * 9; case 6: return (size_t)c2 * c2 * 9; default: return (size_t)c2; }
    }
    return k == 34 ? 16 : 1;
}

// first float of tensor k in the gradient blob; k = UT_NPARAM gives the blob's size
static inline size_t ut_grad_offset(int cin, int k) {
    size_t n = 0;
    for (int q = 0; q < k && q < UT_NPARAM; ++q) n += ut_param_floats(cin, q);
    return n;
}

// Workspace plan: offsets in floats from the 256-byte-aligned base; every buffer starts on a multiple of 64 floats.
// Saved by the forward: a1 / r1 (encoder conv1 output and its norm + ReLU), skip (conv2), pool; up, r (conv1 + ReLU), nrm, dout of
// the decoder; mean / invstd of the five norms; the head map.  The rest is the backward's: one gradient buffer per activation and the
// weight-gradient partials (doubles).
struct UtPlan {
    size_t a1[3], r1[3], skip[3], pool[2], up[2], r[2], nrm[2], dout[2], mean[UT_NNORM], invstd[UT_NNORM], hm;
    size_t g_r1[3], g_skip[3], g_pool[2], g_up[2], g_nrm[2], g_dout[2], g_hm, wpart;
    size_t total;
};

#define UT_WCHUNK_MIN 4096          // pixels (batch x map) per weight-gradient partial, at least
#define UT_WCHUNK_MAX_N 32          // partials per weight, at most

static inline void ut_wchunks(long long pixels, int& chunk, int& nchunk) {
    long long c = (pixels + UT_WCHUNK_MAX_N - 1) / UT_WCHUNK_MAX_N;
    if (c < UT_WCHUNK_MIN) c = UT_WCHUNK_MIN;
    c = (c + 255) / 256 * 256;
    chunk = (int)c; nchunk = (int)((pixels + c - 1) / c);
}

static inline void ut_plan(const UtGeo& g, int n, int cin, UtPlan& p) {
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += (floats + 63) / 64 * 64; return o; };
    for (int i = 0; i < 3; ++i) {
        const size_t c = UT_WIDTHS[i];
        p.a1[i] = take(n * c * g.h[i] * g.w[i]); p.r1[i] = take(n * c * g.h[i] * g.w[i]); p.g_r1[i] = take(n * c * g.h[i] * g.w[i]);
        p.skip[i] = take(n * c * g.hs[i] * g.ws[i]); p.g_skip[i] = take(n * c * g.hs[i] * g.ws[i]);
        if (i < 2) { p.pool[i] = take(n * c * (g.hs[i] / 2) * (g.ws[i] / 2)); p.g_pool[i] = take(n * c * (g.hs[i] / 2) * (g.ws[i] / 2)); }
        p.mean[i] = take(c); p.invstd[i] = take(c);
    }
    for (int j = 0; j < 2; ++j) {
        const size_t c2 = UT_WIDTHS[2 - j] / 2, mid = (size_t)(g.dh[j] + 2) * (g.dw[j] + 2);
        p.up[j] = take(n * c2 * g.uh[j] * g.uw[j]); p.g_up[j] = take(n * c2 * g.uh[j] * g.uw[j]);
        p.r[j] = take(n * c2 * mid); p.nrm[j] = take(n * c2 * mid); p.g_nrm[j] = take(n * c2 * mid);
        p.dout[j] = take(n * c2 * g.dh[j] * g.dw[j]); p.g_dout[j] = take(n * c2 * g.dh[j] * g.dw[j]);
        p.mean[3 + j] = take(c2); p.invstd[3 + j] = take(c2);
    }
    p.hm = take((size_t)n * g.dh[1] * g.dw[1]); p.g_hm = take((size_t)n * g.dh[1] * g.dw[1]);
    // weight-gradient partials (doubles), shared by the layers one after the other: room for the largest weight at the most partials
    size_t wmax = 0;
    for (int k = 0; k < UT_NPARAM; ++k) { const size_t f = ut_param_floats(cin, k); wmax = f > wmax ? f : wmax; }
    p.wpart = take(2 * wmax * UT_WCHUNK_MAX_N);
    p.total = at;
}

// The plan's buffers by index, in the order ut_plan lays them out (so the offsets grow with the index), UT_NBUF in all:
//   encoder stage i = 0..2, from index 0 / 9 / 18:  a1 | r1 | g_r1 | skip | g_skip | pool | g_pool (stages 0 and 1 only) | mean | invstd
//   decoder stage j = 0..1, from index 25 + 9 j:    up | g_up | r | nrm | g_nrm | dout | g_dout | mean (norm 3 + j) | invstd
//   43 hm | 44 g_hm | 45 wpart
// c, h, w: the extent of one batch row of the buffer (n rows each); mean / invstd are (c) vectors (rows = 1, h = w = 1), and wpart is
// UT_WCHUNK_MAX_N rows of DOUBLES, one per entry of the largest weight tensor (c), so it spans 2 rows c floats.
#define UT_NBUF 46

struct UtBuf { size_t off; int rows, c, h, w; };

static inline bool ut_plan_buffer(const UtGeo& g, const UtPlan& p, int n, int cin, int index, UtBuf& b) {
    int k = 0;
    auto hit = [&](size_t off, int rows, int c, int h, int w) { if (k++ != index) return false; b = UtBuf{off, rows, c, h, w}; return true; };
    for (int i = 0; i < 3; ++i) {
        const int c = UT_WIDTHS[i];
        if (hit(p.a1[i], n, c, g.h[i], g.w[i]) || hit(p.r1[i], n, c, g.h[i], g.w[i]) || hit(p.g_r1[i], n, c, g.h[i], g.w[i]) ||
            hit(p.skip[i], n, c, g.hs[i], g.ws[i]) || hit(p.g_skip[i], n, c, g.hs[i], g.ws[i])) return true;
        if (i < 2 && (hit(p.pool[i], n, c, g.hs[i] / 2, g.ws[i] / 2) || hit(p.g_pool[i], n, c, g.hs[i] / 2, g.ws[i] / 2))) return true;
        if (hit(p.mean[i], 1, c, 1, 1) || hit(p.invstd[i], 1, c, 1, 1)) return true;
    }
    for (int j = 0; j < 2; ++j) {
        const int c2 = UT_WIDTHS[2 - j] / 2, mh = g.dh[j] + 2, mw = g.dw[j] + 2;
        if (hit(p.up[j], n, c2, g.uh[j], g.uw[j]) || hit(p.g_up[j], n, c2, g.uh[j], g.uw[j]) || hit(p.r[j], n, c2, mh, mw) ||
            hit(p.nrm[j], n, c2, mh, mw) || hit(p.g_nrm[j], n, c2, mh, mw) || hit(p.dout[j], n, c2, g.dh[j], g.dw[j]) ||
            hit(p.g_dout[j], n, c2, g.dh[j], g.dw[j]) || hit(p.mean[3 + j], 1, c2, 1, 1) || hit(p.invstd[3 + j], 1, c2, 1, 1)) return true;
    }
    size_t wmax = 0;
    for (int q = 0; q < UT_NPARAM; ++q) { const size_t f = ut_param_floats(cin, q); wmax = f > wmax ? f : wmax; }
    return hit(p.hm, n, 1, g.dh[1], g.dw[1]) || hit(p.g_hm, n, 1, g.dh[1], g.dw[1]) || hit(p.wpart, UT_WCHUNK_MAX_N, (int)wmax, 1, 1);
}

// buffer `index` of the plan of a supported shape; false for an unsupported shape or an index outside [0, UT_NBUF)
static inline bool ut_workspace_buffer(int n, int cin, int h8, int w8, int index, UtBuf& b) {
    UtGeo g;
    if (n <= 0 || cin <= 0 || cin % 8 != 0 || index < 0 || index >= UT_NBUF || !ut_geo(h8, w8, g)) return false;
    UtPlan p;
    ut_plan(g, n, cin, p);
    return ut_plan_buffer(g, p, n, cin, index, b);
}

static inline size_t ut_workspace_bytes(int n, int cin, int h8, int w8) {
    UtGeo g;
    if (n <= 0 || cin <= 0 || cin % 8 != 0 || !ut_geo(h8, w8, g)) return 0;
    UtPlan p;
    ut_plan(g, n, cin, p);
    return p.total * sizeof(float) + 256;
}
