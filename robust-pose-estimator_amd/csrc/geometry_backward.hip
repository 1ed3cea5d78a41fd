// Backward of the fused geometry stage (geometry.hip): the adjoint of depth from disparity, back-projection, the bilinear warps by the
// temporal flow and the two 1/8 stacks -- the link between the gradients the pose layer and the weight heads hand back (pcl1, pcl2w,
// inp1, inp2) and the three flows.  Reference lines: core/pose/pose_net.py:73-79,104-113, core/interpol/flow_utils.py:4-14.
//
// Per row (rows never share anything, so a row's result does not depend on its batch):
//   k_gb_dest   : one thread per 4 pixels of a line (16-byte loads and stores).  grad_depth1 = <G1, ray>, grad_stereo_flow1 = the spread
//                 inp1 channels 0-1, grad_time_flow = sum over the sampled channels of g * d(sample)/d(ix, iy) with torch's convention
//                 (tap differences, a tap outside the image is absent, d ix / d flow.x = 1); and it COUNTS, per source pixel, the
//                 in-image taps that land on it (integer atomics).
//   k_gb_scan_* : exclusive scan of the counts (per 1024-pixel tile, then over the tile sums of a row).
//   k_gb_fill   : every tap writes (destination index * 4 + tap) into its source pixel's list (slot by integer atomic: any order).
//   k_gb_src    : one thread per 4 source pixels.  Sorts each list (ascending: destination-index order, whatever order the slots were
//                 handed out in), re-derives each entry's tap weight from the temporal flow of its destination, sums weight * upstream
//                 in that order, and applies the disparity adjoint  d depth / d sf.x = b / sf.x^2  (0 where the depth was clamped).
// No float atomics; the only run-to-run freedom is the order of the list slots, which the sort removes: results are bit-identical from
// run to run.  Sampling positions and tap indices come from sampling.h / geometry_device.h exactly as in the forward (float32, one
// rounded operation at a time); everything after those decisions is accumulated in float64 in registers and rounded once on the store
// (the stage is bandwidth-bound: the f64 arithmetic is free, and the result carries no summation-order error of its own).
#include "geometry_device.h"

#define GB_TILE 1024          // pixels per scan tile (256 threads x int4)
#define GB_INSERTION_MAX 24   // lists up to this length are sorted by insertion, longer ones by heapsort (both in place)

struct K64 { double m[9]; };

// component j of a 4-vector held in registers (j is a constant after unrolling; taking a member's address would put it in scratch)
__device__ __forceinline__ float comp(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ int comp(const int4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// the adjugate inverse of invert_k, kept in f64
__device__ __forceinline__ K64 invert_k64(const float* K) {
    double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    double r = 1.0 / (a * A + b * B + c * C);
    K64 o;
    o.m[0] = A * r; o.m[1] = -(b * i - c * h) * r; o.m[2] = (b * f - c * e) * r;
    o.m[3] = B * r; o.m[4] = (a * i - c * g) * r;  o.m[5] = -(a * f - c * d) * r;
    o.m[6] = C * r; o.m[7] = -(a * h - b * g) * r; o.m[8] = (a * e - b * d) * r;
    return o;
}

// <g, K^-1 [x+.5, y+.5, 1]>
__device__ __forceinline__ double dot_ray(const K64& Ki, int x, int y, double g0, double g1, double g2) {
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    return g0 * (Ki.m[0] * px + Ki.m[1] * py + Ki.m[2]) + g1 * (Ki.m[3] * px + Ki.m[4] * py + Ki.m[5]) +
           g2 * (Ki.m[6] * px + Ki.m[7] * py + Ki.m[8]);
}

// the 2x2 centre pixels (offsets 3 and 4) of each 8x8 cell: the only pixels the x0.125 stacks read, each with weight 1/4
__device__ __forceinline__ bool is_centre(int x, int y) { return (((x & 7) - 3) >> 1) == 0 && (((y & 7) - 3) >> 1) == 0; }

// upstream gradient of the warp's 8 sampled channels at one destination pixel: warped cloud (3), warped stereo flow (2), warped image (3)
struct Upstream { double c[3], s[2], im[3]; };

__device__ __forceinline__ double quarter(const float* ginp, int row, int ch, size_t hw8, size_t cell) {
    return 0.25 * (double)ginp[((size_t)row * 8 + ch) * hw8 + cell];
}

struct Frac { int x0, y0; double wx0, wx1, wy0, wy1; };      // floor taps and the exact weights (x0 + 1 - ix, ix - x0, ...)

__device__ __forceinline__ Frac frac_taps(float fx, float fy, int x, int y, int w, int h) {
    const float ix = sample_pos(fx, x, w), iy = sample_pos(fy, y, h);
    Frac t;
    float fx0, fy0;
    t.x0 = safe_floor(ix, fx0); t.y0 = safe_floor(iy, fy0);
    t.wx0 = (double)((fx0 + 1.0f) - ix); t.wx1 = (double)(ix - fx0);       // exact in f32 for every position that reads
    t.wy0 = (double)((fy0 + 1.0f) - iy); t.wy1 = (double)(iy - fy0);
    return t;
}

__device__ __forceinline__ double tap_weight(const Frac& t, int k) { return ((k & 1) ? t.wx1 : t.wx0) * ((k & 2) ? t.wy1 : t.wy0); }

// ---------------------------------------------------------------------------------------------------------------- destination pass
__global__ __launch_bounds__(256) void k_gb_dest(const float* __restrict__ sflow2, const float* __restrict__ tflow,
                                                 const float* __restrict__ baseline, const float* __restrict__ K,
                                                 const float* __restrict__ image2l, int h, int w,
                                                 const float* __restrict__ gpcl1, const float* __restrict__ gpcl2w,
                                                 const float* __restrict__ ginp1, const float* __restrict__ ginp2,
                                                 float* __restrict__ gtflow, float* __restrict__ gsflow1, float* __restrict__ gdepth1,
                                                 int* __restrict__ cnt) {
    const int row = blockIdx.y;
    const size_t hw = (size_t)h * w, hw8 = hw / 64;
    const size_t p4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p4 >= hw) return;
    const int y = (int)(p4 / w), xb = (int)(p4 - (size_t)y * w);
    const K64 Ki = invert_k64(K + (size_t)row * 9);
    const double b = (double)baseline[row];
    const float* sf2 = sflow2 + (size_t)row * 2 * hw;
    const float* im2 = image2l + (size_t)row * 3 * hw;
    const float4 tfx = *(const float4*)(tflow + (size_t)row * 2 * hw + p4), tfy = *(const float4*)(tflow + (size_t)row * 2 * hw + hw + p4);
    float4 g1[3], g2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g1[c] = g2[c] = make_float4(0.f, 0.f, 0.f, 0.f);                                  // a NULL upstream gradient is zero
        if (gpcl1) g1[c] = *(const float4*)(gpcl1 + ((size_t)row * 3 + c) * hw + p4);
        if (gpcl2w) g2[c] = *(const float4*)(gpcl2w + ((size_t)row * 3 + c) * hw + p4);
    }
    int* rcnt = cnt ? cnt + (size_t)row * hw : nullptr;
    float o_tx[4], o_ty[4], o_d1[4], o_s1x[4], o_s1y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = xb + j;
        const bool centre = is_centre(x, y);
        const size_t cell = (size_t)(y >> 3) * (w >> 3) + (x >> 3);
        double a0 = (double)comp(g1[0], j), a1 = (double)comp(g1[1], j), a2 = (double)comp(g1[2], j);
        double s1x = 0.0, s1y = 0.0;
        if (centre && ginp1) {
            s1x = quarter(ginp1, row, 0, hw8, cell); s1y = quarter(ginp1, row, 1, hw8, cell);
            a0 += quarter(ginp1, row, 5, hw8, cell); a1 += quarter(ginp1, row, 6, hw8, cell); a2 += quarter(ginp1, row, 7, hw8, cell);
        }
        o_s1x[j] = (float)s1x; o_s1y[j] = (float)s1y;
        o_d1[j] = (float)dot_ray(Ki, x, y, a0, a1, a2);                                   // pcl1 = depth1 * ray
        Upstream u;
        u.c[0] = (double)comp(g2[0], j); u.c[1] = (double)comp(g2[1], j); u.c[2] = (double)comp(g2[2], j);
        u.s[0] = u.s[1] = u.im[0] = u.im[1] = u.im[2] = 0.0;
        const bool stacked = centre && ginp2;
        if (stacked) {
            u.s[0] = quarter(ginp2, row, 0, hw8, cell); u.s[1] = quarter(ginp2, row, 1, hw8, cell);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                u.im[c] = quarter(ginp2, row, 2 + c, hw8, cell);
                u.c[c] += quarter(ginp2, row, 5 + c, hw8, cell);
            }
        }
        const bool listed = rcnt && (gpcl2w || stacked);                                 // k_gb_fill lists exactly these taps
        const Frac t = frac_taps(comp(tfx, j), comp(tfy, j), x, y, w, h);
        double m[4];                                                                     // sum_channels g * (tap value), 0 for an absent tap
        bool any = false;                                                                // (a position that does not read has no tap at all)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = t.x0 + (k & 1), yy = t.y0 + (k >> 1);
            m[k] = 0.0;
            if (inb(xx, yy, w, h)) {
                const size_t q = (size_t)yy * w + xx;
                const float s = sf2[q];
                bool v;
                depth_from_disp((float)b, s, v);
                const double d = v ? b / -(double)s : 1.0;
                m[k] = d * dot_ray(Ki, xx, yy, u.c[0], u.c[1], u.c[2]);
                if (stacked) {
                    m[k] += u.s[0] * (double)s + u.s[1] * (double)sf2[hw + q];
#pragma unroll
                    for (int c = 0; c < 3; ++c) m[k] += u.im[c] * (double)im2[(size_t)c * hw + q];
                }
                if (listed) atomicAdd(rcnt + q, 1);
                any = true;
            }
        }
        o_tx[j] = any ? (float)(t.wy0 * (m[1] - m[0]) + t.wy1 * (m[3] - m[2])) : 0.0f;
        o_ty[j] = any ? (float)(t.wx0 * (m[2] - m[0]) + t.wx1 * (m[3] - m[1])) : 0.0f;
    }
    if (gtflow) {
        *(float4*)(gtflow + (size_t)row * 2 * hw + p4) = make_float4(o_tx[0], o_tx[1], o_tx[2], o_tx[3]);
        *(float4*)(gtflow + (size_t)row * 2 * hw + hw + p4) = make_float4(o_ty[0], o_ty[1], o_ty[2], o_ty[3]);
    }
    if (gsflow1) {
        *(float4*)(gsflow1 + (size_t)row * 2 * hw + p4) = make_float4(o_s1x[0], o_s1x[1], o_s1x[2], o_s1x[3]);
        *(float4*)(gsflow1 + (size_t)row * 2 * hw + hw + p4) = make_float4(o_s1y[0], o_s1y[1], o_s1y[2], o_s1y[3]);
    }
    if (gdepth1) *(float4*)(gdepth1 + (size_t)row * hw + p4) = make_float4(o_d1[0], o_d1[1], o_d1[2], o_d1[3]);
}

// -------------------------------------------------------------------------------------------------------------------------- scan
// exclusive scan of one value per thread over a 256-thread block (Hillis-Steele in LDS); total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < 256; off <<= 1) {
        int add = t >= off ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int incl = lds[t];
    total = lds[255];
    __syncthreads();
    return incl - v;
}

// offs[p] = exclusive scan of cnt inside p's tile; tsum[row][tile] = the tile's total
__global__ __launch_bounds__(256) void k_gb_scan_tile(const int* __restrict__ cnt, int hw, int tiles, int* __restrict__ offs,
                                                      int* __restrict__ tsum) {
    __shared__ int lds[256];
    const int row = blockIdx.y, tile = blockIdx.x;
    const int p4 = tile * GB_TILE + threadIdx.x * 4;
    int4 c = make_int4(0, 0, 0, 0);
    if (p4 < hw) c = *(const int4*)(cnt + (size_t)row * hw + p4);
    int total;
    const int base = block_excl_scan(c.x + c.y + c.z + c.w, lds, total);
    if (p4 < hw) *(int4*)(offs + (size_t)row * hw + p4) = make_int4(base, base + c.x, base + c.x + c.y, base + c.x + c.y + c.z);
    if (threadIdx.x == 0) tsum[(size_t)row * tiles + tile] = total;
}

// tbase[row][tile] = exclusive scan of tsum over a row's tiles (one block per row)
__global__ __launch_bounds__(256) void k_gb_scan_rows(const int* __restrict__ tsum, int tiles, int* __restrict__ tbase) {
    __shared__ int lds[256];
    const int row = blockIdx.x;
    int carry = 0;
    for (int t0 = 0; t0 < tiles; t0 += 256) {
        const int t = t0 + threadIdx.x;
        const int v = t < tiles ? tsum[(size_t)row * tiles + t] : 0;
        int total;
        const int e = block_excl_scan(v, lds, total);
        if (t < tiles) tbase[(size_t)row * tiles + t] = carry + e;
        carry += total;
    }
}

// -------------------------------------------------------------------------------------------------------------------------- fill
__global__ __launch_bounds__(256) void k_gb_fill(const float* __restrict__ tflow, int h, int w, int has_gpcl2w, int tiles,
                                                 const int* __restrict__ offs, const int* __restrict__ tbase, int* __restrict__ cur,
                                                 int* __restrict__ list) {
    const int row = blockIdx.y;
    const size_t hw = (size_t)h * w;
    const size_t p4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p4 >= hw) return;
    const int y = (int)(p4 / w), xb = (int)(p4 - (size_t)y * w);
    const float4 tfx = *(const float4*)(tflow + (size_t)row * 2 * hw + p4), tfy = *(const float4*)(tflow + (size_t)row * 2 * hw + hw + p4);
    const int* roffs = offs + (size_t)row * hw;
    const int* rbase = tbase + (size_t)row * tiles;
    int* rcur = cur + (size_t)row * hw;
    int* rlist = list + (size_t)row * 4 * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = xb + j;
        if (!(has_gpcl2w || is_centre(x, y))) continue;
        const Frac t = frac_taps(comp(tfx, j), comp(tfy, j), x, y, w, h);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = t.x0 + (k & 1), yy = t.y0 + (k >> 1);
            if (inb(xx, yy, w, h)) {
                const int q = yy * w + xx;
                const size_t at = (size_t)rbase[q / GB_TILE] + roffs[q] + atomicAdd(rcur + q, 1);
                if (at < 4 * hw) rlist[at] = (int)(p4 + j) * 4 + k;          // (always true: k_gb_dest counted this very tap)
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- source pass
__device__ __forceinline__ void sift_down(int* a, int i, int n) {
    const int v = a[i];
    for (;;) {
        int c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && a[c + 1] > a[c]) ++c;
        if (a[c] <= v) break;
        a[i] = a[c];
        i = c;
    }
    a[i] = v;
}

// ascending, in place; entries are distinct
__device__ __forceinline__ void sort_list(int* a, int n) {
    if (n <= GB_INSERTION_MAX) {
        for (int i = 1; i < n; ++i) {
            const int v = a[i];
            int j = i - 1;
            for (; j >= 0 && a[j] > v; --j) a[j + 1] = a[j];
            a[j + 1] = v;
        }
        return;
    }
    for (int i = n / 2 - 1; i >= 0; --i) sift_down(a, i, n);
    for (int e = n - 1; e > 0; --e) {
        const int v = a[0];
        a[0] = a[e];
        a[e] = v;
        sift_down(a, 0, e);
    }
}

__global__ __launch_bounds__(256) void k_gb_src(const float* __restrict__ sflow2, const float* __restrict__ tflow,
                                                const float* __restrict__ baseline, const float* __restrict__ K, int h, int w,
                                                const float* __restrict__ gpcl2w, const float* __restrict__ ginp2, int tiles,
                                                const int* __restrict__ cnt, const int* __restrict__ offs,
                                                const int* __restrict__ tbase, int* __restrict__ list, float* __restrict__ gsflow2) {
    const int row = blockIdx.y;
    const size_t hw = (size_t)h * w, hw8 = hw / 64;
    const size_t q4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (q4 >= hw) return;
    const int y = (int)(q4 / w), xb = (int)(q4 - (size_t)y * w);
    const K64 Ki = invert_k64(K + (size_t)row * 9);
    const double b = (double)baseline[row];
    const float* tf = tflow + (size_t)row * 2 * hw;
    const int4 c4 = *(const int4*)(cnt + (size_t)row * hw + q4);
    const int4 o4 = *(const int4*)(offs + (size_t)row * hw + q4);
    const float4 s4 = *(const float4*)(sflow2 + (size_t)row * 2 * hw + q4);
    const int tb = tbase[(size_t)row * tiles + q4 / GB_TILE];                            // (4 | GB_TILE: the four pixels share a tile)
    int* rlist = list + (size_t)row * 4 * hw;
    float ox[4], oy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int len = comp(c4, j);
        int* L = rlist + tb + comp(o4, j);
        sort_list(L, len);
        double S0 = 0.0, S1 = 0.0, S2 = 0.0, F0 = 0.0, F1 = 0.0;
        for (int i = 0; i < len; ++i) {
            const int e = L[i];
            const int p = e >> 2, k = e & 3;
            if ((size_t)(unsigned)p >= hw) continue;                       // (never: k_gb_fill wrote every slot k_gb_dest counted)
            const int py = p / w, px = p - py * w;
            const double wt = tap_weight(frac_taps(tf[p], tf[hw + p], px, py, w, h), k);
            double g0 = 0.0, g1 = 0.0, g2 = 0.0;
            if (gpcl2w) {
                const float* g = gpcl2w + (size_t)row * 3 * hw + p;
                g0 = (double)g[0]; g1 = (double)g[hw]; g2 = (double)g[2 * hw];
            }
            if (ginp2 && is_centre(px, py)) {
                const size_t cell = (size_t)(py >> 3) * (w >> 3) + (px >> 3);
                F0 += wt * quarter(ginp2, row, 0, hw8, cell); F1 += wt * quarter(ginp2, row, 1, hw8, cell);
                g0 += quarter(ginp2, row, 5, hw8, cell); g1 += quarter(ginp2, row, 6, hw8, cell); g2 += quarter(ginp2, row, 7, hw8, cell);
            }
            S0 += wt * g0; S1 += wt * g1; S2 += wt * g2;
        }
        const float s = comp(s4, j);
        bool v;
        depth_from_disp((float)b, s, v);
        // pcl2 = depth2 * ray, depth2 = b / -sf.x where 0 < depth <= 1 (else the constant 1): d depth2 / d sf.x = b / sf.x^2
        const double gd = v ? dot_ray(Ki, xb + j, y, S0, S1, S2) * b / ((double)s * (double)s) : 0.0;
        ox[j] = (float)(gd + F0);
        oy[j] = (float)F1;
    }
    *(float4*)(gsflow2 + (size_t)row * 2 * hw + q4) = make_float4(ox[0], ox[1], ox[2], ox[3]);
    *(float4*)(gsflow2 + (size_t)row * 2 * hw + hw + q4) = make_float4(oy[0], oy[1], oy[2], oy[3]);
}

// ------------------------------------------------------------------------------------------------------------ first-frame disparity
__global__ __launch_bounds__(256) void k_flow2depth_bwd(const float* __restrict__ sflow, const float* __restrict__ baseline,
                                                        const float* __restrict__ gdepth, int h, int w, float* __restrict__ gsflow) {
    const int row = blockIdx.y;
    const size_t hw = (size_t)h * w;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    const float b = baseline[row], s = sflow[(size_t)row * 2 * hw + p];
    bool v;
    depth_from_disp(b, s, v);
    gsflow[(size_t)row * 2 * hw + p] = v ? (float)((double)gdepth[(size_t)row * hw + p] * (double)b / ((double)s * (double)s)) : 0.0f;
    gsflow[(size_t)row * 2 * hw + hw + p] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------- entry points
static inline size_t gb_tiles(int h, int w) { return ((size_t)h * w + GB_TILE - 1) / GB_TILE; }

// ints: cnt | cur (zeroed together) | offs (n*hw each) | tsum | tbase (n*tiles each) | list (4*n*hw)
extern "C" size_t rpe_depth_backproject_warp_backward_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const size_t hw = (size_t)h * w;
    return (((size_t)n * (7 * hw + 2 * gb_tiles(h, w))) * sizeof(int) + 255) / 256 * 256;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int rpe_depth_backproject_warp_backward(const float* stereo_flow2, const float* time_flow, const float* baseline,
                                                   const float* K, const float* depth1, const float* image2l,
                                                   const float* stereo_flow1, const uint8_t* mask2, int n, int h, int w,
                                                   const float* grad_pcl1, const float* grad_pcl2w, const float* grad_inp1,
                                                   const float* grad_inp2, float* grad_time_flow, float* grad_stereo_flow2,
                                                   float* grad_stereo_flow1, float* grad_depth1, void* workspace, void* stream) {
    if (!stereo_flow2 || !time_flow || !baseline || !K || !depth1 || !image2l || !stereo_flow1 || !mask2 || !workspace)
        return RPE_E_BADARG;
    if (n < 0 || n > 65535 || h <= 0 || w <= 0 || h % 8 || w % 8) return RPE_E_BADARG;
    if (!aligned16(stereo_flow2) || !aligned16(time_flow) || !aligned16(grad_pcl1) || !aligned16(grad_pcl2w) ||
        !aligned16(grad_time_flow) || !aligned16(grad_stereo_flow2) || !aligned16(grad_stereo_flow1) || !aligned16(grad_depth1) ||
        !aligned16(workspace))
        return RPE_E_BADARG;
    const size_t hw = (size_t)h * w;
    if (hw >= ((size_t)1 << 29)) return RPE_E_UNSUPPORTED;                // a list entry is (pixel * 4 + tap) in 32 bits
    if (n == 0) return RPE_OK;
    hipStream_t s = (hipStream_t)stream;
    const int tiles = (int)gb_tiles(h, w);
    int* cnt = (int*)workspace;
    int* cur = cnt + (size_t)n * hw;
    int* offs = cur + (size_t)n * hw;
    int* tsum = offs + (size_t)n * hw;
    int* tbase = tsum + (size_t)n * tiles;
    int* list = tbase + (size_t)n * tiles;
    const bool scatter = grad_stereo_flow2 != nullptr;
    const dim3 g4(ceil_div(hw / 4, 256), n);
    if (scatter && hipMemsetAsync(cnt, 0, 2 * (size_t)n * hw * sizeof(int), s) != hipSuccess) return RPE_E_LAUNCH;
    if (scatter || grad_time_flow || grad_stereo_flow1 || grad_depth1)
        hipLaunchKernelGGL(k_gb_dest, g4, dim3(256), 0, s, stereo_flow2, time_flow, baseline, K, image2l, h, w, grad_pcl1, grad_pcl2w,
                           grad_inp1, grad_inp2, grad_time_flow, grad_stereo_flow1, grad_depth1, scatter ? cnt : (int*)nullptr);
    if (scatter) {
        hipLaunchKernelGGL(k_gb_scan_tile, dim3(tiles, n), dim3(256), 0, s, (const int*)cnt, (int)hw, tiles, offs, tsum);
        hipLaunchKernelGGL(k_gb_scan_rows, dim3(n), dim3(256), 0, s, (const int*)tsum, tiles, tbase);
        if (grad_pcl2w || grad_inp2)
            hipLaunchKernelGGL(k_gb_fill, g4, dim3(256), 0, s, time_flow, h, w, grad_pcl2w ? 1 : 0, tiles, (const int*)offs,
                               (const int*)tbase, cur, list);
        hipLaunchKernelGGL(k_gb_src, g4, dim3(256), 0, s, stereo_flow2, time_flow, baseline, K, h, w, grad_pcl2w, grad_inp2, tiles,
                           (const int*)cnt, (const int*)offs, (const int*)tbase, list, grad_stereo_flow2);
    }
    return rpe_check_launch();
}

extern "C" int rpe_flow2depth_backward(const float* stereo_flow, const float* baseline, const float* grad_depth, int n, int h, int w,
                                       float* grad_stereo_flow, void* stream) {
    if (!stereo_flow || !baseline || !grad_depth || !grad_stereo_flow || n < 0 || n > 65535 || h <= 0 || w <= 0) return RPE_E_BADARG;
    if (n == 0) return RPE_OK;
    hipLaunchKernelGGL(k_flow2depth_bwd, dim3(ceil_div((size_t)h * w, 256), n), dim3(256), 0, (hipStream_t)stream, stereo_flow,
                       baseline, grad_depth, h, w, grad_stereo_flow);
    return rpe_check_launch();
}
