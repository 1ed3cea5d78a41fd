// Backward of the tail of RAFT's last iteration -- the flow head, the mask head and the convex 8x up-sampling (core/RAFT/core/update.py
// FlowHead / BasicUpdateBlock.mask, core/RAFT/core/raft.py RAFT.upsample_flow):
//     t_f = relu(conv3x3(net; fh.conv1))   delta = conv3x3(t_f; fh.conv2)
//     t_m = relu(conv3x3(net; mask.0))     m = 0.25 * conv1x1(t_m; mask.2)
//     flow_up = upsample_convex(flow_prev + delta, m)
// Upstream detaches coords1 at the top of every iteration, so this tail carries the EXACT pose-loss gradient of the eight head parameters.
// Here: the up-sampling's adjoint, the weight (and bias) gradient of a stride-1 'same' convolution as a GEMM on the f32 matrix cores with a
// fixed split of the pixel axis -- for the heads' 3x3 and 1x1 and for the update block's 1x5, 5x1 and 7x7 layers alike --, the data gradient
// of the 2-channel output layer with t_f's ReLU mask, and the ReLU mask as a pass of its own.  The other data gradients are FORWARD
// convolutions on transposed, flipped weights and reuse the forward's kernels (ops.py).
// No float atomics anywhere; every sum runs in an order fixed by the shapes, so two runs give the same bits on any device.
#include "rpe_common.h"
#include "upsample_device.h"
#include "bw_gemm.h"

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------ convex up-sampling, adjoint
// up[c][8y+i][8x+j] = sum_k p_k(y,x,i,j) * 8 flow[c][(y,x) + d_k],  p = softmax_k(mask[k*64 + i*8 + j][y][x]),  zero outside the map.
//   d mask_k = p_k (g_k - sum_k' p_k' g_k'),  g_k = gu_x * 8 flow_x[(y,x)+d_k] + gu_y * 8 flow_y[(y,x)+d_k]            per sub-pixel
//   d flow[c][y][x] = 8 sum_k S_k,c[(y,x) - d_k],  S_k,c[cell] = sum_ij p_k(cell,i,j) gu_c(cell,i,j)       the nine cells whose window holds (y,x)
// One thread per 1/8 cell of a 16 x 16 tile whose inner 14 x 14 the workgroup owns: every thread recomputes the softmax of its cell's 64
// sub-pixels (the forward's code, in double), the owners store d mask, all leave their 18 sums S in LDS, and the owners GATHER d flow from the
// nine neighbours' sums -- the halo cells are computed by two workgroups instead of being scattered to.
#define UB_T 16
#define UB_I (UB_T - 2)
__global__ __launch_bounds__(UB_T * UB_T) void k_upsample_convex_bwd(const float* __restrict__ gu, const float* __restrict__ flow,
                                                                     const float* __restrict__ mask, int h8, int w8, int tiles_x,
                                                                     float* __restrict__ dflow, float* __restrict__ dmask) {
    __shared__ double S[18][UB_T * UB_T];
    const int bz = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ly = threadIdx.x / UB_T, lx = threadIdx.x - ly * UB_T;
    const int y = ty * UB_I + ly - 1, x = tx * UB_I + lx - 1;
    const bool in_map = y >= 0 && y < h8 && x >= 0 && x < w8;
    const bool owner = in_map && ly >= 1 && ly <= UB_I && lx >= 1 && lx <= UB_I;
    const size_t mp = (size_t)h8 * w8;
    double s[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) s[k] = 0.0;
    if (in_map) {
        float fx[9], fy[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {                              // F.unfold(8*flow, 3, padding=1): zero padded, as the forward reads it
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            const bool ok = yy >= 0 && yy < h8 && xx >= 0 && xx < w8;
            fx[k] = ok ? 8.0f * flow[((size_t)bz * 2 + 0) * mp + (size_t)yy * w8 + xx] : 0.0f;
            fy[k] = ok ? 8.0f * flow[((size_t)bz * 2 + 1) * mp + (size_t)yy * w8 + xx] : 0.0f;
        }
        const size_t cell = (size_t)y * w8 + x;
        const float* mb = mask + (size_t)bz * 576 * mp + cell;
        float* db = dmask + (size_t)bz * 576 * mp + cell;
        const size_t W = 8 * (size_t)w8;
        const float* gx = gu + ((size_t)bz * 2 + 0) * 64 * mp;
        const float* gy = gu + ((size_t)bz * 2 + 1) * 64 * mp;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const size_t o = (size_t)(8 * y + i) * W + 8 * (size_t)x;       // 8 floats = 32 bytes, aligned (the entry point checks the base)
            float gxr[8], gyr[8];
            *(float4*)&gxr[0] = *(const float4*)(gx + o); *(float4*)&gxr[4] = *(const float4*)(gx + o + 4);
            *(float4*)&gyr[0] = *(const float4*)(gy + o); *(float4*)&gyr[4] = *(const float4*)(gy + o + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float m[9], mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < 9; ++k) { m[k] = mb[(size_t)(k * 64 + i * 8 + j) * mp]; mx = fmaxf(mx, m[k]); }
                double e[9], sum = 0.0;
                CONVEX_SOFTMAX9(m, mx, e, sum)
                const double inv = 1.0 / sum, ux = (double)gxr[j], uy = (double)gyr[j];
                double g[9], gbar = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) { e[k] *= inv; g[k] = ux * (double)fx[k] + uy * (double)fy[k]; gbar += e[k] * g[k]; }
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    if (owner) db[(size_t)(k * 64 + i * 8 + j) * mp] = (float)(e[k] * (g[k] - gbar));
                    s[k] += e[k] * ux; s[9 + k] += e[k] * uy;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 18; ++k) S[k][threadIdx.x] = s[k];
    __syncthreads();
    if (owner) {
        double ax = 0.0, ay = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {                              // the cell whose tap k is (y,x): (y,x) - d_k, inside the tile for every owner
            const int src = (ly - (k / 3 - 1)) * UB_T + lx - (k % 3 - 1);
            ax += S[k][src]; ay += S[9 + k][src];                  // (a cell outside the map left zeros)
        }
        dflow[((size_t)bz * 2 + 0) * mp + (size_t)y * w8 + x] = (float)(8.0 * ax);
        dflow[((size_t)bz * 2 + 1) * mp + (size_t)y * w8 + x] = (float)(8.0 * ay);
    }
}

// ------------------------------------------------------------------------------------------------------------ convolution, weight gradient
// dW[co][ci][ky][kx] = sum_{b,y,x} dy[b][co][y][x] * x[b][ci][y + ky - kh/2][x + kx - kw/2]  (zero outside the map):  a GEMM with
// M = cout, N = cin * taps (n = ci * taps + tap: dW's own layout), K = b * h * w.  Both operands are contiguous along K in memory.
//
// The split of K: chunks of split_chunk(K, 64, 1024) pixels -- a function of b * h * w alone, never of the device --, chunk c -> partial c,
// and the partials are added in index order in f64 (k_splitk_reduce).  Inside a chunk the f32 matrix cores sum in steps of 32 pixels, each
// step's pixels in the fixed order of the instruction: one bit pattern per shape.
// (the tile's body and the second pass: bw_gemm.h, which corr_backward.hip shares; here: the kernel sizes and their one launch path)
static inline long long bw_chunk(long long K) { return split_chunk(K, 64, 1024); }
static inline int bw_chunks(long long K) { return split_chunks(K, 64, 1024); }

// grid (N tiles, M tiles, chunks): M = cout, N = cin * taps, at any cout (a ragged M or N tile is selected to zero: convf1's 2 x 49 = 98
// columns fill one tile in part)
template <int KH, int KW>
__global__ __launch_bounds__(256) void k_bw_gemm(const float* __restrict__ x, long long xbs, const float* __restrict__ dy, long long dybs,
                                                 int cin, int cout, int h, int w, long long K, long long kc, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sA[BW_BM * BW_LD];
    __shared__ __attribute__((aligned(16))) float sB[BW_BN * BW_LD];
    bw_gemm_body<KH, KW>(x, xbs, dy, dybs, cin, cout, h, w, K, kc, part, sA, sB);
}

// The layers with one or two output channels (FlowHead.conv2, 256 -> 2) do not fill a matrix tile: a plain kernel, one workgroup per
// (input channel, chunk), every thread walking the chunk's pixels with stride 256 and the workgroup adding its threads' sums in a fixed
// tree.  Same chunks, same partials, same second pass as the GEMM.
template <int TAPS>
__global__ __launch_bounds__(256) void k_bw_small(const float* __restrict__ x, long long xbs, const float* __restrict__ dy, long long dybs,
                                                  int cin, int cout, int h, int w, long long K, long long kc, float* __restrict__ part) {
    __shared__ double red[4][2 * TAPS];
    const int ci = blockIdx.x, hw = h * w;
    const long long kbeg = (long long)blockIdx.y * kc, kend = kbeg + kc < K ? kbeg + kc : K;
    double acc[2][TAPS];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int t = 0; t < TAPS; ++t) acc[o][t] = 0.0;
    for (long long k = kbeg + threadIdx.x; k < kend; k += 256) {
        const int bb = (int)(k / hw), p = (int)(k - (long long)bb * hw);
        const int py = p / w, px = p - py * w;
        const float* db = dy + (size_t)bb * dybs + p;
        const double d0 = (double)db[0], d1 = cout > 1 ? (double)db[hw] : 0.0;
        const float* xb = x + (size_t)bb * xbs + (size_t)ci * hw;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int yy = TAPS == 9 ? py + t / 3 - 1 : py, xx = TAPS == 9 ? px + t % 3 - 1 : px;
            const bool ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
            const float v = xb[ok ? yy * w + xx : p];
            const double xv = ok ? (double)v : 0.0;
            acc[0][t] += d0 * xv; acc[1][t] += d1 * xv;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const double v = wave_sum(acc[o][t]);
            if (lane == 0) red[wv][o * TAPS + t] = v;
        }
    __syncthreads();
    if (threadIdx.x < 2 * TAPS) {
        const int o = threadIdx.x / TAPS, t = threadIdx.x - o * TAPS;
        const double v = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        if (o < cout) part[(size_t)blockIdx.y * cout * cin * TAPS + ((size_t)o * cin + ci) * TAPS + t] = (float)v;
    }
}

// db[co] = sum of dy's channel co: one workgroup per (channel, chunk) -> an f64 partial, then the same index-order sum
__global__ __launch_bounds__(256) void k_bw_bias_part(const float* __restrict__ dy, long long dybs, int cout, int hw, long long K, long long kc,
                                                      double* __restrict__ part) {
    __shared__ double red[4];
    const int co = blockIdx.x;
    const long long kbeg = (long long)blockIdx.y * kc, kend = kbeg + kc < K ? kbeg + kc : K;
    double s = 0.0;
    for (long long k = kbeg + threadIdx.x; k < kend; k += 256) {
        const int bb = (int)(k / hw), p = (int)(k - (long long)bb * hw);
        s += (double)dy[(size_t)bb * dybs + (size_t)co * hw + p];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * cout + co] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_bw_bias_sum(const double* __restrict__ part, int chunks, int cout, double scale, float* __restrict__ db) {
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= cout) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * cout + co];
    db[co] = (float)(s * scale);
}

// ------------------------------------------------------------------------------------------------------------ data gradients, small parts
// FlowHead.conv2's data gradient with the ReLU mask of its input:  dx[c][y][x] = (act[c][y][x] > 0) * sum_{o,ky,kx} W[o][c][ky][kx] *
// dy[o][y - ky + 1][x - kx + 1] -- two incoming planes, 18 products per element, bandwidth work.  grid (pixels / 256, c, b).
__global__ __launch_bounds__(256) void k_conv3x3_to2_bwd_data(const float* __restrict__ dy, long long dybs, const float* __restrict__ wgt,
                                                              const float* __restrict__ act, long long abs_, int C, int h, int w,
                                                              float* __restrict__ dx, long long dxbs) {
    const int c = blockIdx.y, bz = blockIdx.z, hw = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int py = p / w, px = p - py * w;
    const float* d0 = dy + (size_t)bz * dybs;
    const float* w0 = wgt + (size_t)c * 9;                          // (2, C, 3, 3): uniform over the workgroup
    const float* w1 = wgt + (size_t)(C + c) * 9;
    float a = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = py - (t / 3 - 1), xx = px - (t % 3 - 1);
        const bool ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const int q = ok ? yy * w + xx : p;
        const float v0 = d0[q], v1 = d0[hw + q];
        a = fmaf(ok ? v0 : 0.0f, w0[t], a);
        a = fmaf(ok ? v1 : 0.0f, w1[t], a);
    }
    if (act) a = act[(size_t)bz * abs_ + (size_t)c * hw + p] > 0.0f ? a : 0.0f;
    dx[(size_t)bz * dxbs + (size_t)c * hw + p] = a;
}

// out = act > 0 ? grad : 0, channel slices (out may be grad: in place)
__global__ __launch_bounds__(256) void k_relu_bwd(const float* grad, long long gbs, const float* __restrict__ act, long long abs_, size_t per,
                                                  float* out, long long obs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const float g = grad[(size_t)bz * gbs + e];
        out[(size_t)bz * obs + e] = act[(size_t)bz * abs_ + e] > 0.0f ? g : 0.0f;
    }
}

// The forward convolution kernels add their products in one k-ordered f32 chain, whose rounding error grows with the square root of the
// term count: at 1152 (128 channels x 9 taps) and 4608 terms it is 3-5 times that of a blocked float32 sum.  The tail therefore runs them
// on GROUPS of input channels and adds the groups' results here, in group order, in f64:  out = act(sum_g part[g] + bias[c]).
__global__ __launch_bounds__(256) void k_sum_groups(const float* __restrict__ parts, int groups, size_t group_stride, int hw, size_t per,
                                                    const float* __restrict__ bias, int relu, float* __restrict__ out, long long obs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += (double)parts[(size_t)g * group_stride + (size_t)bz * per + e];
        if (bias) s += (double)bias[e / hw];
        float v = (float)s;
        if (relu) v = v < 0.0f ? 0.0f : v;
        out[(size_t)bz * obs + e] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- entry points
extern "C" int rpe_upsample_convex_backward(const float* grad_up, const float* flow, const float* mask, int b, int h8, int w8,
                                            float* d_flow, float* d_mask, void* stream) {
    if (!grad_up || !flow || !mask || !d_flow || !d_mask || b < 0 || b > 65535 || h8 <= 0 || w8 <= 0) return RPE_E_BADARG;
    if (!aligned16(grad_up)) return RPE_E_BADARG;                    // rows of 8 w8 floats: a cell's 8 sub-pixels are two 16-byte pieces
    if ((long long)h8 * w8 * 576 >= (1LL << 31)) return RPE_E_UNSUPPORTED;
    if (b == 0) return RPE_OK;
    const int tx = ceil_div(w8, UB_I), ty = ceil_div(h8, UB_I);
    hipLaunchKernelGGL(k_upsample_convex_bwd, dim3(tx * ty, b), dim3(UB_T * UB_T), 0, (hipStream_t)stream, grad_up, flow, mask, h8, w8, tx,
                       d_flow, d_mask);
    return rpe_check_launch();
}

// the kernel sizes, each with 'same' padding: the heads' 3x3 and 1x1, the update block's 1x5, 5x1 and 7x7
typedef void (*bw_kernel_t)(const float*, long long, const float*, long long, int, int, int, int, long long, long long, float*);
static inline bw_kernel_t bw_gemm_kernel(int kh, int kw) {
    if (kh == 3 && kw == 3) return k_bw_gemm<3, 3>;
    if (kh == 1 && kw == 1) return k_bw_gemm<1, 1>;
    if (kh == 1 && kw == 5) return k_bw_gemm<1, 5>;
    if (kh == 5 && kw == 1) return k_bw_gemm<5, 1>;
    if (kh == 7 && kw == 7) return k_bw_gemm<7, 7>;
    return nullptr;
}

// one or two output channels at 3x3 and 1x1: no matrix tile to fill (nullptr: the GEMM)
static inline bw_kernel_t bw_small_kernel(int kh, int kw, int cout) {
    if (cout > 2) return nullptr;
    if (kh == 3 && kw == 3) return k_bw_small<9>;
    if (kh == 1 && kw == 1) return k_bw_small<1>;
    return nullptr;
}

static inline bool bw_shape_ok(int b, int cin, int cout, int h, int w, int kh, int kw) {
    return b > 0 && cin > 0 && cout > 0 && h > 0 && w > 0 && bw_gemm_kernel(kh, kw);
}

// floats: partials (chunks, cout, cin, kh, kw), rounded up to 256 bytes | doubles: bias partials (chunks, cout)
extern "C" size_t rpe_conv_bwd_weight_workspace_bytes(int b, int cin, int cout, int h, int w, int kh, int kw) {
    if (!bw_shape_ok(b, cin, cout, h, w, kh, kw)) return 0;
    const long long K = (long long)b * h * w;
    const size_t chunks = (size_t)bw_chunks(K);
    const size_t wbytes = (chunks * cout * cin * kh * kw * sizeof(float) + 255) / 256 * 256;
    return wbytes + (chunks * cout * sizeof(double) + 255) / 256 * 256;
}

extern "C" int rpe_conv_bwd_weight(const float* x, long long x_batch_stride, const float* dy, long long dy_batch_stride, int b, int cin,
                                   int cout, int h, int w, int kh, int kw, float scale, float* d_weight, float* d_bias, void* workspace, void* stream) {
    if (!x || !dy || !workspace || (!d_weight && !d_bias)) return RPE_E_BADARG;
    if (!bw_shape_ok(b, cin, cout, h, w, kh, kw)) return RPE_E_BADARG;
    if (x_batch_stride < (long long)cin * h * w || dy_batch_stride < (long long)cout * h * w || !aligned16(workspace)) return RPE_E_BADARG;
    const long long K = (long long)b * h * w;
    const long long per = (long long)cout * cin * kh * kw;
    if (K >= (1LL << 31) || per >= (1LL << 31) || (long long)cin * h * w >= (1LL << 31) || (long long)cout * h * w >= (1LL << 31))
        return RPE_E_UNSUPPORTED;                                    // offsets inside a batch item and pixel indices are 32 bits
    const long long kc = bw_chunk(K);
    const int chunks = bw_chunks(K), taps = kh * kw;
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    double* bpart = (double*)((char*)workspace + ((size_t)chunks * per * sizeof(float) + 255) / 256 * 256);
    if (d_weight) {
        if (const bw_kernel_t small = bw_small_kernel(kh, kw, cout)) {
            hipLaunchKernelGGL(small, dim3(cin, chunks), dim3(256), 0, s, x, x_batch_stride, dy, dy_batch_stride, cin, cout, h, w, K, kc, part);
        } else {
            const dim3 g(ceil_div((long long)cin * taps, BW_BN), ceil_div(cout, BW_BM), chunks);
            if (g.y > 65535) return RPE_E_UNSUPPORTED;
            hipLaunchKernelGGL(bw_gemm_kernel(kh, kw), g, dim3(256), 0, s, x, x_batch_stride, dy, dy_batch_stride, cin, cout, h, w, K, kc, part);
        }
        splitk_reduce_launch(part, 1, chunks, per, (double)scale, d_weight, s);
    }
    if (d_bias) {
        hipLaunchKernelGGL(k_bw_bias_part, dim3(cout, chunks), dim3(256), 0, s, dy, dy_batch_stride, cout, h * w, K, kc, bpart);
        hipLaunchKernelGGL(k_bw_bias_sum, dim3(ceil_div(cout, 256)), dim3(256), 0, s, (const double*)bpart, chunks, cout, (double)scale, d_bias);
    }
    return rpe_check_launch();
}

extern "C" int rpe_conv3x3_to2_bwd_data(const float* dy, long long dy_batch_stride, const float* weight, const float* act,
                                        long long act_batch_stride, int b, int c, int h, int w, float* dx, long long dx_batch_stride,
                                        void* stream) {
    if (!dy || !weight || !dx || b < 0 || b > 65535 || c <= 0 || c > 65535 || h <= 0 || w <= 0) return RPE_E_BADARG;
    if (dy_batch_stride < 2LL * h * w || dx_batch_stride < (long long)c * h * w || (act && act_batch_stride < (long long)c * h * w))
        return RPE_E_BADARG;
    if ((long long)c * h * w >= (1LL << 31)) return RPE_E_UNSUPPORTED;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_conv3x3_to2_bwd_data, dim3(ceil_div((long long)h * w, 256), c, b), dim3(256), 0, (hipStream_t)stream, dy,
                       dy_batch_stride, weight, act, act_batch_stride, c, h, w, dx, dx_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_relu_backward(const float* grad, long long grad_batch_stride, const float* act, long long act_batch_stride, int b, int c,
                                 int hw, float* out, long long out_batch_stride, void* stream) {
    if (!grad || !act || !out || b < 0 || b > 65535 || c <= 0 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (grad_batch_stride < per || act_batch_stride < per || out_batch_stride < per) return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_relu_bwd, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, grad, grad_batch_stride, act,
                       act_batch_stride, (size_t)per, out, out_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_sum_groups(const float* parts, int groups, int b, int c, int hw, const float* bias, int relu, float* out,
                              long long out_batch_stride, void* stream) {
    if (!parts || !out || groups <= 0 || b < 0 || b > 65535 || c <= 0 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (out_batch_stride < per) return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_sum_groups, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, parts, groups,
                       (size_t)b * per, hw, (size_t)per, bias, relu, out, out_batch_stride);
    return rpe_check_launch();
}
