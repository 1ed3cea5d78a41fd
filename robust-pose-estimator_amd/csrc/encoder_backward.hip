// Backward of RAFT's two encoders (core/RAFT/core/extractor.py BasicEncoder / ResidualBlock): what the stride-1 backward files do not have.
//   k_eb_gemm_s2        weight gradient of a STRIDE-2 convolution (3x3 pad 1, 1x1 pad 0, the 7x7 pad 3 stem) on the f32 matrix cores:
//                       bw_gemm.h's tile, chunk rule and second pass, K = b ho wo
//   k_eb_s2_bwd_data    data gradient of the stride-2 3x3 and 1x1 layers in gather form, accumulated in f64
//   k_eb_bn_*           adjoint of a frozen batch norm behind a convolution (cnet): d beta, d gamma, d conv.bias and dz = s dy
//   k_eb_instnorm_bwd   adjoint of an instance norm without affine parameters (fnet), plane moments in f64
//   k_eb_split_act_bwd  adjoint of the context encoder's output activation: tanh on the first channels, ReLU on the rest
// (the residual add needs nothing new: one rpe_relu_backward gives the masked gradient both paths read, rpe_sum_groups adds what they return)
// f32 in memory, no float atomics; every sum runs in an order fixed by the shapes alone, so two runs give the same bits on any device.
#include "rpe_common.h"
#include "bw_gemm.h"

static inline bool eb_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the weight gradient's split of K, rpe_conv_bwd_weight's rule: c(K) = max(1024, round_up(ceil(K / 64), 32))
static inline long long eb_chunk(long long K) { return split_chunk(K, 64, 1024); }
static inline int eb_chunks(long long K) { return split_chunks(K, 64, 1024); }
// the three encoder forms: kernel k with padding k / 2 and stride 2, ho = (hi + 2 p - k) / 2 + 1
static inline bool eb_form_ok(int k, int hi, int wi, int ho, int wo) {
    if (k != 1 && k != 3 && k != 7) return false;
    if (hi <= 0 || wi <= 0) return false;
    const int p = k / 2;
    return ho == (hi + 2 * p - k) / 2 + 1 && wo == (wi + 2 * p - k) / 2 + 1;
}

// ------------------------------------------------------------------------------------------------------------ strided weight gradient
// dW[co][ci][ty][tx] = sum_{b,py,px} dy[b][co][py][px] * x[b][ci][2 py + ty - P][2 px + tx - P]  (zero outside the map): the GEMM of
// bw_gemm_body -- M = cout, N = cin * taps, K = b * ho * wo, the same tile, staging pattern and K permutation -- with the staged pixel's x
// address moved to stride 2.  A copy of that body and not a parameter of it: its stride-1 instantiations keep their code and registers
// (as k_cb_gemm keeps a loop of its own, bw_gemm.h).  In all three forms 2 (ho - 1) <= hi - 1, so a pixel's (2 py, 2 px) lies inside the
// map: the clamped address of a border tap, which is read and SELECTED to zero.
template <int KS>
__global__ __launch_bounds__(256) void k_eb_gemm_s2(const float* __restrict__ x, long long xbs, const float* __restrict__ dy, long long dybs,
                                                    int cin, int cout, int hi, int wi, int ho, int wo, long long K, long long kc,
                                                    float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sA[BW_BM * BW_LD];
    __shared__ __attribute__((aligned(16))) float sB[BW_BN * BW_LD];
    constexpr int TAPS = KS * KS, P = KS / 2;
    typedef typename std::conditional<(TAPS > 31), unsigned long long, unsigned>::type mask_t;      // one bit per tap
    constexpr int NOTAP = TAPS > 31 ? 63 : 31;                       // a bit no tap sets: a row outside the problem
    const int N = cin * TAPS, M = cout;
    const int n0 = blockIdx.x * BW_BN, m0 = blockIdx.y * BW_BM;
    const long long kbeg = (long long)blockIdx.z * kc, kend = kbeg + kc < K ? kbeg + kc : K;
    const int hwo = ho * wo, hwi = hi * wi;
    const int tid = threadIdx.x, kl = tid & 31, r0 = tid >> 5;
    int aoff[16], boff[16], btap[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + r0 + 8 * r, n = n0 + r0 + 8 * r;
        aoff[r] = m < M ? m * hwo : -1;
        const int ci = n / TAPS, tap = n - ci * TAPS;
        boff[r] = ci * hwi + (tap / KS - P) * wi + (tap % KS - P);
        btap[r] = n < N ? tap : NOTAP;
    }
    float ra[16], rb[16];
    auto load = [&](long long kstep) {
        const long long k = kstep + kl;
        const bool kv = k < kend;
        const long long kk = kv ? k : kbeg;                           // (kbeg < K: the grid has no empty chunk)
        const int bb = (int)(kk / hwo), p = (int)(kk - (long long)bb * hwo);
        const int py = p / wo, px = p - py * wo;
        mask_t vm = 0;
        if (TAPS > 1) {
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int yy = 2 * py + t / KS - P, xx = 2 * px + t % KS - P;
                vm |= (mask_t)(kv && yy >= 0 && yy < hi && xx >= 0 && xx < wi) << t;
            }
        } else vm = kv ? 1u : 0u;
        const float* ab = dy + (size_t)bb * dybs + p;
        const float* xb = x + (size_t)bb * xbs + (size_t)(2 * py) * wi + 2 * px;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool av = kv && aoff[r] >= 0;
            const float a = ab[av ? aoff[r] : 0];
            ra[r] = av ? a : 0.0f;
            const bool bv = (vm >> btap[r]) & 1u;
            const float v = xb[bv ? boff[r] : 0];
            rb[r] = bv ? v : 0.0f;
        }
    };
    const int lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int li = lane & 31, lh = lane >> 5;
    // two levels of f32 accumulation: the matrix cores add a block of EB_FOLD steps (128 pixels) into acc, acc is then added into tot and
    // cleared -- a chunk's sum is a chain of at most 64 instruction steps and a chain over its blocks, not one chain over 512 and more
    // (measured against float32 autograd on the CPU, whose GEMM sums in blocks: NOTES.md, "Backward of the encoders")
    constexpr int EB_FOLD = 4;
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[a][c][e] = 0.0f; tot[a][c][e] = 0.0f; }
    int step = 0;
    load(kbeg);
    for (long long ks = kbeg; ks < kend; ks += BW_BK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { sA[(r0 + 8 * r) * BW_LD + kl] = ra[r]; sB[(r0 + 8 * r) * BW_LD + kl] = rb[r]; }
        __syncthreads();
        if (ks + BW_BK < kend) load(ks + BW_BK);
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            float fa[2][4], fb[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float4 va = *(const float4*)&sA[(wm * 64 + a * 32 + li) * BW_LD + lh * 16 + t4 * 4];
                const float4 vb = *(const float4*)&sB[(wn * 64 + a * 32 + li) * BW_LD + lh * 16 + t4 * 4];
                fa[a][0] = va.x; fa[a][1] = va.y; fa[a][2] = va.z; fa[a][3] = va.w;
                fb[a][0] = vb.x; fb[a][1] = vb.y; fb[a][2] = vb.z; fb[a][3] = vb.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a][e], fb[c][e], acc[a][c], 0, 0, 0);
        }
        if (++step == EB_FOLD || ks + BW_BK >= kend) {
            step = 0;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int e = 0; e < 16; ++e) { tot[a][c][e] += acc[a][c][e]; acc[a][c][e] = 0.0f; }
        }
        __syncthreads();
    }
    float* out = part + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n = n0 + wn * 64 + c * 32 + li;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m < M && n < N) out[(size_t)m * N + n] = tot[a][c][e];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------ strided data gradient
// dx[b][ci][y][x] = sum_{co} sum_{taps} W[co][ci][ty][tx] dy[b][co][oy][ox] over the taps with 2 oy + ty - P = y, 2 ox + tx - P = x: per axis the
// taps of the pixel's parity only -- ty = (y + P) & 1 and, at 3x3, that + 2 --, so 1, 2, 2 or 4 taps at 3x3 and one pixel in four at 1x1;
// a pixel no tap reaches is written as an exact zero.  Nothing is zero-inserted.  One thread per (pixel, ci), the chain over cout and the
// taps in f64 (at most 128 x 4 terms here: DESIGN.md 4.3b asks for no f32 chain beyond 288), rounded once.  grid (pixels / 256, cin, b).
template <int KS>
__global__ __launch_bounds__(256) void k_eb_s2_bwd_data(const float* __restrict__ dy, long long dybs, const float* __restrict__ wgt, int cin,
                                                        int cout, int hi, int wi, int ho, int wo, float* __restrict__ dx, long long dxbs) {
    constexpr int P = KS / 2, TAPS = KS * KS;
    const int ci = blockIdx.y, bz = blockIdx.z;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hi * wi) return;
    const int y = p / wi, xq = p - y * wi;
    int oy[2], ox[2], ty[2], tx[2];
    bool vy[2], vx[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        ty[a] = ((y + P) & 1) + 2 * a;
        tx[a] = ((xq + P) & 1) + 2 * a;
        const int ny = y + P - ty[a], nx = xq + P - tx[a];           // even by the choice of the tap
        oy[a] = ny >> 1; ox[a] = nx >> 1;
        vy[a] = ty[a] < KS && ny >= 0 && oy[a] < ho;
        vx[a] = tx[a] < KS && nx >= 0 && ox[a] < wo;
    }
    const int hwo = ho * wo;
    const float* db = dy + (size_t)bz * dybs;
    double acc = 0.0;
    for (int co = 0; co < cout; ++co) {
        const float* wr = wgt + ((size_t)co * cin + ci) * TAPS;
        const float* dr = db + (size_t)co * hwo;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bool ok = vy[a] && vx[c];
                const float d = dr[ok ? oy[a] * wo + ox[c] : 0];
                const float w = wr[ok ? ty[a] * KS + tx[c] : 0];
                acc += ok ? (double)d * (double)w : 0.0;
            }
    }
    dx[(size_t)bz * dxbs + (size_t)ci * hi * wi + p] = (float)acc;
}

// ------------------------------------------------------------------------------------------------------------ frozen batch norm, adjoint
// y = relu?(s (z + bias - mean) + beta), s = gamma / sqrt(var + eps), running statistics: constants.  From dy (behind the ReLU mask) and the
// raw convolution output z:  S0 = sum dy, S1 = sum dy z per channel over (b, pixels) ->
//     d beta = S0,   d gamma = (S1 + (bias - mean) S0) / sqrt(var + eps),   d conv.bias = s S0,   dz = s dy.
// The sums: chunks of c(K), K = b hw, one workgroup per (channel, chunk) -- threads stride the chunk, butterfly per wave, the four waves in
// index order --, the chunks added in index order; all in f64.
__global__ __launch_bounds__(256) void k_eb_bn_part(const float* __restrict__ dy, long long dybs, const float* __restrict__ z, long long zbs,
                                                    int c, int hw, long long K, long long kc, double* __restrict__ part) {
    __shared__ double red[4][2];
    const int ch = blockIdx.x;
    const long long kbeg = (long long)blockIdx.y * kc, kend = kbeg + kc < K ? kbeg + kc : K;
    double s0 = 0.0, s1 = 0.0;
    for (long long k = kbeg + threadIdx.x; k < kend; k += 256) {
        const int bb = (int)(k / hw), p = (int)(k - (long long)bb * hw);
        const double d = (double)dy[(size_t)bb * dybs + (size_t)ch * hw + p];
        s0 += d; s1 += d * (double)z[(size_t)bb * zbs + (size_t)ch * hw + p];
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s0; red[threadIdx.x >> 6][1] = s1; }
    __syncthreads();
    if (threadIdx.x < 2)
        part[((size_t)blockIdx.y * c + ch) * 2 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void k_eb_bn_final(const double* __restrict__ part, int chunks, int c, const float* __restrict__ gamma,
                                                     const float* __restrict__ cbias, const float* __restrict__ mean,
                                                     const float* __restrict__ var, double eps, float* __restrict__ d_gamma,
                                                     float* __restrict__ d_beta, float* __restrict__ d_cbias) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < chunks; ++k) { s0 += part[((size_t)k * c + ch) * 2]; s1 += part[((size_t)k * c + ch) * 2 + 1]; }
    const double inv = 1.0 / sqrt((double)var[ch] + eps);
    const double sh = (cbias ? (double)cbias[ch] : 0.0) - (double)mean[ch];
    if (d_beta) d_beta[ch] = (float)s0;
    if (d_gamma) d_gamma[ch] = (float)((s1 + sh * s0) * inv);
    if (d_cbias) d_cbias[ch] = (float)((double)gamma[ch] * inv * s0);
}

// dz = s dy, s formed in f64 from the parameters, one rounding per element (dz may be dy).  grid (blocks, c, b)
__global__ __launch_bounds__(256) void k_eb_bn_scale(const float* dy, long long dybs, const float* __restrict__ gamma,
                                                     const float* __restrict__ var, double eps, int hw, float* dz, long long dzbs) {
    const int ch = blockIdx.y, bz = blockIdx.z;
    const double s = (double)gamma[ch] / sqrt((double)var[ch] + eps);
    const float* src = dy + (size_t)bz * dybs + (size_t)ch * hw;
    float* dst = dz + (size_t)bz * dzbs + (size_t)ch * hw;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) dst[p] = (float)(s * (double)src[p]);
}

// ------------------------------------------------------------------------------------------------------------ instance norm, adjoint
// y = (z - mean) / sigma per plane, sigma = sqrt(var + eps), var the biased variance; no affine parameters (raft._norm).  With
// xh = (z - mean) / sigma:  dz = (dy - mean(dy) - xh mean(dy xh)) / sigma.  One workgroup per plane: mean, then the centred second moment,
// then the two means of dy, each a pass over the plane summed in f64 (threads stride the plane, butterfly per wave, the waves in index
// order), then the pass that applies them.  A NaN stays inside its plane.  (dz may be dy or z.)
__device__ __forceinline__ double eb_block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void k_eb_instnorm_bwd(const float* dy, long long dybs, const float* z, long long zbs, int hw, double eps,
                                                         float* dz, long long dzbs) {
    __shared__ double red[4];
    const int ch = blockIdx.x, bz = blockIdx.y;
    const float* zp = z + (size_t)bz * zbs + (size_t)ch * hw;
    const float* dp = dy + (size_t)bz * dybs + (size_t)ch * hw;
    float* op = dz + (size_t)bz * dzbs + (size_t)ch * hw;
    const double n = (double)hw;
    double s = 0.0;
    for (int p = threadIdx.x; p < hw; p += 256) s += (double)zp[p];
    const double mean = eb_block_sum(s, red) / n;
    s = 0.0;
    for (int p = threadIdx.x; p < hw; p += 256) { const double d = (double)zp[p] - mean; s += d * d; }
    const double inv = 1.0 / sqrt(eb_block_sum(s, red) / n + eps);
    double s0 = 0.0, s1 = 0.0;
    for (int p = threadIdx.x; p < hw; p += 256) {
        const double d = (double)dp[p];
        s0 += d; s1 += d * (((double)zp[p] - mean) * inv);
    }
    const double m0 = eb_block_sum(s0, red) / n, m1 = eb_block_sum(s1, red) / n;
    for (int p = threadIdx.x; p < hw; p += 256) {
        const double xh = ((double)zp[p] - mean) * inv;
        op[p] = (float)(((double)dp[p] - m0 - xh * m1) * inv);
    }
}

// ------------------------------------------------------------------------------------------------------------ split activation, adjoint
// out = tanh on channels [0, half), ReLU on [half, c) (the context encoder as RAFT uses it); from the activated output ``act``:
// d (1 - act^2) in f64 with one rounding, resp. act > 0 ? d : 0.  grid (blocks, b); out may be grad.
__global__ __launch_bounds__(256) void k_eb_split_act_bwd(const float* grad, long long gbs, const float* __restrict__ act, long long abs_,
                                                          int half, int hw, size_t per, float* out, long long obs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const float g = grad[(size_t)bz * gbs + e], a = act[(size_t)bz * abs_ + e];
        const bool th = e < (size_t)half * hw;
        const float t = (float)((double)g * (1.0 - (double)a * (double)a));
        out[(size_t)bz * obs + e] = th ? t : (a > 0.0f ? g : 0.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- entry points
static inline bool eb_wshape_ok(int b, int cin, int cout, int hi, int wi, int ho, int wo, int k) {
    return b > 0 && cin > 0 && cout > 0 && eb_form_ok(k, hi, wi, ho, wo);
}
static inline size_t eb_wpart_bytes(int chunks, int cin, int cout, int k) {
    return ((size_t)chunks * cout * cin * k * k * sizeof(float) + 255) / 256 * 256;
}

// floats: partials (chunks, cout, cin, k, k), rounded up to 256 bytes | the workspace of the bias sum (rpe_conv_bwd_weight's own, on dy)
extern "C" size_t rpe_conv_s2_bwd_weight_workspace_bytes(int b, int cin, int cout, int hi, int wi, int ho, int wo, int k) {
    if (!eb_wshape_ok(b, cin, cout, hi, wi, ho, wo, k)) return 0;
    const size_t bias = rpe_conv_bwd_weight_workspace_bytes(b, 1, cout, ho, wo, 1, 1);
    return bias ? eb_wpart_bytes(eb_chunks((long long)b * ho * wo), cin, cout, k) + bias : 0;
}

extern "C" int rpe_conv_s2_bwd_weight(const float* x, long long x_batch_stride, const float* dy, long long dy_batch_stride, int b, int cin,
                                      int cout, int hi, int wi, int ho, int wo, int k, float scale, float* d_weight, float* d_bias,
                                      void* workspace, void* stream) {
    if (!x || !dy || !workspace || (!d_weight && !d_bias)) return RPE_E_BADARG;
    if (!eb_wshape_ok(b, cin, cout, hi, wi, ho, wo, k)) return RPE_E_BADARG;
    if (x_batch_stride < (long long)cin * hi * wi || dy_batch_stride < (long long)cout * ho * wo || !eb_aligned16(workspace)) return RPE_E_BADARG;
    const long long K = (long long)b * ho * wo, per = (long long)cout * cin * k * k;
    if (K >= (1LL << 31) || per >= (1LL << 31) || (long long)cin * hi * wi >= (1LL << 31) || (long long)cout * ho * wo >= (1LL << 31))
        return RPE_E_UNSUPPORTED;                                    // offsets inside a batch item and pixel indices are 32 bits
    const long long kc = eb_chunk(K);
    const int chunks = eb_chunks(K);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (d_weight) {
        const dim3 g(ceil_div((long long)cin * k * k, BW_BN), ceil_div(cout, BW_BM), chunks);
        if (g.y > 65535) return RPE_E_UNSUPPORTED;
        auto kernel = k == 3 ? k_eb_gemm_s2<3> : k == 1 ? k_eb_gemm_s2<1> : k_eb_gemm_s2<7>;
        hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, x, x_batch_stride, dy, dy_batch_stride, cin, cout, hi, wi, ho, wo, K, kc, part);
        splitk_reduce_launch(part, 1, chunks, per, (double)scale, d_weight, s);
        if (rpe_check_launch() != RPE_OK) return RPE_E_LAUNCH;
    }
    if (d_bias)                                                      // dy's channel sums do not see the stride: the stride-1 path's bias pass
        return rpe_conv_bwd_weight(dy, dy_batch_stride, dy, dy_batch_stride, b, 1, cout, ho, wo, 1, 1, scale, nullptr, d_bias,
                                   (char*)workspace + eb_wpart_bytes(chunks, cin, cout, k), stream);
    return RPE_OK;
}

extern "C" int rpe_conv_s2_bwd_data(const float* dy, long long dy_batch_stride, const float* weight, int b, int cin, int cout, int hi, int wi,
                                    int ho, int wo, int k, float* dx, long long dx_batch_stride, void* stream) {
    if (!dy || !weight || !dx || b < 0 || b > 65535 || cin <= 0 || cin > 65535 || cout <= 0) return RPE_E_BADARG;
    if ((k != 1 && k != 3) || !eb_form_ok(k, hi, wi, ho, wo)) return RPE_E_BADARG;      // (the stem has no data gradient: images are not trained)
    if (dy_batch_stride < (long long)cout * ho * wo || dx_batch_stride < (long long)cin * hi * wi) return RPE_E_BADARG;
    if ((long long)cin * hi * wi >= (1LL << 31) || (long long)cout * ho * wo >= (1LL << 31) || (long long)cout * cin * k * k >= (1LL << 31))
        return RPE_E_UNSUPPORTED;
    if (b == 0) return RPE_OK;
    const dim3 g(ceil_div((long long)hi * wi, 256), cin, b);
    hipLaunchKernelGGL(k == 3 ? k_eb_s2_bwd_data<3> : k_eb_s2_bwd_data<1>, g, dim3(256), 0, (hipStream_t)stream, dy, dy_batch_stride, weight,
                       cin, cout, hi, wi, ho, wo, dx, dx_batch_stride);
    return rpe_check_launch();
}

// doubles: the chunks' partial sums (chunks, c, 2)
extern "C" size_t rpe_bn_frozen_backward_workspace_bytes(int b, int c, int hw) {
    if (b <= 0 || c <= 0 || hw <= 0) return 0;
    return ((size_t)eb_chunks((long long)b * hw) * c * 2 * sizeof(double) + 255) / 256 * 256;
}

extern "C" int rpe_bn_frozen_backward(const float* dy, long long dy_batch_stride, const float* z, long long z_batch_stride, const float* gamma,
                                      const float* conv_bias, const float* mean, const float* var, double eps, int b, int c, int hw,
                                      float* d_gamma, float* d_beta, float* d_conv_bias, float* dz, long long dz_batch_stride,
                                      void* workspace, void* stream) {
    if (!dy || !z || !gamma || !mean || !var || !workspace || b <= 0 || b > 65535 || c <= 0 || c > 65535 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw, K = (long long)b * hw;
    if (dy_batch_stride < per || z_batch_stride < per || (dz && dz_batch_stride < per) || !eb_aligned16(workspace) || !(eps >= 0.0))
        return RPE_E_BADARG;
    if (per >= (1LL << 31) || K >= (1LL << 31)) return RPE_E_UNSUPPORTED;
    const long long kc = eb_chunk(K);
    const int chunks = eb_chunks(K);
    hipStream_t s = (hipStream_t)stream;
    if (d_gamma || d_beta || d_conv_bias) {
        hipLaunchKernelGGL(k_eb_bn_part, dim3(c, chunks), dim3(256), 0, s, dy, dy_batch_stride, z, z_batch_stride, c, hw, K, kc, (double*)workspace);
        hipLaunchKernelGGL(k_eb_bn_final, dim3(ceil_div(c, 256)), dim3(256), 0, s, (const double*)workspace, chunks, c, gamma, conv_bias, mean,
                           var, eps, d_gamma, d_beta, d_conv_bias);
    }
    if (dz)
        hipLaunchKernelGGL(k_eb_bn_scale, dim3(min(ceil_div(hw, 256), 64), c, b), dim3(256), 0, s, dy, dy_batch_stride, gamma, var, eps, hw, dz,
                           dz_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_instnorm_backward(const float* dy, long long dy_batch_stride, const float* z, long long z_batch_stride, int b, int c, int hw,
                                     double eps, float* dz, long long dz_batch_stride, void* stream) {
    if (!dy || !z || !dz || b < 0 || b > 65535 || c <= 0 || hw <= 0 || !(eps >= 0.0)) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (dy_batch_stride < per || z_batch_stride < per || dz_batch_stride < per) return RPE_E_BADARG;
    if (per >= (1LL << 31)) return RPE_E_UNSUPPORTED;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_eb_instnorm_bwd, dim3(c, b), dim3(256), 0, (hipStream_t)stream, dy, dy_batch_stride, z, z_batch_stride, hw, eps, dz,
                       dz_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_split_act_backward(const float* grad, long long grad_batch_stride, const float* act, long long act_batch_stride, int b, int c,
                                      int half, int hw, float* out, long long out_batch_stride, void* stream) {
    if (!grad || !act || !out || b < 0 || b > 65535 || c <= 0 || hw <= 0 || half < 0 || half > c) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (grad_batch_stride < per || act_batch_stride < per || out_batch_stride < per) return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_eb_split_act_bwd, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, grad, grad_batch_stride,
                       act, act_batch_stride, half, hw, (size_t)per, out, out_batch_stride);
    return rpe_check_launch();
}
