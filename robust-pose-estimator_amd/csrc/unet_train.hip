// Training route of one TinyUNet weight head: forward (keeping what the backward needs) and backward, one plain kernel per
// operation -- the other half of csrc/unet.hip, which runs the same architecture with frozen, folded norms.
//
// Replaces (reference): core/unet/unet.py:7-82 under autograd while scripts/train_posenet.py trains the two heads with the flow
// network frozen: F.conv2d / F.batch_norm / F.max_pool2d / F.conv_transpose2d / F.interpolate and their library backward kernels.
//
// Everything is f32 NCHW in torch's own parameter layouts (no packing: the pointers are read from the modules per call), order
// and workspace plan in unet_train_host.h.  The maps are tiny (44x44 .. 80x64 at 1/8 scale, 16/32/64 channels), so these are direct
// kernels written for correctness: every long sum (the convolutions' 9 cin terms, the weight gradients' n h w pixels, the norm
// statistics) is accumulated in f64 and rounded to f32 once, and every reduction runs in a fixed order -- per-thread strided sums,
// a butterfly per wave, the waves and then the per-block partials added in index order.  No float atomics anywhere: two runs agree
// bit for bit, and nothing but the batch statistics and the parameter gradients of a row depends on the batch it is launched in.
#include "rpe_common.h"
#include "unet_train_host.h"

#define TCT 8                 // channels per thread of the convolution kernels (every channel count of the architecture is a multiple)
#define TCK 8                 // channels of the summed axis staged in LDS at a time

struct TSrc { const float* p; long long bs; int c, h, w, oy, ox; };         // (n, c, h, w) read at (y + oy, x + ox)

// sum over the workgroup (256 threads), every thread gets it; fixed order
__device__ __forceinline__ double block_sum(double v, double* sm) {
    v = wave_sum(v);
    __syncthreads();                                               // (sm may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// ------------------------------------------------------------------------------------------------ 3x3 valid convolution
struct TConvP { TSrc src[4]; int nsrc, cin; const float* w; const float* bias; float* out; int cout, ho, wo, relu; };

// thread = output pixel x TCT output channels; the input is the channel concatenation of the sources (never materialised)
__global__ __launch_bounds__(256) void k_t_conv3(TConvP P) {
    __shared__ double wsm[TCK * 9 * TCT];                          // [ci][tap][co]
    const int bz = blockIdx.z, co0 = blockIdx.y * TCT, tid = threadIdx.x;
    const int npix = P.ho * P.wo, p = blockIdx.x * 256 + tid;
    const bool ok = p < npix;
    const int y = ok ? p / P.wo : 0, x = ok ? p - (p / P.wo) * P.wo : 0;
    double acc[TCT];
#pragma unroll
    for (int j = 0; j < TCT; ++j) acc[j] = 0.0;
    int cbase = 0;
    for (int s = 0; s < P.nsrc; ++s) {
        const TSrc S = P.src[s];
        const float* base = S.p + (size_t)bz * S.bs + (size_t)(y + S.oy) * S.w + (x + S.ox);
        const size_t plane = (size_t)S.h * S.w;
        for (int ci0 = 0; ci0 < S.c; ci0 += TCK) {
            __syncthreads();
            for (int e = tid; e < TCK * 9 * TCT; e += 256) {
                const int cl = e / (9 * TCT), r = e - cl * 9 * TCT, t = r / TCT, j = r - t * TCT;
                wsm[e] = (double)P.w[((size_t)(co0 + j) * P.cin + cbase + ci0 + cl) * 9 + t];
            }
            __syncthreads();
#pragma unroll 2
            for (int c = 0; c < TCK; ++c) {
                const float* ip = base + (size_t)(ci0 + c) * plane;
                float v[9];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) v[dy * 3 + dx] = ip[dy * S.w + dx];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const double dv = (double)v[t];
#pragma unroll
                    for (int j = 0; j < TCT; ++j) acc[j] = fma(dv, wsm[(c * 9 + t) * TCT + j], acc[j]);
                }
            }
        }
        cbase += S.c;
    }
    if (!ok) return;
    float* o = P.out + ((size_t)bz * P.cout + co0) * npix + p;
#pragma unroll
    for (int j = 0; j < TCT; ++j) {
        float v = (float)(acc[j] + (P.bias ? (double)P.bias[co0 + j] : 0.0));
        if (P.relu) v = (v > 0.0f || v != v) ? v : 0.0f;               // NaN stays NaN, as in torch.relu
        o[(size_t)j * npix] = v;
    }
}

// data gradient: the full correlation of dy (n, cout, ho, wo) with the flipped kernel, for input channels [ci_begin, ci_begin + ci_n),
// written to dst (n, ci_n, dst_h, dst_w) whose (oy, ox) is the convolution input's (0, 0): zero outside the input (the centre crop).
struct TConvBdP { const float* dy; const float* w; float* dst; int cout, cin, ci_begin, ci_n, ho, wo, dst_h, dst_w, oy, ox; };

__global__ __launch_bounds__(256) void k_t_conv3_bwd_data(TConvBdP P) {
    __shared__ double wsm[TCK * TCT * 9];                          // [co][ci][tap]
    const int bz = blockIdx.z, cig = blockIdx.y * TCT, tid = threadIdx.x;
    const int npix = P.dst_h * P.dst_w, p = blockIdx.x * 256 + tid;
    const bool ok = p < npix;
    const int Y = ok ? p / P.dst_w : 0, X = ok ? p - (p / P.dst_w) * P.dst_w : 0;
    const int yi = Y - P.oy, xi = X - P.ox;
    const bool inside = ok && yi >= 0 && yi < P.ho + 2 && xi >= 0 && xi < P.wo + 2;
    bool tap_ok[9]; int tap_off[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = yi - ky, xx = xi - kx;
            const bool v = inside && yy >= 0 && yy < P.ho && xx >= 0 && xx < P.wo;
            tap_ok[ky * 3 + kx] = v; tap_off[ky * 3 + kx] = v ? yy * P.wo + xx : 0;
        }
    double acc[TCT];
#pragma unroll
    for (int j = 0; j < TCT; ++j) acc[j] = 0.0;
    const size_t oplane = (size_t)P.ho * P.wo;
    const float* dyb = P.dy + (size_t)bz * P.cout * oplane;
    for (int co0 = 0; co0 < P.cout; co0 += TCK) {
        __syncthreads();
        for (int e = tid; e < TCK * TCT * 9; e += 256) {
            const int col = e / (TCT * 9), r = e - col * TCT * 9;   // r = j * 9 + t: contiguous in torch's (cout, cin, 3, 3)
            wsm[e] = (double)P.w[((size_t)(co0 + col) * P.cin + P.ci_begin + cig) * 9 + r];
        }
        __syncthreads();
#pragma unroll 1
        for (int col = 0; col < TCK; ++col) {
            const float* dp = dyb + (size_t)(co0 + col) * oplane;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const double dv = tap_ok[t] ? (double)dp[tap_off[t]] : 0.0;
#pragma unroll
                for (int j = 0; j < TCT; ++j) acc[j] = fma(dv, wsm[(col * TCT + j) * 9 + t], acc[j]);
            }
        }
    }
    if (!ok) return;
    float* o = P.dst + ((size_t)bz * P.ci_n + cig) * npix + p;
#pragma unroll
    for (int j = 0; j < TCT; ++j) o[(size_t)j * npix] = inside ? (float)acc[j] : 0.0f;
}

// weight gradient, stage 1: workgroup = (input channel, 4 output channels, chunk of the n ho wo pixels) -> one f64 partial of the 4 x 9 weights
#define TWC 4
struct TConvBwP { TSrc src[4]; int nsrc, cin; const float* dy; double* part; int cout, ho, wo, n, chunk; };

__global__ __launch_bounds__(256) void k_t_conv3_bwd_weight(TConvBwP P) {
    __shared__ double sm[4][TWC * 9];
    const int ci = blockIdx.x, co0 = blockIdx.y * TWC, tid = threadIdx.x;
    int s = 0, cl = ci;
    while (s + 1 < P.nsrc && cl >= P.src[s].c) { cl -= P.src[s].c; ++s; }        // (workgroup-uniform)
    const TSrc S = P.src[s];
    const int npix = P.ho * P.wo;
    const long long total = (long long)P.n * npix;
    const long long q0 = (long long)blockIdx.z * P.chunk;
    const long long q1 = q0 + P.chunk < total ? q0 + P.chunk : total;
    double acc[TWC][9];
#pragma unroll
    for (int j = 0; j < TWC; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[j][t] = 0.0;
    for (long long q = q0 + tid; q < q1; q += 256) {
        const int b = (int)(q / npix), p = (int)(q - (long long)b * npix);
        const int y = p / P.wo, x = p - y * P.wo;
        const float* ip = S.p + (size_t)b * S.bs + (size_t)cl * S.h * S.w + (size_t)(y + S.oy) * S.w + (x + S.ox);
        double v[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) v[dy * 3 + dx] = (double)ip[dy * S.w + dx];
        const float* gp = P.dy + ((size_t)b * P.cout + co0) * npix + p;
#pragma unroll
        for (int j = 0; j < TWC; ++j) {
            const double g = (double)gp[(size_t)j * npix];
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[j][t] = fma(g, v[t], acc[j][t]);
        }
    }
#pragma unroll
    for (int j = 0; j < TWC; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const double r = wave_sum(acc[j][t]);
            if ((tid & 63) == 0) sm[tid >> 6][j * 9 + t] = r;
        }
    __syncthreads();
    if (tid < TWC * 9) {
        const int j = tid / 9, t = tid - j * 9;
        const double r = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
        P.part[(size_t)blockIdx.z * P.cout * P.cin * 9 + ((size_t)(co0 + j) * P.cin + ci) * 9 + t] = r;
    }
}

// stage 2 of every partial reduction: out[e] = sum over the partials in index order
__global__ void k_t_sum_partials(const double* __restrict__ part, int nparts, long long count, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    double a = 0.0;
    for (int z = 0; z < nparts; ++z) a += part[(size_t)z * count + e];
    out[e] = (float)a;
}

// out[c] = sum over (n, h w) of g (n, C, hw): the bias gradients.  One workgroup per channel.
__global__ __launch_bounds__(256) void k_t_chan_sum(const float* __restrict__ g, int n, int C, int hw, float* __restrict__ out) {
    __shared__ double sm[4];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int b = 0; b < n; ++b) {
        const float* p = g + ((size_t)b * C + c) * hw;
        for (int i = threadIdx.x; i < hw; i += 256) a += (double)p[i];
    }
    a = block_sum(a, sm);
    if (threadIdx.x == 0) out[c] = (float)a;
}

// ------------------------------------------------------------------------------------------------ batch norm
// One workgroup per channel.  train: mean and biased variance of x over (n, h w) (two passes, f64), the running statistics updated as
// F.batch_norm(training=True) does (momentum, unbiased variance; channel 0 counts the batch).  Otherwise the running statistics.
// Either way mean / invstd are saved for the apply pass and the backward.
__global__ __launch_bounds__(256) void k_t_bn_stats(const float* __restrict__ x, int n, int C, int hw, float eps, float momentum, int train,
                                                    float* running_mean, float* running_var, long long* num_batches_tracked,
                                                    float* __restrict__ mean_out, float* __restrict__ invstd_out) {
    __shared__ double sm[4];
    const int c = blockIdx.x;
    if (!train) {
        if (threadIdx.x == 0) { mean_out[c] = running_mean[c]; invstd_out[c] = (float)(1.0 / sqrt((double)running_var[c] + (double)eps)); }
        return;
    }
    const double cnt = (double)n * hw;
    double a = 0.0;
    for (int b = 0; b < n; ++b) {
        const float* p = x + ((size_t)b * C + c) * hw;
        for (int i = threadIdx.x; i < hw; i += 256) a += (double)p[i];
    }
    const double mean = block_sum(a, sm) / cnt;
    a = 0.0;
    for (int b = 0; b < n; ++b) {
        const float* p = x + ((size_t)b * C + c) * hw;
        for (int i = threadIdx.x; i < hw; i += 256) { const double d = (double)p[i] - mean; a = fma(d, d, a); }
    }
    const double m2 = block_sum(a, sm);
    if (threadIdx.x == 0) {
        const double var = m2 / cnt;
        mean_out[c] = (float)mean; invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) {
            const double m = (double)momentum;
            running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
            running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (m2 / (cnt - 1.0)));
            if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
        }
    }
}

// y = (x - mean) * invstd * gamma + beta, [ReLU]
__global__ void k_t_bn_apply(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                             const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out, int C, int hw,
                             long long total, int relu) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)((e / hw) % C);
    float v = fmaf(rn_mul(rn_sub(x[e], mean[c]), invstd[c]), gamma[c], beta[c]);
    if (relu) v = (v > 0.0f || v != v) ? v : 0.0f;                       // NaN stays NaN, as in torch.relu
    out[e] = v;
}

// dgamma[c] = sum dy xhat, dbeta[c] = sum dy over (n, h w); dy is masked by (relu_out > 0) when the norm feeds a ReLU (encoder stages)
__global__ __launch_bounds__(256) void k_t_bn_bwd_reduce(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ relu_out,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd, int n, int C, int hw,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sm[4];
    const int c = blockIdx.x;
    const double mu = (double)mean[c], is = (double)invstd[c];
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < n; ++b) {
        const size_t o = ((size_t)b * C + c) * hw;
        for (int i = threadIdx.x; i < hw; i += 256) {
            double g = (double)dy[o + i];
            if (relu_out && !(relu_out[o + i] > 0.0f)) g = 0.0;
            s1 += g; s2 = fma(g, ((double)x[o + i] - mu) * is, s2);
        }
    }
    s1 = block_sum(s1, sm); s2 = block_sum(s2, sm);
    if (threadIdx.x == 0) { dbeta[c] = (float)s1; dgamma[c] = (float)s2; }
}

// dx in place of dy.  train: gamma invstd (dy - mean(dy) - xhat mean(dy xhat)); frozen: gamma invstd dy.  post_mask: the norm's input is a
// ReLU output (decoder stages), whose gradient is passed on to the convolution in front of it: zero where x <= 0.
__global__ void k_t_bn_bwd_dx(float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ relu_out, const float* __restrict__ mean,
                              const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ dgamma,
                              const float* __restrict__ dbeta, int n, int C, int hw, long long total, int train, int post_mask) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)((e / hw) % C);
    float g = dy[e];
    if (relu_out && !(relu_out[e] > 0.0f)) g = 0.0f;
    const float xv = x[e];
    const double gi = (double)gamma[c] * (double)invstd[c];
    float d;
    if (train) {                                                 // in f64, rounded once: sums of dx over a channel vanish, and should in f32 too
        const double inv_cnt = 1.0 / ((double)n * (double)hw);
        const double xhat = ((double)xv - (double)mean[c]) * (double)invstd[c];
        d = (float)(gi * (((double)g - (double)dbeta[c] * inv_cnt) - xhat * ((double)dgamma[c] * inv_cnt)));
    } else {
        d = (float)((double)g * gi);
    }
    if (post_mask && !(xv > 0.0f)) d = 0.0f;
    dy[e] = d;
}

// ------------------------------------------------------------------------------------------------ 2x2 max pool
__global__ void k_t_pool(const float* __restrict__ in, float* __restrict__ out, int h, int w, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int ho = h / 2, wo = w / 2;
    const int x = (int)(e % wo), y = (int)((e / wo) % ho);
    const long long pl = e / ((long long)wo * ho);
    const float* s = in + pl * h * w + (size_t)(2 * y) * w + 2 * x;
    out[e] = pool_max4(s[0], s[1], s[w], s[w + 1]);
}

// routing, as a gather: thread = pixel of the pooled map's input; it takes its window's gradient if it is the window's first maximum in
// row-major order (torch's tie rule; recomputed from the saved maps) and ADDS it to dskip, which already holds the skip connection's share
__global__ void k_t_pool_bwd_add(const float* __restrict__ in, const float* __restrict__ pooled, const float* __restrict__ dpool,
                                 float* __restrict__ dskip, int h, int w, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int ho = h / 2, wo = w / 2;
    const int x = (int)(e % w), y = (int)((e / w) % h);
    const long long pl = e / ((long long)w * h);
    const int py = y >> 1, px = x >> 1;
    if (py >= ho || px >= wo) return;                            // the odd last row / column is pooled by nothing
    const float* s = in + pl * h * w + (size_t)(2 * py) * w + 2 * px;
    const size_t po = (size_t)pl * ho * wo + (size_t)py * wo + px;
    const float m = pooled[po];
    const int first = s[0] == m ? 0 : s[1] == m ? 1 : s[w] == m ? 2 : 3;
    if (first == (y & 1) * 2 + (x & 1)) dskip[e] += dpool[po];
}

// ------------------------------------------------------------------------------------------------ 2x2 stride-2 transposed convolution
// w (cin, cout, 2, 2).  forward: thread = output pixel x TCT output channels
__global__ __launch_bounds__(256) void k_t_upconv(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ out, int cin, int cout, int h, int wd) {
    const int bz = blockIdx.z, co0 = blockIdx.y * TCT;
    const int ho = 2 * h, wo = 2 * wd, npo = ho * wo, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npo) return;
    const int Y = p / wo, X = p - Y * wo, tap = (Y & 1) * 2 + (X & 1);
    const float* ip = in + (size_t)bz * cin * h * wd + (size_t)(Y >> 1) * wd + (X >> 1);
    double acc[TCT];
#pragma unroll
    for (int j = 0; j < TCT; ++j) acc[j] = 0.0;
    for (int ci = 0; ci < cin; ++ci) {
        const double v = (double)ip[(size_t)ci * h * wd];
        const float* wp = w + ((size_t)ci * cout + co0) * 4 + tap;
#pragma unroll
        for (int j = 0; j < TCT; ++j) acc[j] = fma(v, (double)wp[j * 4], acc[j]);
    }
    float* o = out + ((size_t)bz * cout + co0) * npo + p;
#pragma unroll
    for (int j = 0; j < TCT; ++j) o[(size_t)j * npo] = (float)(acc[j] + (double)bias[co0 + j]);
}

// data gradient: thread = input pixel x TCT input channels, over its 2x2 output pixels and every output channel
__global__ __launch_bounds__(256) void k_t_upconv_bwd_data(const float* __restrict__ dout, const float* __restrict__ w, float* __restrict__ din,
                                                           int cin, int cout, int h, int wd) {
    const int bz = blockIdx.z, ci0 = blockIdx.y * TCT;
    const int npi = h * wd, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npi) return;
    const int y = p / wd, x = p - y * wd, wo = 2 * wd;
    const size_t opl = (size_t)4 * npi;
    const float* gp = dout + (size_t)bz * cout * opl + (size_t)(2 * y) * wo + 2 * x;
    double acc[TCT];
#pragma unroll
    for (int j = 0; j < TCT; ++j) acc[j] = 0.0;
    for (int co = 0; co < cout; ++co) {
        const float* q = gp + (size_t)co * opl;
        const double g[4] = {(double)q[0], (double)q[1], (double)q[wo], (double)q[wo + 1]};
#pragma unroll
        for (int j = 0; j < TCT; ++j) {
            const float* wp = w + ((size_t)(ci0 + j) * cout + co) * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[j] = fma(g[t], (double)wp[t], acc[j]);
        }
    }
    float* o = din + ((size_t)bz * cin + ci0) * npi + p;
#pragma unroll
    for (int j = 0; j < TCT; ++j) o[(size_t)j * npi] = (float)acc[j];
}

// weight gradient: one workgroup per (ci, co) -> its four taps over every (n, y, x)
__global__ __launch_bounds__(256) void k_t_upconv_bwd_weight(const float* __restrict__ in, const float* __restrict__ dout, float* __restrict__ dw,
                                                             int n, int cin, int cout, int h, int wd) {
    __shared__ double sm[4];
    const int ci = blockIdx.x, co = blockIdx.y;
    const int npi = h * wd, wo = 2 * wd;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < n; ++b) {
        const float* ip = in + ((size_t)b * cin + ci) * npi;
        const float* gp = dout + ((size_t)b * cout + co) * 4 * npi;
        for (int p = threadIdx.x; p < npi; p += 256) {
            const int y = p / wd, x = p - y * wd;
            const double v = (double)ip[p];
            const float* q = gp + (size_t)(2 * y) * wo + 2 * x;
            acc[0] = fma(v, (double)q[0], acc[0]); acc[1] = fma(v, (double)q[1], acc[1]);
            acc[2] = fma(v, (double)q[wo], acc[2]); acc[3] = fma(v, (double)q[wo + 1], acc[3]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double r = block_sum(acc[t], sm);
        if (threadIdx.x == 0) dw[((size_t)ci * cout + co) * 4 + t] = (float)r;
    }
}

// ------------------------------------------------------------------------------------------------ 1x1 head (16 -> 1)
__global__ void k_t_head(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int npix) {
    const int bz = blockIdx.z, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float* ip = in + (size_t)bz * 16 * npix + p;
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a = fma((double)ip[(size_t)c * npix], (double)w[c], a);
    out[(size_t)bz * npix + p] = (float)(a + (double)bias[0]);
}

__global__ void k_t_head_bwd_data(const float* __restrict__ dhm, const float* __restrict__ w, float* __restrict__ din, int npix) {
    const int bz = blockIdx.z, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float g = dhm[(size_t)bz * npix + p];
#pragma unroll
    for (int c = 0; c < 16; ++c) din[((size_t)bz * 16 + c) * npix + p] = rn_mul(g, w[c]);
}

// workgroup c < 16: dw[c] = sum dhm x[c]; workgroup 16: db = sum dhm
__global__ __launch_bounds__(256) void k_t_head_bwd_weight(const float* __restrict__ in, const float* __restrict__ dhm, int n, int npix,
                                                           float* __restrict__ dw, float* __restrict__ db) {
    __shared__ double sm[4];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int b = 0; b < n; ++b) {
        const float* g = dhm + (size_t)b * npix;
        const float* ip = in + ((size_t)b * 16 + (c < 16 ? c : 0)) * npix;
        for (int p = threadIdx.x; p < npix; p += 256) a = c < 16 ? fma((double)g[p], (double)ip[p], a) : a + (double)g[p];
    }
    a = block_sum(a, sm);
    if (threadIdx.x == 0) { if (c < 16) dw[c] = (float)a; else db[0] = (float)a; }
}

// ------------------------------------------------------------------------------------------------ bilinear resize (align_corners=False) [+ sigmoid]
// the tap arithmetic of csrc/unet.hip's k_u_resize_sigmoid (torch's area_pixel_compute_source_index in float)
struct TTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ TTap t_tap(float scale, int o, int n_in) {
    float f = rn_sub(rn_mul(scale, rn_add((float)o, 0.5f)), 0.5f);
    f = f < 0.0f ? 0.0f : f;
    TTap t;
    t.i0 = (int)f; t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = f - (float)t.i0; t.l0 = 1.0f - t.l1;
    return t;
}

__global__ void k_t_resize(const float* __restrict__ in, float* __restrict__ out, int h, int w, int H, int W, float sy, float sx, int sigmoid) {
    const int bz = blockIdx.z;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)H * W) return;
    const int oy = (int)(e / W), ox = (int)(e - (long long)oy * W);
    const TTap ty = t_tap(sy, oy, h), tx = t_tap(sx, ox, w);
    const float* s = in + (size_t)bz * h * w;
    const float v = ty.l0 * (tx.l0 * s[ty.i0 * w + tx.i0] + tx.l1 * s[ty.i0 * w + tx.i1]) + ty.l1 * (tx.l0 * s[ty.i1 * w + tx.i0] + tx.l1 * s[ty.i1 * w + tx.i1]);
    out[(size_t)bz * H * W + e] = sigmoid ? 1.0f / (1.0f + expf(-v)) : v;
}

// backward as a gather: one wave per source pixel, its lanes stride over the window of output pixels that can read it (a conservative
// window; each output pixel's taps are recomputed exactly as the forward did), then a butterfly.  With sigmoid: g y (1 - y) on the way in.
__global__ __launch_bounds__(256) void k_t_resize_bwd(const float* __restrict__ gout, const float* __restrict__ yout, float* __restrict__ dhm,
                                                      int n, int h, int w, int H, int W, float sy, float sx, int sigmoid) {
    const long long src = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (src >= (long long)n * h * w) return;                     // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int bz = (int)(src / (h * w)), r = (int)(src - (long long)bz * h * w), ys = r / w, xs = r - ys * w;
    // output rows with floor(f) in {ys - 1, ys}: f in [ys - 1, ys + 1)  ->  o + 0.5 in [(ys - 0.5) / sy, (ys + 1.5) / sy); two pixels of slack
    int y_lo = (int)floorf(((float)ys - 0.5f) / sy - 0.5f) - 2, y_hi = (int)ceilf(((float)ys + 1.5f) / sy - 0.5f) + 2;
    int x_lo = (int)floorf(((float)xs - 0.5f) / sx - 0.5f) - 2, x_hi = (int)ceilf(((float)xs + 1.5f) / sx - 0.5f) + 2;
    y_lo = y_lo < 0 ? 0 : y_lo; x_lo = x_lo < 0 ? 0 : x_lo;
    y_hi = y_hi > H - 1 ? H - 1 : y_hi; x_hi = x_hi > W - 1 ? W - 1 : x_hi;
    const int wy = y_hi - y_lo + 1, wx = x_hi - x_lo + 1;
    double a = 0.0;
    if (wy > 0 && wx > 0) {
        const float* g = gout + (size_t)bz * H * W;
        const float* yo = yout ? yout + (size_t)bz * H * W : nullptr;
        for (int i = lane; i < wy * wx; i += 64) {
            const int oy = y_lo + i / wx, ox = x_lo + i % wx;
            const TTap ty = t_tap(sy, oy, h), tx = t_tap(sx, ox, w);
            const float cy = (ty.i0 == ys ? ty.l0 : 0.0f) + (ty.i1 == ys ? ty.l1 : 0.0f);
            const float cx = (tx.i0 == xs ? tx.l0 : 0.0f) + (tx.i1 == xs ? tx.l1 : 0.0f);
            if (cy != 0.0f && cx != 0.0f) {
                float gv = g[(size_t)oy * W + ox];
                if (sigmoid) { const float yv = yo[(size_t)oy * W + ox]; gv = gv * yv * (1.0f - yv); }
                a = fma((double)gv, (double)cy * (double)cx, a);
            }
        }
    }
    a = wave_sum(a);
    if (lane == 0) dhm[src] = (float)a;
}

// ------------------------------------------------------------------------------------------------ host side
extern "C" size_t rpe_unet_train_workspace_bytes(int n, int cin, int h8, int w8, int out_h, int out_w) {
    if (out_h <= 0 || out_w <= 0) return 0;
    return ut_workspace_bytes(n, cin, h8, w8);
}

extern "C" size_t rpe_unet_train_grad_floats(int cin) { return cin > 0 && cin % 8 == 0 ? ut_grad_offset(cin, UT_NPARAM) : 0; }

extern "C" size_t rpe_unet_train_grad_offset(int cin, int index) {
    return cin > 0 && cin % 8 == 0 && index >= 0 && index <= UT_NPARAM ? ut_grad_offset(cin, index) : 0;
}

extern "C" size_t rpe_unet_train_workspace_offset(int n, int cin, int h8, int w8, int index) {
    UtBuf b;
    return ut_workspace_buffer(n, cin, h8, w8, index, b) ? b.off : (size_t)-1;
}

extern "C" int rpe_unet_train_workspace_extent(int n, int cin, int h8, int w8, int index, int* extent) {
    UtBuf b;
    if (!extent) return RPE_E_BADARG;
    if (!ut_workspace_buffer(n, cin, h8, w8, index, b)) return index < 0 || index >= UT_NBUF ? RPE_E_BADARG : RPE_E_UNSUPPORTED;
    extent[0] = b.rows; extent[1] = b.c; extent[2] = b.h; extent[3] = b.w;
    return RPE_OK;
}

namespace {
struct TCall {                      // what forward and backward share: checked arguments, the geometry and the workspace plan
    UtGeo g; UtPlan pl; float* ws; TSrc in[4]; int nsrc, cin, n, h8, w8; const float* const* prm; hipStream_t s;
    float* at(size_t off) const { return ws + off; }
};

int t_setup(TCall& C, const float* const* src, const int* src_channels, const long long* src_bs, int nsrc, const float* const* params,
            int n, int h8, int w8, int out_h, int out_w, void* workspace, void* stream) {
    if (!src || !src_channels || !src_bs || !params || !workspace || nsrc < 1 || nsrc > 4 || n <= 0 || out_h <= 0 || out_w <= 0) return RPE_E_BADARG;
    int cin = 0;
    for (int k = 0; k < nsrc; ++k) {
        if (!src[k] || src_channels[k] <= 0 || src_bs[k] < (long long)src_channels[k] * h8 * w8) return RPE_E_BADARG;
        if (src_channels[k] % TCK != 0) return RPE_E_UNSUPPORTED;
        C.in[k] = TSrc{src[k], src_bs[k], src_channels[k], h8, w8, 0, 0};
        cin += src_channels[k];
    }
    for (int k = 0; k < UT_NPARAM; ++k) if (!params[k]) return RPE_E_BADARG;
    if (!ut_geo(h8, w8, C.g)) return RPE_E_UNSUPPORTED;
    ut_plan(C.g, n, cin, C.pl);
    C.ws = (float*)(((uintptr_t)workspace + 255) / 256 * 256);
    C.nsrc = nsrc; C.cin = cin; C.n = n; C.h8 = h8; C.w8 = w8; C.prm = params; C.s = (hipStream_t)stream;
    return RPE_OK;
}

TSrc t_map(const float* p, int c, int h, int w, int oy = 0, int ox = 0) { return TSrc{p, (long long)c * h * w, c, h, w, oy, ox}; }

void t_conv3(const TCall& C, const TSrc* src, int nsrc, int cin, const float* w, const float* bias, float* out, int cout, int ho, int wo, int relu) {
    TConvP P{};
    for (int k = 0; k < nsrc; ++k) P.src[k] = src[k];
    P.nsrc = nsrc; P.cin = cin; P.w = w; P.bias = bias; P.out = out; P.cout = cout; P.ho = ho; P.wo = wo; P.relu = relu;
    hipLaunchKernelGGL(k_t_conv3, dim3(ceil_div(ho * wo, 256), cout / TCT, C.n), dim3(256), 0, C.s, P);
}

void t_conv3_bwd_data(const TCall& C, const float* dy, const float* w, float* dst, int cout, int cin, int ci_begin, int ci_n, int ho, int wo,
                      int dst_h, int dst_w, int oy, int ox) {
    TConvBdP P{dy, w, dst, cout, cin, ci_begin, ci_n, ho, wo, dst_h, dst_w, oy, ox};
    hipLaunchKernelGGL(k_t_conv3_bwd_data, dim3(ceil_div(dst_h * dst_w, 256), ci_n / TCT, C.n), dim3(256), 0, C.s, P);
}

// weight and bias gradient of a 3x3 convolution whose input was the concatenation of src and whose output gradient is dy
void t_conv3_bwd_wb(const TCall& C, const TSrc* src, int nsrc, int cin, const float* dy, int cout, int ho, int wo, float* dw, float* db) {
    TConvBwP P{};
    for (int k = 0; k < nsrc; ++k) P.src[k] = src[k];
    int nchunk;
    ut_wchunks((long long)C.n * ho * wo, P.chunk, nchunk);
    P.nsrc = nsrc; P.cin = cin; P.dy = dy; P.part = (double*)C.at(C.pl.wpart); P.cout = cout; P.ho = ho; P.wo = wo; P.n = C.n;
    hipLaunchKernelGGL(k_t_conv3_bwd_weight, dim3(cin, cout / TWC, nchunk), dim3(256), 0, C.s, P);
    const long long count = (long long)cout * cin * 9;
    hipLaunchKernelGGL(k_t_sum_partials, dim3(ceil_div(count, 256)), dim3(256), 0, C.s, (const double*)P.part, nchunk, count, dw);
    hipLaunchKernelGGL(k_t_chan_sum, dim3(cout), dim3(256), 0, C.s, dy, C.n, cout, ho * wo, db);
}

void t_bn_bwd(const TCall& C, float* dy, const float* x, const float* relu_out, int norm, int c, int hw, const float* gamma, float* dgamma, float* dbeta,
              int train, int post_mask) {
    const float* mean = C.at(C.pl.mean[norm]); const float* invstd = C.at(C.pl.invstd[norm]);
    hipLaunchKernelGGL(k_t_bn_bwd_reduce, dim3(c), dim3(256), 0, C.s, (const float*)dy, x, relu_out, mean, invstd, C.n, c, hw, dgamma, dbeta);
    const long long total = (long long)C.n * c * hw;
    hipLaunchKernelGGL(k_t_bn_bwd_dx, dim3(ceil_div(total, 256)), dim3(256), 0, C.s, dy, x, relu_out, mean, invstd, gamma, (const float*)dgamma,
                       (const float*)dbeta, C.n, c, hw, total, train, post_mask);
}
}  // namespace

extern "C" int rpe_unet_train_forward(const float* const* src, const int* src_channels, const long long* src_batch_strides, int nsrc,
                                      const float* const* params, float* const* running_mean, float* const* running_var,
                                      long long* const* num_batches_tracked, const float* momentum, const float* eps, int train_mask,
                                      int n, int h8, int w8, int out_h, int out_w, int sigmoid, float* out, void* workspace, void* stream) {
    TCall C;
    if (!out || !running_mean || !running_var || !momentum || !eps) return RPE_E_BADARG;
    const int st = t_setup(C, src, src_channels, src_batch_strides, nsrc, params, n, h8, w8, out_h, out_w, workspace, stream);
    if (st != RPE_OK) return st;
    for (int k = 0; k < UT_NNORM; ++k) if (!running_mean[k] || !running_var[k]) return RPE_E_BADARG;
    const UtGeo& g = C.g; const UtPlan& pl = C.pl; const float* const* prm = params;
    auto bn = [&](int norm, const float* x, float* y, int c, int hw, const float* gamma, const float* beta, int relu) {
        hipLaunchKernelGGL(k_t_bn_stats, dim3(c), dim3(256), 0, C.s, x, n, c, hw, eps[norm], momentum[norm], (train_mask >> norm) & 1, running_mean[norm],
                           running_var[norm], num_batches_tracked ? num_batches_tracked[norm] : nullptr, C.at(pl.mean[norm]), C.at(pl.invstd[norm]));
        const long long total = (long long)n * c * hw;
        hipLaunchKernelGGL(k_t_bn_apply, dim3(ceil_div(total, 256)), dim3(256), 0, C.s, x, (const float*)C.at(pl.mean[norm]),
                           (const float*)C.at(pl.invstd[norm]), gamma, beta, y, c, hw, total, relu);
    };
    int ch = h8, cw = w8;
    const float* cur = nullptr;
    for (int i = 0; i < 3; ++i) {
        const int c = UT_WIDTHS[i], cin = i ? UT_WIDTHS[i - 1] : C.cin;
        const float* const* q = prm + 6 * i;
        TSrc one = i ? t_map(cur, cin, ch, cw) : TSrc{};
        t_conv3(C, i ? &one : C.in, i ? 1 : C.nsrc, cin, q[0], q[1], C.at(pl.a1[i]), c, g.h[i], g.w[i], 0);
        bn(i, C.at(pl.a1[i]), C.at(pl.r1[i]), c, g.h[i] * g.w[i], q[2], q[3], 1);
        TSrc mid = t_map(C.at(pl.r1[i]), c, g.h[i], g.w[i]);
        t_conv3(C, &mid, 1, c, q[4], q[5], C.at(pl.skip[i]), c, g.hs[i], g.ws[i], 0);
        if (i < 2) {
            ch = g.hs[i] / 2; cw = g.ws[i] / 2;
            const long long total = (long long)n * c * ch * cw;
            hipLaunchKernelGGL(k_t_pool, dim3(ceil_div(total, 256)), dim3(256), 0, C.s, (const float*)C.at(pl.skip[i]), C.at(pl.pool[i]), g.hs[i], g.ws[i], total);
            cur = C.at(pl.pool[i]);
        } else { cur = C.at(pl.skip[2]); ch = g.hs[2]; cw = g.ws[2]; }
    }
    for (int j = 0; j < 2; ++j) {
        const int c = UT_WIDTHS[2 - j], c2 = c / 2, si = 1 - j, mh = g.dh[j] + 2, mw = g.dw[j] + 2;
        const float* const* q = prm + 18 + 8 * j;
        hipLaunchKernelGGL(k_t_upconv, dim3(ceil_div(4 * ch * cw, 256), c2 / TCT, n), dim3(256), 0, C.s, cur, q[0], q[1], C.at(pl.up[j]), c, c2, ch, cw);
        TSrc two[2] = {t_map(C.at(pl.up[j]), c2, g.uh[j], g.uw[j]),
                       t_map(C.at(pl.skip[si]), c2, g.hs[si], g.ws[si], (g.hs[si] - g.uh[j]) / 2, (g.ws[si] - g.uw[j]) / 2)};
        t_conv3(C, two, 2, c, q[2], q[3], C.at(pl.r[j]), c2, mh, mw, 1);
        bn(3 + j, C.at(pl.r[j]), C.at(pl.nrm[j]), c2, mh * mw, q[4], q[5], 0);
        TSrc mid = t_map(C.at(pl.nrm[j]), c2, mh, mw);
        t_conv3(C, &mid, 1, c2, q[6], q[7], C.at(pl.dout[j]), c2, g.dh[j], g.dw[j], 0);
        cur = C.at(pl.dout[j]); ch = g.dh[j]; cw = g.dw[j];
    }
    hipLaunchKernelGGL(k_t_head, dim3(ceil_div(ch * cw, 256), 1, n), dim3(256), 0, C.s, cur, prm[34], prm[35], C.at(pl.hm), ch * cw);
    hipLaunchKernelGGL(k_t_resize, dim3(ceil_div((long long)out_h * out_w, 256), 1, n), dim3(256), 0, C.s, (const float*)C.at(pl.hm), out, ch, cw, out_h, out_w,
                       (float)ch / (float)out_h, (float)cw / (float)out_w, sigmoid);
    return rpe_check_launch();
}

extern "C" int rpe_unet_train_backward(const float* grad_out, const float* out, const float* const* src, const int* src_channels,
                                       const long long* src_batch_strides, int nsrc, const float* const* params, int train_mask, int n, int h8, int w8,
                                       int out_h, int out_w, int sigmoid, float* grad_params, float* grad_input, void* workspace, void* stream) {
    TCall C;
    if (!grad_out || !grad_params || (sigmoid && !out)) return RPE_E_BADARG;
    const int st = t_setup(C, src, src_channels, src_batch_strides, nsrc, params, n, h8, w8, out_h, out_w, workspace, stream);
    if (st != RPE_OK) return st;
    const UtGeo& g = C.g; const UtPlan& pl = C.pl; const float* const* prm = params;
    auto gp = [&](int k) { return grad_params + ut_grad_offset(C.cin, k); };
    const int fh = g.dh[1], fw = g.dw[1], fpix = fh * fw;
    hipLaunchKernelGGL(k_t_resize_bwd, dim3(ceil_div((long long)n * fpix, 4)), dim3(256), 0, C.s, grad_out, sigmoid ? out : nullptr, C.at(pl.g_hm), n, fh, fw,
                       out_h, out_w, (float)fh / (float)out_h, (float)fw / (float)out_w, sigmoid);
    hipLaunchKernelGGL(k_t_head_bwd_weight, dim3(17), dim3(256), 0, C.s, (const float*)C.at(pl.dout[1]), (const float*)C.at(pl.g_hm), n, fpix, gp(34), gp(35));
    hipLaunchKernelGGL(k_t_head_bwd_data, dim3(ceil_div(fpix, 256), 1, n), dim3(256), 0, C.s, (const float*)C.at(pl.g_hm), prm[34], C.at(pl.g_dout[1]), fpix);
    for (int j = 1; j >= 0; --j) {
        const int c = UT_WIDTHS[2 - j], c2 = c / 2, si = 1 - j, mh = g.dh[j] + 2, mw = g.dw[j] + 2, kb = 18 + 8 * j;
        const float* const* q = prm + kb;
        // conv2, then the norm and the ReLU in front of it
        TSrc mid = t_map(C.at(pl.nrm[j]), c2, mh, mw);
        t_conv3_bwd_wb(C, &mid, 1, c2, C.at(pl.g_dout[j]), c2, g.dh[j], g.dw[j], gp(kb + 6), gp(kb + 7));
        t_conv3_bwd_data(C, C.at(pl.g_dout[j]), q[6], C.at(pl.g_nrm[j]), c2, c2, 0, c2, g.dh[j], g.dw[j], mh, mw, 0, 0);
        t_bn_bwd(C, C.at(pl.g_nrm[j]), C.at(pl.r[j]), nullptr, 3 + j, c2, mh * mw, q[4], gp(kb + 4), gp(kb + 5), (train_mask >> (3 + j)) & 1, 1);
        // conv1 over (up | centre-cropped skip): the skip's share is written over the whole skip map, zero outside the crop
        const int oy = (g.hs[si] - g.uh[j]) / 2, ox = (g.ws[si] - g.uw[j]) / 2;
        TSrc two[2] = {t_map(C.at(pl.up[j]), c2, g.uh[j], g.uw[j]), t_map(C.at(pl.skip[si]), c2, g.hs[si], g.ws[si], oy, ox)};
        t_conv3_bwd_wb(C, two, 2, c, C.at(pl.g_nrm[j]), c2, mh, mw, gp(kb + 2), gp(kb + 3));
        t_conv3_bwd_data(C, C.at(pl.g_nrm[j]), q[2], C.at(pl.g_up[j]), c2, c, 0, c2, mh, mw, g.uh[j], g.uw[j], 0, 0);
        t_conv3_bwd_data(C, C.at(pl.g_nrm[j]), q[2], C.at(pl.g_skip[si]), c2, c, c2, c2, mh, mw, g.hs[si], g.ws[si], oy, ox);
        // up-convolution; its input was the previous decoder stage's output, or the last encoder stage's
        const int ih = g.uh[j] / 2, iw = g.uw[j] / 2;
        const float* uin = j ? C.at(pl.dout[0]) : C.at(pl.skip[2]);
        float* duin = j ? C.at(pl.g_dout[0]) : C.at(pl.g_skip[2]);
        hipLaunchKernelGGL(k_t_upconv_bwd_weight, dim3(c, c2), dim3(256), 0, C.s, uin, (const float*)C.at(pl.g_up[j]), gp(kb), n, c, c2, ih, iw);
        hipLaunchKernelGGL(k_t_chan_sum, dim3(c2), dim3(256), 0, C.s, (const float*)C.at(pl.g_up[j]), n, c2, g.uh[j] * g.uw[j], gp(kb + 1));
        hipLaunchKernelGGL(k_t_upconv_bwd_data, dim3(ceil_div(ih * iw, 256), c / TCT, n), dim3(256), 0, C.s, (const float*)C.at(pl.g_up[j]), q[0], duin, c, c2, ih, iw);
    }
    for (int i = 2; i >= 0; --i) {
        const int c = UT_WIDTHS[i], cin = i ? UT_WIDTHS[i - 1] : C.cin, kb = 6 * i;
        const float* const* q = prm + kb;
        TSrc mid = t_map(C.at(pl.r1[i]), c, g.h[i], g.w[i]);
        t_conv3_bwd_wb(C, &mid, 1, c, C.at(pl.g_skip[i]), c, g.hs[i], g.ws[i], gp(kb + 4), gp(kb + 5));
        t_conv3_bwd_data(C, C.at(pl.g_skip[i]), q[4], C.at(pl.g_r1[i]), c, c, 0, c, g.hs[i], g.ws[i], g.h[i], g.w[i], 0, 0);
        t_bn_bwd(C, C.at(pl.g_r1[i]), C.at(pl.a1[i]), C.at(pl.r1[i]), i, c, g.h[i] * g.w[i], q[2], gp(kb + 2), gp(kb + 3), (train_mask >> i) & 1, 0);
        if (i) {
            const int ph = g.hs[i - 1] / 2, pw = g.ws[i - 1] / 2;
            TSrc one = t_map(C.at(pl.pool[i - 1]), cin, ph, pw);
            t_conv3_bwd_wb(C, &one, 1, cin, C.at(pl.g_r1[i]), c, g.h[i], g.w[i], gp(kb), gp(kb + 1));
            t_conv3_bwd_data(C, C.at(pl.g_r1[i]), q[0], C.at(pl.g_pool[i - 1]), c, cin, 0, cin, g.h[i], g.w[i], ph, pw, 0, 0);
            const long long total = (long long)n * cin * g.hs[i - 1] * g.ws[i - 1];
            hipLaunchKernelGGL(k_t_pool_bwd_add, dim3(ceil_div(total, 256)), dim3(256), 0, C.s, (const float*)C.at(pl.skip[i - 1]), (const float*)C.at(pl.pool[i - 1]),
                               (const float*)C.at(pl.g_pool[i - 1]), C.at(pl.g_skip[i - 1]), g.hs[i - 1], g.ws[i - 1], total);
        } else {
            t_conv3_bwd_wb(C, C.in, C.nsrc, cin, C.at(pl.g_r1[0]), c, g.h[0], g.w[0], gp(0), gp(1));
            if (grad_input)
                t_conv3_bwd_data(C, C.at(pl.g_r1[0]), q[0], grad_input, c, cin, 0, cin, g.h[0], g.w[0], C.h8, C.w8, 0, 0);
        }
    }
    return rpe_check_launch();
}
