// What the split-K GEMMs of the training backward share, whatever their operands: part = A B^T per chunk of the contraction axis on the f32
// matrix cores, then a second pass that adds the chunks' partials.  The users are the convolution weight gradient (raft_backward.hip, all five
// kernel sizes) and the two GEMMs of the correlation build's adjoint (corr_backward.hip).
//   split_chunk / split_chunks   the chunk of the contraction axis, a function of its length alone (part of the result's bits)
//   BW_*, f32x16                 the tile: 128 x 128 x 32 per workgroup, LDS pitch, the accumulator type
//   bw_gemm_body<KH, KW>         the weight gradient's tile over one chunk: stage, multiply, store the partial
//   k_splitk_reduce              out = scale * the partials added in chunk order in f64, rounded once
// k_cb_gemm (corr_backward.hip) keeps a main loop of its own with the same tile: one loop over a loader object was tried and moved the
// register allocation of every instantiation (NOTES.md), so the two loops stay apart until that can be done at equal registers.
#pragma once
#include <type_traits>
#include "rpe_common.h"

// at most max_chunks chunks of whole 32-steps, each at least min_len long
static inline long long split_chunk(long long K, int max_chunks, int min_len) {
    const long long c = ((K + max_chunks - 1) / max_chunks + 31) / 32 * 32;
    return c < min_len ? min_len : c;
}
static inline int split_chunks(long long K, int max_chunks, int min_len) {
    const long long c = split_chunk(K, max_chunks, min_len);
    return (int)((K + c - 1) / c);
}

#define BW_BM 128                 // rows of A (M) per workgroup: output channels
#define BW_BN 128                 // rows of B (N) per workgroup: (input channel, tap) pairs
#define BW_BK 32                  // k per step: pixels
#define BW_LD (BW_BK + 4)         // LDS row pitch in floats: 16-byte aligned rows, 4-float reads of a lane's k-run
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Workgroup = 4 waves, each 2 x 2 tiles of v_mfma_f32_32x32x2_f32 (64 accumulators per lane).  Staging: thread t loads pixel column
// t & 31 of rows (t >> 5) + 8 r, r = 0..15, of both operand tiles, so the pixel's (batch, y, x) split and its kh * kw border tests are done
// once per step and a load is coalesced along the pixels; a tap outside the map (or a row / pixel outside the problem) is read from a
// clamped address and SELECTED to zero.  K is permuted inside a step (lane half h takes pixels 16 h .. 16 h + 15 of the step, for BOTH
// operands): a sum does not care, and a lane's operands of four consecutive instructions are one 16-byte LDS read.
// The body is a device function over (KH, KW) -- tap t = (t / KW - KH / 2, t % KW - KW / 2) --, one piece of code for the five kernel sizes of
// raft_backward.hip's k_bw_gemm; sA / sB: BW_BM * BW_LD and BW_BN * BW_LD floats of LDS, 16-byte aligned.
template <int KH, int KW>
__device__ __forceinline__ void bw_gemm_body(const float* __restrict__ x, long long xbs, const float* __restrict__ dy, long long dybs, int cin,
                                             int cout, int h, int w, long long K, long long kc, float* __restrict__ part, float* sA, float* sB) {
    constexpr int TAPS = KH * KW;
    typedef typename std::conditional<(TAPS > 31), unsigned long long, unsigned>::type mask_t;      // one bit per tap
    constexpr int NOTAP = TAPS > 31 ? 63 : 31;                       // a bit no tap sets: a row outside the problem
    const int N = cin * TAPS, M = cout;
    const int n0 = blockIdx.x * BW_BN, m0 = blockIdx.y * BW_BM;
    const long long kbeg = (long long)blockIdx.z * kc, kend = kbeg + kc < K ? kbeg + kc : K;
    const int hw = h * w;
    const int tid = threadIdx.x, kl = tid & 31, r0 = tid >> 5;
    // per staged row: the operand's offset inside a batch item, and (B) the tap whose border test decides it; NOTAP = a row outside the problem
    int aoff[16], boff[16], btap[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + r0 + 8 * r, n = n0 + r0 + 8 * r;
        aoff[r] = m < M ? m * hw : -1;
        const int ci = n / TAPS, tap = n - ci * TAPS;
        const int dyo = tap / KW - KH / 2, dxo = tap % KW - KW / 2;
        boff[r] = ci * hw + dyo * w + dxo;
        btap[r] = n < N ? tap : NOTAP;
    }
    float ra[16], rb[16];
    auto load = [&](long long kstep) {
        const long long k = kstep + kl;
        const bool kv = k < kend;
        const long long kk = kv ? k : kbeg;                           // (kbeg < K: the grid has no empty chunk)
        const int bb = (int)(kk / hw), p = (int)(kk - (long long)bb * hw);
        const int py = p / w, px = p - py * w;
        mask_t vm = 0;
        if (TAPS > 1) {
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int yy = py + t / KW - KH / 2, xx = px + t % KW - KW / 2;
                vm |= (mask_t)(kv && yy >= 0 && yy < h && xx >= 0 && xx < w) << t;
            }
        } else vm = kv ? 1u : 0u;
        const float* ab = dy + (size_t)bb * dybs + p;
        const float* xb = x + (size_t)bb * xbs + p;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool av = kv && aoff[r] >= 0;
            const float a = ab[av ? aoff[r] : 0];                     // (offset 0 + p: inside channel 0 of this batch item)
            ra[r] = av ? a : 0.0f;
            const bool bv = (vm >> btap[r]) & 1u;
            const float v = xb[bv ? boff[r] : 0];
            rb[r] = bv ? v : 0.0f;
        }
    };
    const int lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int li = lane & 31, lh = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][c][e] = 0.0f;
    load(kbeg);
    for (long long ks = kbeg; ks < kend; ks += BW_BK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { sA[(r0 + 8 * r) * BW_LD + kl] = ra[r]; sB[(r0 + 8 * r) * BW_LD + kl] = rb[r]; }
        __syncthreads();
        if (ks + BW_BK < kend) load(ks + BW_BK);                      // the next step's operands travel while this one multiplies
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
        __syncthreads();
    }
    // C / D layout of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* out = part + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n = n0 + wn * 64 + c * 32 + li;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m < M && n < N) out[(size_t)m * N + n] = acc[a][c][e];
            }
        }
}

// out[bz][e] = (float)(scale * sum_c part[bz][c][e]), e < per: c in index order, in f64, one rounding.  grid (blocks, batch), any block count.
static __global__ __launch_bounds__(256) void k_splitk_reduce(const float* __restrict__ part, int chunks, size_t per, double scale,
                                                              float* __restrict__ out) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += (double)part[((size_t)bz * chunks + c) * per + e];
        out[(size_t)bz * per + e] = (float)(scale * s);
    }
}
static inline void splitk_reduce_launch(const float* part, int batch, int chunks, long long per, double scale, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_splitk_reduce, dim3(min(ceil_div(per, 256), 2048), batch), dim3(256), 0, s, part, chunks, (size_t)per, scale, out);
}
