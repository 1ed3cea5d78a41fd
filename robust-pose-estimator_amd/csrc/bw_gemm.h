// The convolution weight gradient's GEMM on the f32 matrix cores, shared by raft_backward.hip (3x3, 1x1) and update_backward.hip (1x5, 5x1,
// 7x7): the split of K, the tile constants and the kernel body.
#pragma once
#include <type_traits>
#include "rpe_common.h"

static inline long long bw_chunk(long long K) {
    long long c = ((K + 63) / 64 + 31) / 32 * 32;                 // at most 64 chunks, whole 32-pixel steps
    return c < 1024 ? 1024 : c;                                   // ... of at least 1024 pixels
}
static inline int bw_chunks(long long K) { return (int)((K + bw_chunk(K) - 1) / bw_chunk(K)); }

#define BW_BM 128                 // output channels per workgroup
#define BW_BN 128                 // (input channel, tap) pairs per workgroup
#define BW_BK 32                  // pixels per step
#define BW_LD (BW_BK + 4)         // LDS row pitch in floats: 16-byte aligned rows, 4-float reads of a lane's k-run
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Workgroup = 4 waves, each 2 x 2 tiles of v_mfma_f32_32x32x2_f32 (64 accumulators per lane).  Staging: thread t loads pixel column
// t & 31 of rows (t >> 5) + 8 r, r = 0..15, of both operand tiles, so the pixel's (batch, y, x) split and its kh * kw border tests are done
// once per step and a load is coalesced along the pixels; a tap outside the map (or a row / pixel outside the problem) is read from a
// clamped address and SELECTED to zero.  K is permuted inside a step (lane half h takes pixels 16 h .. 16 h + 15 of the step, for BOTH
// operands): a sum does not care, and a lane's operands of four consecutive instructions are one 16-byte LDS read.
// The body is a device function over (KH, KW) -- tap t = (t / KW - KH / 2, t % KW - KW / 2) -- so that the kernels of raft_backward.hip (3x3, 1x1)
// and of update_backward.hip (1x5, 5x1, 7x7) are one piece of code; sA / sB: BW_BM * BW_LD and BW_BN * BW_LD floats of LDS, 16-byte aligned.
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

// The kernel sizes beyond 3x3 and 1x1 ('same' padding (0,2), (2,0), (3,3)) and the launch of their first pass (update_backward.hip)
static inline bool bw_ext_kernel(int kh, int kw) { return (kh == 1 && kw == 5) || (kh == 5 && kw == 1) || (kh == 7 && kw == 7); }
bool bw_gemm_launch_ext(const float* x, long long xbs, const float* dy, long long dybs, int cin, int cout, int h, int w, int kh, int kw,
                        long long K, long long kc, int chunks, float* part, hipStream_t s);
