// rpe_conv_f16: the update block's stride-1 "same" convolutions (1x1, 3x3, 1x5, 5x1) with fp16 OPERANDS on the 16-bit matrix cores
// (v_mfma_f32_32x32x16_f16), the route of RAFT's ``update_fp16``.  Upstream RAFT's mixed_precision runs these layers under autocast
// (core/RAFT/core/update.py: BasicMotionEncoder, SepConvGRU, FlowHead.conv1, the mask head; call sites core/pose/pose_net.py:47,65,129).
//
// Contract (include/rpe.h): every input activation and every weight is rounded to IEEE fp16, round to nearest even, unscaled; products are
// exact in f32; the sum is f32 in ONE fixed order (K steps of 32 channels, inside a step tap by tap, inside a tap two 16-channel matrix
// instructions) whatever the tile class, the batch or the launch size -- no atomics, no split K; everything after the sum is
// rpe_conv_fused's f32 epilogue (conv_epilogue.h, shared with conv.hip).  Activations stay f32 in memory: the rounding happens while a
// patch is staged.
//
// GEMM view per batch item: M = output channels (A = the packed fp16 weights, read from global memory in fragment order: a lane's 8 halves
// are one 16-byte load that every workgroup of the launch shares through L2), N = a 16 x 8 pixel patch, K = cin * taps.
// LDS: the raw input patch WITH its halo as a [pixel][channel] fp16 image, staged once per K step and reused by every tap: a tap is an
// address offset, a lane's B fragment one ds_read_b128.  A pixel holds 32 channels in 80 bytes (16 consecutive pixels tile the 64 banks).
// Staging: a thread converts 4 channels x 4 pixels (four 16-byte loads) and writes four 8-byte pieces, lanes running over the channel quads
// first, so 32 lanes write 64 distinct banks.  Zero padding, and the channels beyond cin of the last K step, are selected as zero here and
// never read: a NaN behind the slice cannot enter through 0 * NaN.  The image is double buffered: the next step's global loads are issued
// before the current step's matrix instructions, and written to LDS after them; one barrier per step.
// Workgroup = 4 waves, a wave owns 32 output channels x 128 pixels (WM = 4: 128-channel tiles) or x 64 pixels (WM = 2: 64-channel tiles, for
// cout % 128 in 1..64: 20, 64, 192, 576).
#include "conv_host.h"
#include "conv_epilogue.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define F16_KC 32                             /* channels per K step: two matrix instructions per tap */
#define F16_PS 40                             /* halves per LDS pixel (32 used) */
#define F16_TX 16
#define F16_TY 8
#define F16_FRAG 512                          /* halves of one packed A fragment: 64 lanes x 8 */

struct ConvF16P {
    const float* x; long long xbs;
    const _Float16* wp;                       // [co / 32][step][tap][2][64 lanes][8]
    int cin, cout, coP, H, W, hw;
    const float* bias;
    const float* add; long long abs_;
    int mode;
    float* out; long long obs;
    float* out2; long long o2bs;
    const float* h; long long hbs;
    const float* z; long long zbs;
    int cgate;
};

template <int KH, int KW, int WM>
__global__ __launch_bounds__(256) void k_conv_f16(ConvF16P P) {
    constexpr int WN = 4 / WM, NBW = 4 / WN, BM = 32 * WM, TAPS = KH * KW;
    constexpr int ROWS = F16_TY + KH - 1, XOFF = KW > 1 ? 4 : 0, COLS = F16_TX + 2 * XOFF, CQ = COLS / 4, NPQ = ROWS * CQ;
    constexpr int NIT = (NPQ * 8 + 255) / 256;                   // staging items (4 channels x 4 pixels) per thread
    constexpr int CSH = XOFF - KW / 2;                           // staged column of tap dx = 0 at output column 0
    __shared__ __attribute__((aligned(16))) _Float16 Bs[2][ROWS * COLS][F16_PS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int wm = wv / WN, wn = wv % WN;
    const int W = P.W, H = P.H, hw = P.hw;
    const int tiles_x = (W + F16_TX - 1) / F16_TX;
    const int tx0 = (blockIdx.x % tiles_x) * F16_TX, ty0 = (blockIdx.x / tiles_x) * F16_TY;
    const int bz = blockIdx.z, m0 = blockIdx.y * BM;
    const float* xb = P.x + (size_t)bz * P.xbs;
    const int nsteps = (P.cin + F16_KC - 1) / F16_KC;

    // staging items of this thread: item = (channel quad cq = idx % 8, pixel quad pq = idx / 8); step-invariant part
    const int cq = tid & 7;
    int poff[NIT], pix[NIT]; bool pin[NIT];
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int pq = (tid + 256 * u) >> 3, r = pq / CQ, q = pq - r * CQ;
        const int y = ty0 + r - KH / 2, x = tx0 - XOFF + 4 * q;
        pix[u] = pq < NPQ ? r * COLS + 4 * q : -1;               // -1: no such item
        pin[u] = pq < NPQ && y >= 0 && y < H && x >= 0 && x + 3 < W;   // (w % 4 == 0: a quad lies wholly inside or outside the row)
        poff[u] = pin[u] ? y * W + x : 0;
    }
    struct RB { float4 v[NIT][4]; unsigned ok; };
    // the global loads of step s; issued unconditionally (lanes without data read the slice's first 16 bytes and are selected to zero
    // when the patch is written: a load under a branch makes the compiler wait for it on every path)
    auto load_b = [&](RB& R, int s) {
        R.ok = 0;
#pragma unroll
        for (int u = 0; u < NIT; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ch = s * F16_KC + 4 * cq + k;
                const bool ok = pin[u] && ch < P.cin;
                R.v[u][k] = *(const float4*)(ok ? xb + (size_t)ch * hw + poff[u] : P.x);
                R.ok |= ok ? (1u << (4 * u + k)) : 0u;
            }
    };
    auto store_b = [&](const RB& R, int buf) {
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            if (pix[u] < 0) continue;
            float c[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = (R.ok >> (4 * u + k)) & 1;
                c[k][0] = ok ? R.v[u][k].x : 0.0f; c[k][1] = ok ? R.v[u][k].y : 0.0f; c[k][2] = ok ? R.v[u][k].z : 0.0f; c[k][3] = ok ? R.v[u][k].w : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {                        // (a plain conversion rounds to nearest even; v_cvt_pkrtz_f16_f32 would truncate)
                const f16x4 hv = {(_Float16)c[0][i], (_Float16)c[1][i], (_Float16)c[2][i], (_Float16)c[3][i]};
                *(f16x4*)&Bs[buf][pix[u] + i][4 * cq] = hv;
            }
        }
    };

    f32x16 acc[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    // false: this wave's 32 output rows lie beyond cout (scalar on purpose; the wave still stages and synchronises).  Its fragments do not
    // exist in the packed weights either.
    const bool active = __builtin_amdgcn_readfirstlane(m0 + wm * 32) < P.cout;
    const _Float16* wa = P.wp + (size_t)(m0 / 32 + wm) * nsteps * TAPS * 2 * F16_FRAG + lane * 8;
    const int prow0 = l31 >> 4, pcol0 = (l31 & 15) + CSH;

    auto compute = [&](int s, int buf) {
        if (!active) return;
        const _Float16* ws = wa + (size_t)s * TAPS * 2 * F16_FRAG;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int dy = t / KW, dx = t % KW;
            const f16x8 a0 = *(const f16x8*)(ws + (2 * t) * F16_FRAG), a1 = *(const f16x8*)(ws + (2 * t + 1) * F16_FRAG);
#pragma unroll
            for (int jj = 0; jj < NBW; ++jj) {
                const int j = wn * NBW + jj;
                const _Float16* bp = &Bs[buf][(2 * j + prow0 + dy) * COLS + pcol0 + dx][8 * lh];
                const f16x8 b0 = *(const f16x8*)bp, b1 = *(const f16x8*)(bp + 16);
                acc[jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[jj], 0, 0, 0);
            }
        }
    };

    RB R;
    load_b(R, 0);
    store_b(R, 0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        load_b(R, s + 1);                                        // (past the end: every channel is >= cin, nothing is read)
        compute(s, s & 1);
        if (s + 1 < nsteps) store_b(R, (s + 1) & 1);             // its last readers, step s - 1, sit before the previous barrier
        __syncthreads();
    }

    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    if (!active) return;
    const ConvEpi E = {P.bias, P.add ? P.add + (size_t)bz * P.abs_ : nullptr, P.h ? P.h + (size_t)bz * P.hbs : nullptr,
                       P.z ? P.z + (size_t)bz * P.zbs : nullptr, P.out + (size_t)bz * P.obs, P.out2 ? P.out2 + (size_t)bz * P.o2bs : nullptr,
                       P.mode, P.cgate, P.cout, hw};
    const int co0 = m0 + wm * 32 + 4 * lh;
#pragma unroll
    for (int jj = 0; jj < NBW; ++jj) {
        const int oy = ty0 + 2 * (wn * NBW + jj) + prow0, ox = tx0 + (l31 & 15);
        const bool pok = oy < H && ox < W;
        const int px = pok ? oy * W + ox : 0;
#pragma unroll
        for (int rb = 0; rb < 16; rb += 4)
            conv_epilogue_rows4(E, acc[jj][rb], acc[jj][rb + 1], acc[jj][rb + 2], acc[jj][rb + 3], co0 + 8 * (rb >> 2), px, pok);
    }
}

static inline bool f16_kernel_ok(int kh, int kw) { return (kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 1 && kw == 5) || (kh == 5 && kw == 1); }
static inline int f16_steps(int cin) { return (cin + F16_KC - 1) / F16_KC; }

// (cout, cin, kh, kw) f32 -> fp16 (round to nearest even) in A-fragment order [co / 32][step][tap = dy * kw + dx][2][lane][8]: element i of
// lane l of fragment kk is weight[32 * mt + l % 32][32 * step + 16 * kk + 8 * (l / 32) + i][dy][dx], zero beyond cout / cin (the K tail).
__global__ void k_conv_f16_pack(const float* __restrict__ w, _Float16* __restrict__ wp, int cout, int cin, int kh, int kw, int nsteps, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e & 7), lane = (int)((e >> 3) & 63), kk = (int)((e >> 9) & 1);
    long long rest = e >> 10;
    const int taps = kh * kw;
    const int t = (int)(rest % taps); rest /= taps;
    const int s = (int)(rest % nsteps), mt = (int)(rest / nsteps);
    const int co = mt * 32 + (lane & 31), ci = s * F16_KC + kk * 16 + 8 * (lane >> 5) + i, dy = t / kw, dx = t % kw;
    wp[e] = (co < cout && ci < cin) ? (_Float16)w[(((size_t)co * cin + ci) * kh + dy) * kw + dx] : (_Float16)0.0f;
}

extern "C" size_t rpe_conv_f16_packed_bytes(int cout, int cin, int kh, int kw) {
    if (cout <= 0 || cin <= 0 || !f16_kernel_ok(kh, kw)) return 0;
    return (size_t)ceil_div(cout, 32) * f16_steps(cin) * kh * kw * 2 * F16_FRAG * sizeof(_Float16);
}

extern "C" int rpe_conv_f16_pack(const float* weight, int cout, int cin, int kh, int kw, void* packed, void* stream) {
    if (!weight || !packed || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) return RPE_E_BADARG;
    if (!f16_kernel_ok(kh, kw) || (((uintptr_t)packed) & 15)) return RPE_E_UNSUPPORTED;
    return launch_pack(k_conv_f16_pack, weight, (_Float16*)packed, cout, cin, 1, (long long)(rpe_conv_f16_packed_bytes(cout, cin, kh, kw) / sizeof(_Float16)),
                       stream, kh, kw, f16_steps(cin));
}

// 64-channel tiles where the last 128-channel tile would be at most half full (cout = 20, 64, 192, 576).  A function of cout alone, and the
// sum order is that of the K walk in either class: a row's bits depend neither on its batch nor on the tile class.
static inline bool f16_tiles64(int cout) { return (cout % 128) != 0 && (cout % 128) <= 64; }

extern "C" int rpe_conv_f16(const rpe_conv_desc* d, void* stream) {
    if (!conv_desc_present(d)) return RPE_E_BADARG;
    if (d->mode < RPE_CONV_LINEAR || d->mode > RPE_CONV_TANH) return RPE_E_BADARG;
    if (!conv_gate_args_ok(d)) return RPE_E_BADARG;
    if (!f16_kernel_ok(d->kh, d->kw) || !stride_is_1(d) || !conv_no_encoder_epilogue(d)) return RPE_E_UNSUPPORTED;
    if ((d->w & 3) || d->b > 65535 || (((uintptr_t)d->packed) & 15)) return RPE_E_UNSUPPORTED;
    if (!aligned16(d->x, d->x_batch_stride) || !aligned16(d->out, d->out_batch_stride) || !aligned16(d->out2, d->out2_batch_stride) ||
        !aligned16(d->add, d->add_batch_stride) || !aligned16(d->hidden, d->hidden_batch_stride) || !aligned16(d->zgate, d->zgate_batch_stride))
        return RPE_E_UNSUPPORTED;
    ConvF16P P;
    fill_common(P, d, round_up(d->cout, 32)); fill_gate(P, d);
    P.H = d->h; P.W = d->w; P.hw = d->h * d->w; P.h = d->hidden; P.hbs = d->hidden_batch_stride;
    const bool t64 = f16_tiles64(d->cout);
    const dim3 grid(ceil_div(d->w, F16_TX) * ceil_div(d->h, F16_TY), ceil_div(d->cout, t64 ? 64 : 128), d->b), block(256);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(KH_, KW_) do { if (t64) hipLaunchKernelGGL((k_conv_f16<KH_, KW_, 2>), grid, block, 0, s, P); \
                              else hipLaunchKernelGGL((k_conv_f16<KH_, KW_, 4>), grid, block, 0, s, P); } while (0)
    if (d->kh == 3) LAUNCH(3, 3); else if (d->kh == 5) LAUNCH(5, 1); else if (d->kw == 5) LAUNCH(1, 5); else LAUNCH(1, 1);
#undef LAUNCH
    return rpe_check_launch();
}
