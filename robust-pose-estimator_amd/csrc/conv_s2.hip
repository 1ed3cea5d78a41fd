// The 96-row tile class of the stride-2 3x3 implicit GEMM (conv.hip: k_conv_igemm<3, 2, true, 2, false, true>) for the encoders'
// 64 -> 96 channel down-sampling layers (core/RAFT/core/extractor.py: layer2's first ResidualBlock.conv1).
//
// k_conv_igemm covers 96 output channels with a 128-row tile: two of its four waves own rows 64..127, of which 96..127 do not exist.
// Those waves skip the matrix instructions of the missing rows, so on every CU two SIMDs carry 4 MFMA blocks per k-step and the other
// two carry 2, and the launch runs at the pace of the loaded pair.  Here the workgroup's tile is 96(co) x 128(px) and each of the four
// waves owns ALL 96 rows of a 32-pixel column block (3 x 1 MFMA 32x32x2 blocks): every SIMD carries 3 blocks, nothing is staged for
// rows that do not exist (the weights tile is [16][96]), and the input staging -- written for 256 threads and a 128-pixel tile -- is
// k_conv_igemm's stride-2 staging unchanged (even / odd de-interleave, O[-1] halo, taps as LDS row offsets).
//
// Bit-identical to the 128-row class: K is walked in the same order ((chunk of 16 ci, dy), dx; lane half lh of k2-step j supplies
// k = 8*lh + j), every output element is the same fmaf chain from a zero accumulator, the epilogue is the same fmaf(acc, scale, bias)
// [ReLU], and the instance-norm statistics are the same records: one per 32-pixel block of the plane, about the block's first column
// as pivot, summed over the 32 lanes by the same DPP tree (a wave's column block here IS one record; there a wave held two).
// Epilogues: scale / bias / ReLU / moments -- what the stride-2 layers use; residual, addend and second output stay on k_conv_igemm.
#include "conv_igemm.h"
#include <type_traits>

// VALID: as k_conv_igemm's -- zero stored outside the valid extent P.Hv x P.Wv of the output map, statistics over the pixels inside it
template <bool VALID>
__global__ __launch_bounds__(256, 2) void k_conv_s2_m96(ConvP P) {
    constexpr int BM = 96, BN = 128, KS = 20, NLB = BN / 32, KW = 3;
    __shared__ __attribute__((aligned(16))) float As[2][BM][KS];
    __shared__ __attribute__((aligned(16))) float Bs[2][2 * BN + 8][KS];        // rows 0..BN-1: E[n]; row BN: O[-1]; rows BN+1+n: O[n]
    __shared__ __attribute__((aligned(8))) float sbt[BM][2];                     // (scale | 1, bias | 0) of the channel rows
    const int bz = blockIdx.z, n0 = blockIdx.x * BN;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int W = P.W, hw = P.hw, ph = P.kh / 2;
    if (tid < BM) {
        sbt[tid][0] = P.scale ? P.scale[tid] : 1.0f;
        sbt[tid][1] = P.bias ? P.bias[tid] : 0.0f;
    }
    const int hw_in = P.Hin * P.Win;
    // weights loader: the [4 k4][96] float4 of a step are 384 = 256 + 128: float4 i -> (k4 = i / 96, m = i % 96), thread -> i = tid and
    // i = 256 + tid % 128 (threads 128..255 repeat the second float4 of threads 0..127: the same value to the same LDS address, and no
    // load or store under a branch).  Packed as [step][k4][coP][4].
    const int i1 = 256 + (tid & 127);
    const int a_m0 = tid % BM, a_k40 = tid / BM, a_m1 = i1 % BM, a_k41 = i1 / BM;
    // input loader: lanes 4j..4j+3 fetch 64 contiguous bytes of channel row k = j; thread -> (k = (tid/4) % 16, output pixel pairs
    // n = 2 * (tid % 4 + 4 * wave + 16 u)).  Halo (threads 0..15): k = tid.
    const int b_k = (tid >> 2) & 15, b_n4 = (tid & 3) + 4 * wv;
    const int h_k = tid & 15;
    const float* xrow = P.x + (size_t)bz * P.xbs + (size_t)b_k * hw_in;
    const float* xrow_h = P.x + (size_t)bz * P.xbs + (size_t)h_k * hw_in;

    f32x16 acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    const int xq = (n0 + wv * 32 + l31) % W;                     // x of this lane's B column: the dx = -1 tap falls off the row at 0
    const int nchunk = (P.cin + CK - 1) / CK;
    const int G = nchunk * P.kh;                                 // groups = staged input tiles; each serves KW steps
    float4 ra0, ra1;
    struct RB { float4 v[NLB]; float halo; unsigned ok; };
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* wnext0 = P.wp + ((size_t)a_k40 * P.coP + a_m0) * 4;
    const float* wnext1 = P.wp + ((size_t)a_k41 * P.coP + a_m1) * 4;
    const size_t wstep = (size_t)4 * P.coP * 4;
    int lc = 0, ld = 0;                                          // (chunk, dy index) of the next group to load

    auto load_a = [&]() {                                        // next step's weights (the packing ends with one zero step)
        ra0 = *(const float4*)wnext0; ra1 = *(const float4*)wnext1;
        wnext0 += wstep; wnext1 += wstep;
    };
    // next group's input tile; advances (lc, ld).  Issued unconditionally: out-of-map lanes read a valid dummy address and are zeroed
    // when the tile is written to LDS.
    auto load_b = [&](RB& R) {
        R.ok = 0;
        const bool cok = lc * CK + b_k < P.cin;
        const float* src = xrow + (size_t)lc * CK * hw_in;
#pragma unroll
        for (int u = 0; u < NLB; ++u) {
            const int na = n0 + 2 * (b_n4 + 16 * u);
            const int y = na / W, x = na - y * W, yi = 2 * y + ld - ph;
            const bool ok = cok && na < hw && yi >= 0 && yi < P.Hin;
            R.v[u] = *(const float4*)(ok ? src + (size_t)yi * P.Win + 2 * x : P.x);
            R.ok |= ok ? (1u << u) : 0u;
        }
        if (tid < 16) {                                          // O[-1]: the input pixel left of the tile's first one
            const int y = n0 / W, x = n0 - y * W, yi = 2 * y + ld - ph;
            const bool ok = lc * CK + h_k < P.cin && x > 0 && yi >= 0 && yi < P.Hin;
            R.halo = *(ok ? xrow_h + (size_t)lc * CK * hw_in + (size_t)yi * P.Win + 2 * x - 1 : P.x);
            R.ok |= ok ? (1u << NLB) : 0u;
        }
        if (++ld == P.kh) { ld = 0; ++lc; }
    };
    auto store_a = [&](int buf) {
        *(float4*)&As[buf][a_m0][4 * a_k40] = ra0;
        *(float4*)&As[buf][a_m1][4 * a_k41] = ra1;
    };
    auto store_b = [&](const RB& R, int buf) {
#pragma unroll
        for (int u = 0; u < NLB; ++u) {
            const int n = 2 * (b_n4 + 16 * u);
            const float4 v = (R.ok >> u) & 1 ? R.v[u] : zero4;
            Bs[buf][n][b_k] = v.x; Bs[buf][BN + 1 + n][b_k] = v.y; Bs[buf][n + 1][b_k] = v.z; Bs[buf][BN + 2 + n][b_k] = v.w;
        }
        if (tid < 16) Bs[buf][BN][h_k] = (R.ok >> NLB) & 1 ? R.halo : 0.0f;
    };
    // One step = 16 k-values of one tap = two halves of 12 MFMAs, scheduled as in k_conv_igemm: half 1 runs on fragments read during the
    // previous step, the next tile goes to LDS and the barrier sits between the halves, the next step's first-half fragments are read
    // right behind it.
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 a0h1, a1h1, a2h1, bh1, a0h2, a1h2, a2h2, bh2;
    auto brow_of = [&](int dx) { return wv * 32 + l31 + (dx == 0 ? 0 : dx < 0 ? BN : BN + 1); };   // in[2x-1] = O[n-1], in[2x] = E[n], in[2x+1] = O[n]
    auto read_h1 = [&](int bufA, int bufB, int dx) {
        const float* arow = &As[bufA][l31][8 * lh];
        const float* brow = &Bs[bufB][brow_of(dx)][8 * lh];
        a0h1 = *(const f32x4*)(arow); a1h1 = *(const f32x4*)(arow + 32 * KS); a2h1 = *(const f32x4*)(arow + 64 * KS);
        bh1 = *(const f32x4*)(brow);
    };
    auto read_h2 = [&](int bufA, int bufB, int dx) {
        const float* arow = &As[bufA][l31][8 * lh + 4];
        const float* brow = &Bs[bufB][brow_of(dx)][8 * lh + 4];
        a0h2 = *(const f32x4*)(arow); a1h2 = *(const f32x4*)(arow + 32 * KS); a2h2 = *(const f32x4*)(arow + 64 * KS);
        bh2 = *(const f32x4*)(brow);
    };
    auto mma_half = [&](const f32x4& a0, const f32x4& a1, const f32x4& a2, const f32x4& b, int dx) {
        const bool v = dx >= 0 || xq > 0;
        float fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = v ? b[j] : 0.0f;      // column mask at use, not at the read
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], fb[j], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], fb[j], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[j], fb[j], acc[2], 0, 0, 0);
        }
    };

    {
        RB R;
        load_a(); load_b(R);
        store_a(0); store_b(R, 0);
        __syncthreads();
        read_h1(0, 0, -1);
        int step = 0;
        for (int g = 0; g < G; ++g) {
            const int curB = g & 1;
#pragma unroll
            for (int t = 0; t < KW; ++t, ++step) {
                const int curA = step & 1;
                const bool last = (g + 1 == G) && (t + 1 == KW);
                load_a();                                         // weights first: their wait must not cover the
                if (t == 0) load_b(R);                            // input loads issued after them (in-order return)
                read_h2(curA, curB, t - 1);
                SCHED_FENCE();
                mma_half(a0h1, a1h1, a2h1, bh1, t - 1);
                SCHED_FENCE();
                if (!last) store_a(curA ^ 1);
                if (t == KW - 1 && g + 1 < G) store_b(R, curB ^ 1);
                __syncthreads();
                if (!last) read_h1(curA ^ 1, t == KW - 1 ? curB ^ 1 : curB, t == KW - 1 ? -1 : t);
                SCHED_FENCE();
                mma_half(a0h2, a1h2, a2h2, bh2, t - 1);
                SCHED_FENCE();
            }
        }
    }

    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    float* red = &As[0][0][0];                                   // [4 waves][BM][3] (sum d, sum d^2, pivot): nothing reads the tiles after the last barrier
    static_assert(4 * 3 <= 2 * KS, "statistics scratch must fit the weights tiles");
    const int px = n0 + wv * 32 + l31;
    const bool pok = px < hw;
    const int py = px / W;
    const bool inx = !VALID || (pok && py < P.Hv && px - py * W < P.Wv);
    const unsigned long long inmask = VALID ? __ballot(inx) : 0ull;
    float* outb = P.out + (size_t)bz * P.obs;
    const bool relu = P.mode == RPE_CONV_RELU;
    auto epilogue = [&](auto statsc) {
        constexpr bool STATS = decltype(statsc)::value;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int row0 = i * 32 + 4 * lh;
#pragma unroll
            for (int rb = 0; rb < 16; rb += 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + r + 8 * (rb >> 2);
                    const float2 s2 = *(const float2*)&sbt[row][0];
                    float v = fmaf(acc[i][rb + r], s2.x, s2.y);
                    if (STATS) {                                 // k_conv_igemm's pivoted record of this 32-pixel block (see there)
                        const int vb = __builtin_bit_cast(int, v);
                        float piv = __builtin_bit_cast(float, lh ? __builtin_amdgcn_readlane(vb, 32) : __builtin_amdgcn_readlane(vb, 0));
                        if (VALID) piv = valid_pivot(v, inmask, lh);
                        const float dv = (pok && inx) ? v - piv : 0.0f;
                        float ssum = 0.0f, ssq = 0.0f;
                        ssum += dv; ssq = fmaf(dv, dv, ssq);
                        const float a = half_wave_sum(ssum), q = half_wave_sum(ssq);
                        float* rd = red + (wv * BM + row) * 3;
                        if (l31 == 31) { rd[0] = a; rd[1] = q; rd[2] = piv; }
                    }
                    if (relu) v = v < 0.0f ? 0.0f : v;
                    if (VALID) v = inx ? v : 0.0f;
                    if (pok) outb[(size_t)row * hw + px] = v;
                }
            }
        }
    };
    if (P.stats) epilogue(std::integral_constant<bool, true>{}); else epilogue(std::integral_constant<bool, false>{});
    if (P.stats) {                                               // one record per 32-pixel block of the plane, as in either class of k_conv_igemm
        __syncthreads();
        const int nrec = (hw + 31) / 32;
        if (tid < BM) {
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) {
                const int blk = (n0 + w2 * 32) >> 5;
                if (blk >= nrec) continue;
                int nw = hw - blk * 32; nw = nw > 32 ? 32 : nw;                            // valid columns of the block (>= 1)
                if (VALID) nw = valid_before(blk * 32 + nw, W, P.Hv, P.Wv) - valid_before(blk * 32, W, P.Hv, P.Wv);
                const float* rd = red + (w2 * BM + tid) * 3;
                StatAcc A;
                A.add_pivoted(nw, rd[0], rd[1], rd[2]);
                float* st = P.stats + (((size_t)bz * P.cout + tid) * nrec + blk) * 3;
                st[0] = (float)A.n; st[1] = (float)A.mean; st[2] = (float)A.m2;
            }
        }
    }
}

int conv_s2_m96_launch(const ConvP& P, int batch, hipStream_t stream, bool valid) {
    if (valid) hipLaunchKernelGGL(k_conv_s2_m96<true>, dim3(ceil_div(P.hw, 128), 1, batch), dim3(256), 0, stream, P);
    else hipLaunchKernelGGL(k_conv_s2_m96<false>, dim3(ceil_div(P.hw, 128), 1, batch), dim3(256), 0, stream, P);
    return rpe_check_launch();
}
