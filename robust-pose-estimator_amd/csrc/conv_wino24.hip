// 3x3 stride-1 "same" convolutions as Winograd F(2x4, 3x3) on the f32 matrix cores: F(2,3) along H, F(4,3) along W.
//
// The same layers, descriptor and epilogues as conv_wino.hip (F(2x2,3x3)): the update block's convc2 / convf2 / conv / FlowHead.conv1
// and mask head (core/RAFT/core/update.py) and the encoders' stride-1 residual convolutions (core/RAFT/core/extractor.py).
//     Y = A^T [ sum_ci U .* V ] A,   U = Gy g Gx^T (packed once, f64 rounded once),  V = By^T d Bx
// per 2 x 4 output tile: d = the 4 x 6 input patch; 24 element-wise products (positions) per tile = 1/3 product per output against
// F(2x2)'s 4/9: a quarter fewer matrix instructions.  Along W the points are {0, 1, -1, 1/2, -2} (+ infinity):
//     Bx^T = [2 -3 -4 3 2 0; 0 -2 1 5 2 0; 0 -2 5 -1 -2 0; 0 2 1 -2 -1 0; 0 1 -2 -1 2 0; 0 2 -3 -4 3 2]   (integers: exact products)
//     Ax^T = [1 1 1 1 1 0; 0 1 -1 1/2 -2 0; 0 1 1 1/4 4 0; 0 1 -1 1/8 -8 1]                                (powers of two)
//     Gx   = [1/2 0 0; 1/6 1/6 1/6; 1/6 -1/6 1/6; 16/15 8/15 4/15; 1/30 -1/15 2/15; 0 0 1/2]
// With these points the f32 pipeline's error is about a serial direct f32 sum's (tools/winograd_numerics.py: max 2.1e-5 against 2.2e-5
// on 256-channel sums; with {0, +-1, +-2}: 2.6e-5).  Along H: conv_wino.hip's F(2,3) (points 0, +-1).
//
// Workgroup = 4 waves = 64 output channels x 16 tiles = the 16 x 8 output pixels of conv_wino.hip's workgroup: the same grid, the same
// raw input patch (4 channels x 10 rows x 18 columns per step, one 16-byte-quad LDS-DMA per wave) and the same moment-record regions.
// Wave = 16 channels x 16 tiles x 24 positions = one v_mfma_f32_16x16x4_f32 block per position: 96 accumulators, so two waves per SIMD
// stay resident.  Per step of 4 input channels: 24 matrix instructions per wave (F(2x2): 32), 6 + 6 fragment reads of 16 B.
// U (4 x 64 x 24 floats = 24 KB a step) needs a two-deep ring to keep the workgroup within half the CU's LDS; it is requested one step
// ahead, the raw patch (three-deep ring) three.  Transform: thread = (row xi of By^T, input channel, tile): the two patch rows of its
// row combination (16-byte + 8-byte reads), then Bx^T; it stores its 6 positions as one 16-byte + one 8-byte write.
// CB = 1 (32 output channels: small launches, the trailing 32 channels of cout = 96): 4 waves = 2 x 16 channels x 2 halves of the 24
// positions, 12 accumulator chains per wave (at batch 1 a 24-long chain per wave left the launch latency-bound: 1.44x F(2x2)'s time);
// the wave pair swaps halves through LDS before the output transform.  Every accumulator is the same chain of matrix instructions and
// every output the same transform in either class (tested bitwise).
#include "wino_common.h"
#include <type_traits>

#define W4_CO 64
#define W4_NT 16                     // tiles per workgroup: 4 across x 4 down
#define W4K 4
#define W4_NP 24                     // positions per tile
#define W4_PS 28                     // floats per (ci, tile) row of V in LDS: 24 + 4 pad (16 rows 112 B apart cover the 64 banks once)
#define W4_RAW 1024                  // floats per raw-patch buffer: 240 quads of the 4 x 10 x 24-float patch (+ the landing shift)

struct Wino24P {
    const float* x; long long xbs;
    const float* wp; int cin, cout, coP, H, W;
    const float* bias;
    float* out; long long obs;
    float* out2; long long o2bs;
    int mode;
    const float* scale; const float* res; long long rbs; float* stats; const float* pre;
    int co_base;
    int Hv, Wv;                                   // valid extent (VALID instantiation, see conv_wino.hip): zero is stored outside it
};

// three 1 KB chunks: global base + voff + 1024 j  ->  LDS lds_addr + 1024 j + lane * 16
__device__ __forceinline__ void dma16x3(const float* base, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    base = wave_uniform(base);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:2048\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds_addr) : "memory");
}

// sum over each 8-lane half of a 16-lane row (DPP): every lane ends with its half's total
__device__ __forceinline__ float row8_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    return v;
}

// Position layout of a (ci, channel | tile) row: 16-byte slot s < 4 = (xi = s, nu = 0..3); slot 4 = (0, 4) (0, 5) (1, 4) (1, 5);
// slot 5 = (2, 4) (2, 5) (3, 4) (3, 5).  A transform thread (row xi) thus writes slot xi whole and half of slot 4 + xi / 2.
// In U, row r keeps logical slot s in physical slot (s + ((r >> 3) & 1)) % 6: the 16 rows of a fragment read (96 B apart) then
// cover the 64 banks once.
__host__ __device__ constexpr int w4_phys(int slot, int row) { return (slot + ((row >> 3) & 1)) % 6; }

// EPI as conv_wino.hip: 0 bias / ReLU / out2; 1 + scale and residual; 2 + moments; 3 all at run time.  Needs W % 4 == 0, even H and
// 16-byte aligned planes (the host checks).
template <int EPI, bool PRE, int CB, bool VALID = false>
__global__ __launch_bounds__(256, 2) void k_conv_wino24(Wino24P P) {
    constexpr bool HAS_AFFINE = EPI == 1 || EPI == 3, HAS_STATS = EPI == 2 || EPI == 3;
    constexpr bool VPRE = VALID && PRE;                                      // (conv_wino.hip: the raw patch outside the valid extent gets the padding value)
    constexpr int NW = 4, TCO = 32 * CB, UT_STEP = W4K * TCO * W4_NP;
    constexpr int NRAW = 1;                                                  // raw-patch DMA instructions per wave and step
    constexpr int NG = 3 * CB;                                               // groups of 4 positions per wave (CB = 1: half of them)
    constexpr int NUD = 3 * CB;                                              // weight DMA instructions (1 KB) per wave and step
    __shared__ __attribute__((aligned(16))) float Us[2][UT_STEP];            // [ci][co][24 positions, slots swizzled]
    __shared__ __attribute__((aligned(16))) float Vs[2][W4K][W4_NT][W4_PS];  // [ci][tile][positions]
    __shared__ __attribute__((aligned(16))) float Rs[3][W4_RAW];             // raw input patches [ci][row][24 columns]
    __shared__ float Pn[PRE ? 2 * 128 : 2];
    static_assert(sizeof(Us) + sizeof(Vs) + sizeof(Rs) + sizeof(Pn) <= 81920, "two workgroups per CU: at most half of the 160 KB LDS each");
    asm volatile("" :: "s"(P.x), "s"(P.wp), "s"(P.out), "s"(P.bias), "s"(P.xbs), "s"(P.obs), "s"(P.cin), "s"(P.cout), "s"(P.coP), "s"(P.H),
                 "s"(P.W), "s"(P.co_base), "s"(P.mode), "s"(P.out2), "s"(P.o2bs));
    if (EPI != 0) asm volatile("" :: "s"(P.scale), "s"(P.res), "s"(P.rbs), "s"(P.stats), "s"(P.pre));
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ptx = (P.W + 15) / 16;
    const int pid = (gridDim.x & 7) == 0 ? (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int x0 = (pid % ptx) * 16, y0 = (pid / ptx) * 8;
    const int co0 = P.co_base + blockIdx.y * TCO, bz = blockIdx.z;
    const int H = P.H, W = P.W, hw = H * W;
    const float* xb = P.x + (size_t)bz * P.xbs;
    const int nsteps = P.cin / W4K;

    // ---- raw patch DMA: quad q = 64 (NW j + wave) + lane -> (ci, row, quad column) of the 4 x 10 x 6 quads (map columns x0 - 4 ..
    // x0 + 19), landing 4 bytes into the buffer (patch column 0 = map column x0 - 1 on a 16-byte boundary).  Out-of-map quads read a
    // clamped in-map quad and are overwritten with the padding value once landed (patch_raw); lanes past quad 239 are masked off.
    unsigned roff[NRAW];
    unsigned oob = 0;
#pragma unroll
    for (int j = 0; j < NRAW; ++j) {
        const int q0 = 64 * (NW * j + wv) + lane, q = q0 < 240 ? q0 : 239;
        const int ci = q / 60, rem = q - ci * 60, r = rem / 6, qc = rem - r * 6;
        int yy = y0 - 1 + r, xx = x0 - 4 + 4 * qc;
        if (q0 < 240 && (yy < 0 || yy >= H || xx < 0 || xx >= W)) oob |= VPRE ? 0xFu : 1u << j;
        else if (VPRE && q0 < 240) {                          // an in-map quad: bit e = its element e lies outside the valid extent
#pragma unroll
            for (int e = 0; e < 4; ++e) oob |= (yy >= P.Hv || xx + e >= P.Wv) ? 1u << e : 0u;
        }
        yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy); xx = xx < 0 ? 0 : (xx >= W ? W - 4 : xx);
        roff[j] = (unsigned)(ci * hw + yy * W + xx) * 4u;
    }
    const bool border = (y0 < 1) | (y0 + 8 >= H) | (x0 < 1) | (x0 + 16 >= W) |       // workgroup-uniform
                        (VPRE && ((y0 + 8 >= P.Hv) | (x0 + 16 >= P.Wv)));
    static_assert(NRAW == 1, "VPRE keeps the quad's four element bits in oob");
    const float padv = PRE ? -__builtin_inff() : 0.0f;                              // relu((-inf - mean) / std) = 0
    auto patch_raw = [&](int buf) {
        if (border) {
#pragma unroll
            for (int j = 0; j < NRAW; ++j)
                if (VPRE ? oob != 0 : (oob >> j) & 1) {
                    float* q4 = &Rs[buf][4 * (64 * (NW * j + wv) + lane) + 1];
                    if (VPRE) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if ((oob >> e) & 1) q4[e] = padv;
                    } else { q4[0] = padv; q4[1] = padv; q4[2] = padv; q4[3] = padv; }
                }
        }
    };
    // packed weights: [step][64-channel tile][ci][co % 64][24].  CB = 2: the workgroup's 24 KB of a step are contiguous, wave = 6 KB of
    // it; CB = 1: the 32 rows of channel ci start at row co0 % 64 (3 KB), wave = input channel wave
    const float* wslice = P.wp + (size_t)(co0 / W4_CO) * (W4K * W4_CO * W4_NP) +
                          (CB == 2 ? (size_t)wv * 1536 : (size_t)wv * (W4_CO * W4_NP) + (size_t)(co0 % W4_CO) * W4_NP);
    const unsigned uoff = lane * 16u;
    const size_t wstep = (size_t)(P.coP / W4_CO) * (W4K * W4_CO * W4_NP), rstep = (size_t)W4K * hw;
    const unsigned us_base = lds_addr_of(&Us[0][0]) + (unsigned)wv * (CB == 2 ? 6144u : 3072u);
    const unsigned rs_base = lds_addr_of(&Rs[0][0]) + (unsigned)wv * 1024u + 4u;
    auto dma_u = [&](const float* src, int buf) {
        const unsigned l = us_base + (unsigned)buf * (UT_STEP * 4u);
        dma16x3(src, uoff, l);
        if (CB == 2) dma16x3(src + 768, uoff, l + 3072u);
    };
    auto dma_raw = [&](const float* src, int buf) {
#pragma unroll
        for (int j = 0; j < NRAW; ++j)
            dma16x1_masked(src, roff[j], rs_base + (unsigned)buf * (W4_RAW * 4u) + (unsigned)(j * NW) * 1024u,
                           NW * j + wv == 3 ? 0x0000FFFFFFFFFFFFull : ~0ull);
    };
    auto clamped = [&](int step) { return step < nsteps ? step : nsteps - 1; };    // (past the end: a harmless repeat)

    // ---- transform role: thread -> (row xi of By^T, input channel, tile).  By^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 -1 0 1]: row xi
    // is t = d[rP] + sigma d[rQ] with (rP, rQ, sigma) = (0, 2, -1) (1, 2, +1) (2, 1, -1) (3, 1, -1) (exact: sigma = +-1).
    const int v_ci = (lane >> 4) & 3, v_tile = lane & 15, v_tx = v_tile & 3, v_ty = v_tile >> 2;
    const int v_base = v_ci * 240 + 2 * v_ty * 24 + 4 * v_tx + 4;                  // patch column 4 tx, its 16-byte-aligned float index
    float td[12], tt[6], tv[6];
    float2 pn = make_float2(0.0f, 1.0f);
    auto tr_read = [&](int step, int k, auto rbufc) {
        constexpr int rbuf = decltype(rbufc)::value;
        const float* rp = &Rs[rbuf][0];
        const int xi = wv + 4 * k, rP = xi, rQ = xi < 2 ? 2 : 1;
        const f32x4 p4 = *(const f32x4*)(rp + v_base + rP * 24), q4 = *(const f32x4*)(rp + v_base + rQ * 24);
        const float2 p2 = *(const float2*)(rp + v_base + rP * 24 + 4), q2 = *(const float2*)(rp + v_base + rQ * 24 + 4);
        td[0] = p4[0]; td[1] = p4[1]; td[2] = p4[2]; td[3] = p4[3]; td[4] = p2.x; td[5] = p2.y;
        td[6] = q4[0]; td[7] = q4[1]; td[8] = q4[2]; td[9] = q4[3]; td[10] = q2.x; td[11] = q2.y;
        if (PRE && k == 0) pn = *(const float2*)&Pn[2 * (step * W4K + v_ci)];   // (-mean / std, 1 / std)
    };
    auto tr_rows = [&](int k) {
        const float sigma = (wv + 4 * k) == 1 ? 1.0f : -1.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            float p = td[c], q = td[6 + c];
            if (PRE) { p = fmaxf(fmaf(p, pn.y, pn.x), 0.0f); q = fmaxf(fmaf(q, pn.y, pn.x), 0.0f); }
            tt[c] = fmaf(sigma, q, p);
        }
    };
    auto tr_cols = [&]() {                                    // v = Bx^T t
        const float* t = tt;
        const float a = t[1] - t[3], b = t[2] - t[4];
        tv[0] = fmaf(2.0f, t[0], fmaf(-3.0f, t[1], fmaf(-4.0f, t[2], fmaf(3.0f, t[3], 2.0f * t[4]))));
        tv[1] = fmaf(-2.0f, t[1], fmaf(5.0f, t[3], fmaf(2.0f, t[4], t[2])));
        tv[2] = fmaf(-2.0f, t[1], fmaf(5.0f, t[2], fmaf(-2.0f, t[4], -t[3])));
        tv[3] = fmaf(2.0f, a, b);
        tv[4] = fmaf(-2.0f, b, a);
        tv[5] = fmaf(2.0f, t[1], fmaf(-3.0f, t[2], fmaf(-4.0f, t[3], fmaf(3.0f, t[4], 2.0f * t[5]))));
    };
    auto tr_store = [&](int vbuf, int k) {
        const int xi = wv + 4 * k;
        float* row = &Vs[vbuf][v_ci][v_tile][0];
        *(f32x4*)(row + 4 * xi) = (f32x4){tv[0], tv[1], tv[2], tv[3]};
        *(float2*)(row + 16 + 2 * xi) = make_float2(tv[4], tv[5]);
    };

    f32x4 acc[4 * NG];
#pragma unroll
    for (int p = 0; p < 4 * NG; ++p) acc[p] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    const int li = lane & 15, lk = lane >> 4;
    // wave -> 16 output channels (cw) and its position groups: CB = 2 all six; CB = 1 the wave pair (cw, ph = 0 | 1) splits them, groups
    // 3 ph .. 3 ph + 2 (every accumulator is the same chain of matrix instructions as in the CB = 2 class)
    const int cw = CB == 2 ? wv : (wv & 1), ph = CB == 2 ? 0 : (wv >> 1);
    float bi_[4], sc_[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = co0 + cw * 16 + 4 * lk + r;
        const int cc = co < P.cout ? co : P.cout - 1;
        bi_[r] = P.bias ? P.bias[cc] : 0.0f;
        sc_[r] = (HAS_AFFINE && P.scale) ? P.scale[cc] : 1.0f;
    }

    // ---- prologue: U(0), raw(0), raw(1), U(1), raw(2) requested at once; wait for the first three groups, V(0), then raw(3)
    const float* xsrc = xb;
    dma_u(wslice, 0); dma_raw(xsrc, 0); dma_raw(xsrc + (size_t)clamped(1) * rstep, 1);
    dma_u(wslice + (size_t)clamped(1) * wstep, 1); dma_raw(xsrc + (size_t)clamped(2) * rstep, 2);
    if (PRE) {
        for (int i = tid; i < P.cin; i += 64 * NW) {
            const float m = P.pre[((size_t)bz * P.cin + i) * 2], iv = P.pre[((size_t)bz * P.cin + i) * 2 + 1];
            Pn[2 * i] = -m * iv; Pn[2 * i + 1] = iv;
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70 | (NUD + NRAW));                                   // vmcnt(U(1) + raw(2) still in flight)
    patch_raw(0); patch_raw(1);
    __builtin_amdgcn_s_waitcnt(0xC07F);                                                // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    tr_read(0, 0, std::integral_constant<int, 0>{}); tr_rows(0); tr_cols(); tr_store(0, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();                                                      // V(0) visible; raw(0)'s buffer free
    dma_raw(xsrc + (size_t)clamped(3) * rstep, 0);
    const float* unext = wave_uniform(wslice + (size_t)clamped(2) * wstep);           // U(s + 2), raw(s + 4) of the step the loop is in
    const float* rnext = wave_uniform(xsrc + (size_t)clamped(4) * rstep);

    // fragment offsets (floats): U row (ci = lk, channel cw * 16 + li), the wave's slots swizzled; V row (ci = lk, tile = li)
    const int urow = (lk * TCO + cw * 16 + li) * W4_NP, voffl = (lk * W4_NT + li) * W4_PS;
    int uslot[NG], vslot[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { uslot[g] = urow + 4 * w4_phys(3 * ph + g, li); vslot[g] = voffl + 4 * (3 * ph + g); }
    f32x4 fa = *(const f32x4*)&Us[0][uslot[0]], fb = *(const f32x4*)(&Vs[0][0][0][0] + vslot[0]);
    auto mfma_group = [&](int g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], fb[e], acc[4 * g + e], 0, 0, 0);
    };
    // ---- step s: NG groups of 4 matrix instructions (one per four positions); beside them (CB = 2):
    //   g0 | fragment reads of g1, patch reads of raw(s+1)     g1 | fragment reads of g2, row pass     g2 | g3's, column pass
    //   g3 | g4's, V(s+1) stored     g4 | g5's | wait: own DMAs but the newest raw group landed, border patch of raw(s+2), BARRIER
    //   g5 | fragment reads of g0 of step s+1 | DMA U(s+2) -> U(s)'s buffer, raw(s+4) -> raw(s+1)'s
    // CB = 1 (three groups): g0 | g1's reads, patch reads     g1 | g2's reads, the whole transform, wait, BARRIER     g2 | as g5
    auto step = [&](auto curc, auto rbc, const int s) {
        constexpr int CUR = decltype(curc)::value, RB = decltype(rbc)::value, RB1 = (RB + 1) % 3, RB2 = (RB + 2) % 3;
        const float* ua = &Us[CUR][0];
        const float* vb = &Vs[CUR][0][0][0];
        const int tstep = s + 1 < nsteps ? s + 1 : nsteps - 1;
        f32x4 na, nb;
        auto frag_reads = [&](const float* u, const float* v, int g) {
            na = *(const f32x4*)(u + uslot[g]);
            nb = *(const f32x4*)(v + vslot[g]);
        };
        frag_reads(ua, vb, 1);
        tr_read(tstep, 0, std::integral_constant<int, RB1>{});
        __builtin_amdgcn_sched_barrier(0);
        mfma_group(0);
        __builtin_amdgcn_sched_barrier(0);
        fa = na; fb = nb;
        frag_reads(ua, vb, 2);
        __builtin_amdgcn_sched_barrier(0);
        tr_rows(0);
        if constexpr (CB == 1) { tr_cols(); tr_store(CUR ^ 1, 0); }
        __builtin_amdgcn_sched_barrier(0);
        mfma_group(1);
        __builtin_amdgcn_sched_barrier(0);
        fa = na; fb = nb;
        if constexpr (CB == 2) {
            frag_reads(ua, vb, 3);
            __builtin_amdgcn_sched_barrier(0);
            tr_cols();
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(2);
            __builtin_amdgcn_sched_barrier(0);
            fa = na; fb = nb;
            frag_reads(ua, vb, 4);
            __builtin_amdgcn_sched_barrier(0);
            tr_store(CUR ^ 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(3);
            __builtin_amdgcn_sched_barrier(0);
            fa = na; fb = nb;
            frag_reads(ua, vb, 5);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(4);
            __builtin_amdgcn_sched_barrier(0);
            fa = na; fb = nb;
        }
        // own DMAs except the newest raw group have landed (U(s+1), raw(s+2)); V stores and this step's fragment reads are complete:
        // after the barrier U(s), V(s) and raw(s+1) may be overwritten
        __builtin_amdgcn_s_waitcnt(0x0F70 | NRAW);
        patch_raw(RB2);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        frag_reads(&Us[CUR ^ 1][0], &Vs[CUR ^ 1][0][0][0], 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[4 * (NG - 1) + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], fb[e], acc[4 * (NG - 1) + e], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (e == 0) { dma_u(unext, CUR); if (s + 3 < nsteps) unext += wstep; }
            if (e == 1) { dma_raw(rnext, RB1); if (s + 5 < nsteps) rnext += rstep; }
            __builtin_amdgcn_sched_barrier(0);
        }
        fa = na; fb = nb;
    };
    {
        typedef std::integral_constant<int, 0> I0; typedef std::integral_constant<int, 1> I1; typedef std::integral_constant<int, 2> I2;
        int s = 0;
        while (true) {
            step(I0{}, I0{}, s); if (++s == nsteps) break;
            step(I1{}, I1{}, s); if (++s == nsteps) break;
            step(I0{}, I2{}, s); if (++s == nsteps) break;
            step(I1{}, I0{}, s); if (++s == nsteps) break;
            step(I0{}, I1{}, s); if (++s == nsteps) break;
            step(I1{}, I2{}, s); if (++s == nsteps) break;
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                       // the repeats issued past the end have landed before LDS is released

    // ---- epilogue.  D layout: column (tile) = lane % 16, row (channel) = 4 (lane / 16) + r.  Lane-local Y = Ay^T M Ax:
    //   s_i[nu] = Ay^T rows [1 1 1 0] / [0 1 -1 1] over xi; y_i = Ax^T s_i; two 16-byte rows per channel
    const int ty = li >> 2, tx = li & 3;
    const int oy = y0 + 2 * ty, ox = x0 + 4 * tx;
    const bool pix_ok = (oy < H) & (ox < W);                  // (H even, W % 4 == 0: a tile is inside or outside as a whole)
    float* ob = P.out + (size_t)bz * P.obs;
    float* ob2 = P.out2 ? P.out2 + (size_t)bz * P.o2bs : nullptr;
    const float* rsb = (HAS_AFFINE && P.res) ? P.res + (size_t)bz * P.rbs : nullptr;
    const unsigned long long vmask = __ballot(pix_ok);
    const int hf = li >> 3;                                   // moment record: top (tiles 0-7) or bottom (8-15) 16 x 4 pixels
    float nvalid = 8.0f * (float)__popcll((vmask >> (8 * hf)) & 0xFFull);
    // VALID: which of the tile's 2 x 4 pixels lie inside the valid extent -- the moments cover those only
    bool ev[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) ev[i][e] = pix_ok && (!VALID || (oy + i < P.Hv && ox + e < P.Wv));
    if (VALID && HAS_STATS) {
        nvalid = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) nvalid += (float)__popcll((__ballot(ev[i][e]) >> (8 * hf)) & 0xFFull);
    }
    const float inv_nvalid = nvalid > 0.0f ? 1.0f / nvalid : 0.0f;
    // CB = 1: the wave pair exchanges halves through LDS (U's buffers, free now): wave ph finishes channel rows 2 ph, 2 ph + 1 and hands
    // its partner (wave ^ 2) the other two rows of its 12 positions.  xr[2 p + rr] = the partner's position p of row 2 ph + rr.
    float xr[CB == 1 ? 24 : 1];
    if constexpr (CB == 1) {
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_s_barrier();                         // every wave is past its last fragment read, its DMAs have landed
        f32x4* X = (f32x4*)&Us[0][0];
        static_assert(sizeof(Us) >= 4 * 6 * 64 * 16, "exchange buffer");
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const f32x4 a = acc[2 * j], b = acc[2 * j + 1];
            X[(wv * 6 + j) * 64 + lane] = ph ? (f32x4){a[0], a[1], b[0], b[1]} : (f32x4){a[2], a[3], b[2], b[3]};
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const f32x4 q = X[((wv ^ 2) * 6 + j) * 64 + lane];
            xr[4 * j] = q[0]; xr[4 * j + 1] = q[1]; xr[4 * j + 2] = q[2]; xr[4 * j + 3] = q[3];
        }
    }
    float rec[3] = {0.0f, 0.0f, 0.0f};                        // lane li % 8 collects the record of channel row r = li % 8, half hf
    auto epilogue = [&](auto phc) {
        constexpr int PH = decltype(phc)::value, R0 = CB == 2 ? 0 : 2 * PH, NR = CB == 2 ? 4 : 2;
        f32x4 rq_[NR][2];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int co = co0 + cw * 16 + 4 * lk + R0 + rr;
            rq_[rr][0] = rq_[rr][1] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            if (HAS_AFFINE && rsb && pix_ok && co < P.cout) {
                const float* rp = rsb + (size_t)co * hw + (size_t)oy * W + ox;
                rq_[rr][0] = *(const f32x4*)rp; rq_[rr][1] = *(const f32x4*)(rp + W);
            }
        }
        auto M = [&](int xi, int nu, int r) -> float {        // position (xi, nu) of channel row r
            const int sl = nu < 4 ? xi : 4 + (xi >> 1), e = nu < 4 ? nu : 2 * (xi & 1) + (nu - 4);
            if (CB == 2) return acc[4 * sl + e][r];
            if (sl / 3 == PH) return acc[4 * (sl - 3 * PH) + e][r];
            return xr[2 * (4 * (sl - 3 * (1 - PH)) + e) + (r - R0)];
        };
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int r = R0 + rr;
            const int co = co0 + cw * 16 + 4 * lk + r;
            float y[2][4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float sv[6];
#pragma unroll
                for (int nu = 0; nu < 6; ++nu)
                    sv[nu] = i == 0 ? (M(0, nu, r) + M(1, nu, r)) + M(2, nu, r) : (M(1, nu, r) - M(2, nu, r)) + M(3, nu, r);
                const float a = sv[1] + sv[2], b = sv[1] - sv[2];
                y[i][0] = (sv[0] + a) + (sv[3] + sv[4]);
                y[i][1] = fmaf(0.5f, sv[3], fmaf(-2.0f, sv[4], b));
                y[i][2] = fmaf(0.25f, sv[3], fmaf(4.0f, sv[4], a));
                y[i][3] = fmaf(0.125f, sv[3], fmaf(-8.0f, sv[4], b)) + sv[5];
            }
            const bool cok = co < P.cout;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (HAS_AFFINE && P.scale) y[i][e] *= sc_[r];
                    y[i][e] += bi_[r];
                }
            if (HAS_STATS && (EPI == 2 || P.stats)) {
                // moments of v over this half's 8 tiles x 8 pixels about a pivot (the half's first value: valid whenever any of its tiles is)
                const int y0b = __builtin_bit_cast(int, y[0][0]);
                const float piv = __builtin_bit_cast(float, __shfl(y0b, lane & 0x38));
                float s1 = 0.0f, s2 = 0.0f;
                if (pix_ok) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (!VALID || ev[i][e]) { const float dv = y[i][e] - piv; s1 += dv; s2 += dv * dv; }
                }
                s1 = row8_sum(s1); s2 = row8_sum(s2);
                const float m = VALID ? (nvalid > 0.0f ? s1 / nvalid : 0.0f) : s1 * inv_nvalid;
                if ((li & 7) == r) { rec[0] = nvalid; rec[1] = (VALID && nvalid == 0.0f) ? 0.0f : piv + m; rec[2] = s2 - s1 * m; }   // (zero-count record: (0, 0, 0))
            }
            if (P.mode == RPE_CONV_RELU) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[i][e] = y[i][e] < 0.0f ? 0.0f : y[i][e];
            }
            if (pix_ok && cok) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    f32x4 q = {y[i][0], y[i][1], y[i][2], y[i][3]};
                    if (rsb) {                                       // ResidualBlock tail: relu(x + y)
                        q += rq_[rr][i];
#pragma unroll
                        for (int e = 0; e < 4; ++e) q[e] = q[e] < 0.0f ? 0.0f : q[e];
                    }
                    if (VALID) {                                     // selects: a NaN outside the extent leaves as zero
#pragma unroll
                        for (int e = 0; e < 4; ++e) q[e] = (oy + i < P.Hv && ox + e < P.Wv) ? q[e] : 0.0f;
                    }
                    const size_t e4 = (size_t)co * hw + (size_t)(oy + i) * W + ox;
                    *(f32x4*)(ob + e4) = q;
                    if (ob2) *(f32x4*)(ob2 + e4) = q;
                }
            }
        }
        if (HAS_STATS && (EPI == 2 || P.stats)) {
            const int co = co0 + cw * 16 + 4 * lk + (li & 7);
            if ((li & 7) >= R0 && (li & 7) < R0 + NR && co < P.cout) {
                float* st = P.stats + (((size_t)bz * (2 * gridDim.x) + 2 * pid + hf) * P.cout + co) * 3;      // (b, records, cout, 3)
                st[0] = rec[0]; st[1] = rec[1]; st[2] = rec[2];
            }
        }
    };
    if constexpr (CB == 2) epilogue(std::integral_constant<int, 0>{});
    else if (ph == 0) epilogue(std::integral_constant<int, 0>{});
    else epilogue(std::integral_constant<int, 1>{});
}

// weight (cout, cin, 3, 3) -> U = Gy g Gx^T in f64, rounded once, laid out [step = ci/4][co tile = co/64][ci%4][co%64][24: slot-swizzled]
__global__ void k_wino24_pack(const float* __restrict__ w, float* __restrict__ wp, int cout, int cin, int coP, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int pp = (int)(e % W4_NP);
    const long long rowi = e / W4_NP;
    const int col = (int)(rowi & 63), cil = (int)((rowi >> 6) & 3);
    const long long rest = rowi >> 8;
    const int ncot = coP / W4_CO;
    const int co = (int)(rest % ncot) * W4_CO + col, ci = (int)(rest / ncot) * W4K + cil;
    float v = 0.0f;
    if (co < cout && ci < cin) {
        int slot = 0;
        for (int s = 0; s < 6; ++s) if (w4_phys(s, col & 15) == pp / 4) slot = s;
        const int c4 = pp % 4;
        const int xi = slot < 4 ? slot : 2 * (slot - 4) + (c4 >> 1), nu = slot < 4 ? c4 : 4 + (c4 & 1);
        const double Gy[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        const double Gx[6][3] = {{0.5, 0, 0}, {1.0 / 6, 1.0 / 6, 1.0 / 6}, {1.0 / 6, -1.0 / 6, 1.0 / 6}, {16.0 / 15, 8.0 / 15, 4.0 / 15},
                                 {1.0 / 30, -1.0 / 15, 2.0 / 15}, {0, 0, 0.5}};
        const float* g = w + ((size_t)co * cin + ci) * 9;
        double u = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) u += Gy[xi][a] * (double)g[3 * a + b] * Gx[nu][b];
        v = (float)u;
    }
    wp[e] = v;
}

extern "C" size_t rpe_conv_wino24_packed_floats(int cout, int cin) {
    if (cout <= 0 || cin <= 0 || cin % W4K) return 0;
    return (size_t)(cin / W4K) * W4K * W4_NP * round_up(cout, W4_CO);
}

extern "C" int rpe_conv_wino24_pack(const float* weight, int cout, int cin, float* packed, void* stream) {
    return launch_pack(k_wino24_pack, weight, packed, cout, cin, W4K, (long long)rpe_conv_wino24_packed_floats(cout, cin), stream, round_up(cout, W4_CO));
}

static int conv_wino24_launch(const rpe_conv_desc* d, int hv, int wv, void* stream, bool enc = false) {
    if (!conv_desc_present(d)) return RPE_E_BADARG;
    // tiles of 2 x 4 outputs, and every map row moved as 16-byte quads
    if (d->kh != 3 || d->kw != 3 || !stride_is_1(d) || (d->cin % W4K) || (d->h & 1) || (d->w & 3)) return RPE_E_UNSUPPORTED;
    if (!conv_linear_or_relu(d) || !conv_plain_only(d)) return RPE_E_UNSUPPORTED;
    if (d->pre_norm && d->cin > 128) return RPE_E_UNSUPPORTED;                                  // LDS room for 128 (mean, 1/std) pairs of the input
    if (!aligned16(d->x, d->x_batch_stride) || !aligned16(d->out, d->out_batch_stride) || !aligned16(d->out2, d->out2_batch_stride) ||
        !aligned16(d->residual, d->residual_batch_stride) || !aligned16(d->packed, 0)) return RPE_E_UNSUPPORTED;
    Wino24P P;
    fill_common(P, d, round_up(d->cout, W4_CO)); fill_encoder(P, d);
    P.H = d->h; P.W = d->w; P.co_base = 0;
    const int epi = wino_epilogue_class(d);
    const unsigned gx = ceil_div(d->w, 16) * ceil_div(d->h, 8);
    const bool valid = hv != d->h || wv != d->w;               // a valid extent smaller than the map: the plain epilogue only
    if (valid && !enc && epi != 0) return RPE_E_UNSUPPORTED;
    P.Hv = hv; P.Wv = wv;
    auto launch = [&](auto cb, int tiles) {
        if (valid && enc) {                                   // rpe_enc_conv_wino24_v: every epilogue class and the normalising loader
            dispatch_epi_pre(epi, d->pre_norm != nullptr, [&](auto e, auto pre) {
                hipLaunchKernelGGL((k_conv_wino24<decltype(e)::value, decltype(pre)::value, decltype(cb)::value, true>), dim3(gx, tiles, d->b), dim3(256), 0,
                                   (hipStream_t)stream, P);
            });
            return;
        }
        if (valid) {
            hipLaunchKernelGGL((k_conv_wino24<0, false, decltype(cb)::value, true>), dim3(gx, tiles, d->b), dim3(256), 0, (hipStream_t)stream, P);
            return;
        }
        dispatch_epi_pre(epi, d->pre_norm != nullptr, [&](auto e, auto pre) {
            hipLaunchKernelGGL((k_conv_wino24<decltype(e)::value, decltype(pre)::value, decltype(cb)::value>), dim3(gx, tiles, d->b), dim3(256), 0,
                               (hipStream_t)stream, P);
        });
    };
    // small launches (sequential tracking): 32-channel tiles, as rpe_conv_wino (same threshold, same workgroup count)
    if ((long long)gx * ceil_div(d->cout, W4_CO) * d->b < WINO_SMALL_WG) launch(std::integral_constant<int, 1>{}, ceil_div(d->cout, 32));
    else launch_tiles64(P, launch);
    return rpe_check_launch();
}

extern "C" int rpe_conv_wino24(const rpe_conv_desc* d, void* stream) { return conv_wino24_launch(d, d ? d->h : 0, d ? d->w : 0, stream); }

extern "C" int rpe_conv_wino24_v(const rpe_conv_desc_v* dv, void* stream) {
    if (!dv || !conv_valid_extent_ok(dv)) return RPE_E_BADARG;
    return conv_wino24_launch(&dv->d, dv->h_valid, dv->w_valid, stream);
}

// The encoders' form (see rpe_enc_conv_wino_v).  Extent == map: literally rpe_conv_wino24's launch.
extern "C" int rpe_enc_conv_wino24_v(const rpe_conv_desc_v* dv, void* stream) {
    if (!dv || !conv_valid_extent_ok(dv)) return RPE_E_BADARG;
    return conv_wino24_launch(&dv->d, dv->h_valid, dv->w_valid, stream, true);
}
