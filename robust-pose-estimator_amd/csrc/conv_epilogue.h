// The update-block epilogue of rpe_conv_fused (include/rpe.h: bias, context addend, ReLU / tanh, the GRU gates with hidden / zgate, out2) for
// four accumulator rows of one pixel column: conv.hip's k_conv_igemm and conv_f16.hip's k_conv_f16 both finish their tiles with it, so the
// fp16-operand route differs from the f32 one in its products alone.  The rows are the four consecutive output channels co_first .. +3 that a
// lane of a 32x32 matrix-core tile holds in registers r .. r+3 (row = (r&3) + 8*(r>>2) + 4*(lane>>5)); loads first, then arithmetic, then
// masked stores (per-element validity branches made the compiler emit load - wait - store per element).
#pragma once
#include "rpe_common.h"

struct ConvEpi {
    const float* bias;                        // [cout] or null
    const float* addb;                        // this batch item's (cout, hw) pre-activation addend or null
    const float* hb;                          // ... hidden state (gates)
    const float* zb;                          // ... update gate (GATE_H)
    float* outb;                              // ... destination slice
    float* out2b;                             // ... second destination or null
    int mode, cg, cout, hw;
};

__device__ __forceinline__ void conv_epilogue_rows4(const ConvEpi& E, float a0, float a1, float a2, float a3, int co_first, int px, bool pok) {
    const float acc[4] = {a0, a1, a2, a3};
    const int mode = E.mode, cg = E.cg, hw = E.hw;
    size_t e[4]; bool ok[4]; float av[4], bv[4], xv[4], yv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = co_first + r;
        ok[r] = pok && co < E.cout;
        e[r] = ok[r] ? (size_t)co * hw + px : 0;
        bv[r] = E.bias ? E.bias[ok[r] ? co : 0] : 0.0f;
        av[r] = E.addb ? E.addb[e[r]] : 0.0f;
    }
    const bool rrows = co_first >= cg;                    // (GATE_ZR; uniform per group when cg % 4 == 0)
    if (mode == RPE_CONV_GATE_ZR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[r] = E.hb[(rrows && ok[r]) ? e[r] - (size_t)cg * hw : 0];
    } else if (mode == RPE_CONV_GATE_H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { xv[r] = E.zb[e[r]]; yv[r] = E.hb[e[r]]; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = acc[r] + av[r] + bv[r];
        if (mode == RPE_CONV_GATE_ZR) {
            const float sg = sigmoid_f(v);
            if (ok[r]) { if (rrows) E.out2b[e[r] - (size_t)cg * hw] = sg * xv[r]; else E.outb[e[r]] = sg; }
        } else if (mode == RPE_CONV_GATE_H) {
            if (ok[r]) E.outb[e[r]] = (1.0f - xv[r]) * yv[r] + xv[r] * tanh_f(v);
        } else {
            if (mode == RPE_CONV_RELU) v = v < 0.0f ? 0.0f : v;    // NaN stays NaN, like torch.relu
            else if (mode == RPE_CONV_TANH) v = tanh_f(v);
            if (ok[r]) { E.outb[e[r]] = v; if (E.out2b) E.out2b[e[r]] = v; }
        }
    }
}
