// What the implicit-GEMM convolution kernels (conv.hip: k_conv_igemm; conv_s2.hip: its 96-row stride-2 class) share: the parameter
// struct rpe_conv_fused fills, the step depth and the half-wave sum of the instance-norm statistics.
#pragma once
#include "rpe_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK 16
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)     /* nothing is scheduled across this point */

struct ConvP {
    const float* x; long long xbs;            // first input channel of the slice; batch stride (floats)
    const float* wp;                          // packed weights [step][16][coP]
    int cin, cout, coP, H, W, hw, kh;         // H, W, hw: OUTPUT map
    int Hin, Win;                             // input map (= H, W unless stride 2)
    const float* bias;                        // [cout] or null
    const float* add; long long abs_;         // (b, cout, hw) pre-activation addend or null
    int mode;
    float* out; long long obs;                // channel 0 of the destination slice; batch stride
    float* out2; long long o2bs;              // second destination (RPE_CONV_RELU/LINEAR: copy; GATE_ZR: r*h)
    const float* h; long long hbs;            // hidden state, channels [0, c)
    const float* z; long long zbs;            // update gate (GATE_H)
    int cgate;
    const float* scale;                       // [cout] or null: v = acc * scale + ...
    const float* res; long long rbs;          // residual added after the activation, then ReLU again (encoder blocks)
    float* stats;                             // [b][cout][tiles_n][2] partial (sum, sum of squares) of v, or null
    const float* pre;                         // [b][cin][2] (mean, 1/std) or null: the input is normalised + ReLU'd as it is staged
    int Hv, Wv;                               // valid extent of the OUTPUT map (the VALID stride-2 instantiations: rpe_enc_conv_s2_v)
};

// VALID: the pixels among the flattened pixels [0, p) of a map of row length W that lie inside its valid extent Hv x Wv
__device__ __forceinline__ int valid_before(int p, int W, int Hv, int Wv) {
    const int y = p / W, x = p - y * W;
    return y < Hv ? y * Wv + (x < Wv ? x : Wv) : Hv * Wv;
}
// VALID: the statistics pivot of a 32-lane half = the value of its first lane inside the extent (``inside`` = the wave's ballot; a half
// wholly outside takes its first lane, and its record's count is zero)
__device__ __forceinline__ float valid_pivot(float v, unsigned long long inside, int lh) {
    const unsigned lo = (unsigned)inside, hi = (unsigned)(inside >> 32);
    const int ilo = lo ? __builtin_ctz(lo) : 0, ihi = 32 + (hi ? __builtin_ctz(hi) : 0);
    const int vb = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, lh ? __builtin_amdgcn_readlane(vb, ihi) : __builtin_amdgcn_readlane(vb, ilo));
}


// Sum over each 32-lane half of the wave with DPP moves (VALU rate, no LDS traffic): quad butterflies, row half-mirror,
// row mirror, then lane 15 of each even 16-lane row is broadcast into the odd row.  Lanes 31 and 63 hold the totals.
__device__ __forceinline__ float half_wave_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, true));   // row_bcast:15 into rows 1, 3
    return v;
}

// conv_s2.hip: the 96-row class of the stride-2 3x3 layers (cout == 96, no residual / addend / second output); P as rpe_conv_fused fills it
int conv_s2_m96_launch(const ConvP& P, int batch, hipStream_t stream, bool valid = false);
