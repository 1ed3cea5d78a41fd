// The tap arithmetic of the correlation window lookup, shared by the pyramid route (corr.hip) and the on-the-fly route (corr_alt.hip):
// both take the integer tap and the fraction of every window position from make_taps, so they cannot disagree on a discrete decision.
#pragma once
#include "rpe_common.h"
#include "sampling.h"

#define RADIUS 4
#define WIN 9            // 2r+1

// The 9 tap positions of one axis at one level.  Tap i reads pixels lo+i+dev_i and lo+i+dev_i+1 with weights
// (w0, w1); written as three weights over the pixels lo+i, lo+i+1, lo+i+2 so the inner loop has no selects:
//   dev_i = 0 -> (w0, w1, 0)      dev_i = 1 -> (0, w0, w1)      unusable tap -> (0, 0, 0)
struct TapAxis {
    int lo;                // min_i (floor(pos_i) - i)
    unsigned dev;          // bit i: floor(pos_i) - i == lo + 1
    unsigned bad;          // bit i: position not finite / deviation > 1 -> tap contributes zero
    float a0[WIN], a1[WIN], a2[WIN];
};

__device__ __forceinline__ void make_taps(float c, int size, TapAxis& T) {
    int f[WIN];
    float w0[WIN], w1[WIN];
    int lo = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < WIN; ++i) {
        float pos = rt_pos(rn_add(c, (float)(i - RADIUS)), size);     // centroid + delta, then grid_sample
        float pf;
        f[i] = safe_floor(pos, pf) - i;
        w1[i] = pos - pf;                                                // ix - ix_nw
        w0[i] = (pf + 1.0f) - pos;                                       // ix_se - ix
        lo = f[i] < lo ? f[i] : lo;
    }
    T.lo = lo; T.dev = 0; T.bad = 0;
#pragma unroll
    for (int i = 0; i < WIN; ++i) {
        const int e = f[i] - lo;
        const bool bad = e > 1 || lo < -500000;
        const bool dv = e == 1;
        if (dv) T.dev |= 1u << i;
        if (bad) T.bad |= 1u << i;
        T.a0[i] = (bad || dv) ? 0.0f : w0[i];
        T.a1[i] = bad ? 0.0f : (dv ? w0[i] : w1[i]);
        T.a2[i] = (bad || !dv) ? 0.0f : w1[i];
    }
}
