// The softmax of the convex 8x up-sampling's nine mask logits (core/RAFT/core/raft.py RAFT.upsample_flow), shared by the forward
// (raft_ops.hip: k_upsample_convex) and its backward (raft_backward.hip), so the backward's weights have the forward's bits.
#pragma once
#include "rpe_common.h"

// e[k] = exp(m[k] - mx) in double for the nine logits m of one sub-pixel, mx = their maximum; sum (0.0 on entry) = the sum of e in k
// order.  A macro, not a function: an inlined function reaches the same arithmetic but lets the compiler commute the operands of the sum's
// additions, and the forward's object file is held byte for byte.
#define CONVEX_SOFTMAX9(m, mx, e, sum) \
    _Pragma("unroll") for (int k = 0; k < 9; ++k) { e[k] = exp((double)m[k] - (double)mx); sum += e[k]; }
