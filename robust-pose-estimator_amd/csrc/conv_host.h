// Host side shared by the convolution entry points that take an rpe_conv_desc (rpe_conv_fused, rpe_conv1x1[_x3], rpe_conv_wino[24|_x3],
// rpe_conv_wino1d[_x3]) and by their weight packers: the descriptor rules, the 64-channel tile split of the 3x3 Winograd kernels, the
// filling of the kernels' parameter structs and the pack launch.  An entry point states its rules in ITS order (which of RPE_E_BADARG /
// RPE_E_UNSUPPORTED a descriptor that breaks several gets is part of the ABI) and names what only its kernel needs, one line each.
#pragma once
#include "rpe_common.h"
#include <type_traits>

// ---- descriptor rules
static inline bool conv_desc_present(const rpe_conv_desc* d) {
    return d && d->x && d->packed && d->out && d->b > 0 && d->cin > 0 && d->cout > 0 && d->h > 0 && d->w > 0;
}
// a tensor the kernel moves in 16-byte (aligned16) or 8-byte (aligned8) pieces: base and batch stride (floats); an absent one passes
static inline bool aligned16(const void* p, long long batch_stride) { return !p || ((((uintptr_t)p) & 15) == 0 && (batch_stride & 3) == 0); }
static inline bool aligned8(const void* p, long long batch_stride) { return !p || ((((uintptr_t)p) & 7) == 0 && (batch_stride & 1) == 0); }
static inline bool conv_plain_only(const rpe_conv_desc* d) { return !d->add && !d->hidden && !d->zgate; }                          // no GRU operands
static inline bool conv_no_encoder_epilogue(const rpe_conv_desc* d) { return !d->scale && !d->residual && !d->stats && !d->pre_norm; }
static inline bool conv_linear_or_relu(const rpe_conv_desc* d) { return d->mode == RPE_CONV_LINEAR || d->mode == RPE_CONV_RELU; }
// what the GRU gate modes need: GATE_ZR writes z to out and r * h to out2 (cout = both gates), GATE_H blends hidden and tanh(v) by zgate
static inline bool conv_gate_args_ok(const rpe_conv_desc* d) {
    if (d->mode == RPE_CONV_GATE_ZR) return d->out2 && d->hidden && d->gate_channels > 0 && d->cout == 2 * d->gate_channels;
    return d->mode != RPE_CONV_GATE_H || (d->hidden && d->zgate);
}
// rpe_conv_*_v: the valid extent lies inside the map (equal to it = the plain entry point's launch)
static inline bool conv_valid_extent_ok(const rpe_conv_desc_v* dv) {
    return dv->h_valid > 0 && dv->w_valid > 0 && dv->h_valid <= dv->d.h && dv->w_valid <= dv->d.w;
}
static inline bool stride_is_1(const rpe_conv_desc* d) { return d->stride == 0 || d->stride == 1; }                                // 0 = unset
static inline int round_up(int n, int tile) { return (n + tile - 1) / tile * tile; }

// ---- parameter structs: the fields every kernel's struct has, then those of the structs with encoder epilogues | GRU operands (the
// structs themselves stay apart: their layout is what the kernels were tuned with)
template <class P> static inline void fill_common(P& p, const rpe_conv_desc* d, int coP) {
    p.x = d->x; p.xbs = d->x_batch_stride; p.wp = (decltype(p.wp))d->packed; p.cin = d->cin; p.cout = d->cout; p.coP = coP;
    p.bias = d->bias; p.out = d->out; p.obs = d->out_batch_stride; p.out2 = d->out2; p.o2bs = d->out2_batch_stride; p.mode = d->mode;
}
template <class P> static inline void fill_encoder(P& p, const rpe_conv_desc* d) {
    p.scale = d->scale; p.res = d->residual; p.rbs = d->residual_batch_stride; p.stats = d->stats; p.pre = d->pre_norm;
}
template <class P> static inline void fill_gate(P& p, const rpe_conv_desc* d) {             // (the hidden state has its own name per struct)
    p.add = d->add; p.abs_ = d->add_batch_stride; p.z = d->zgate; p.zbs = d->zgate_batch_stride; p.cgate = d->gate_channels;
}

// ---- launch planning of the 3x3 Winograd kernels (conv_wino.hip, conv_wino24.hip, conv_wino_x3.hip)
// epilogue shape: 0 plain, 1 scale / residual (cnet), 2 moments alone (fnet), 3 anything else
static inline int wino_epilogue_class(const rpe_conv_desc* d) {
    if (conv_no_encoder_epilogue(d)) return 0;
    return (d->stats && !d->scale && !d->residual) ? 2 : !d->stats ? 1 : 3;
}
// 64-channel tiles; a remainder of at most 32 channels (cout = 96) runs as one 32-channel tile instead of a half-empty 64
struct Tiles64 { int n64; bool tail32; };
static inline Tiles64 tiles64(int cout) {
    const int rem = cout % 64;
    const bool tail32 = rem > 0 && rem <= 32;
    return {tail32 ? cout / 64 : round_up(cout, 64) / 64, tail32};
}
// Launches below this many 64-channel workgroups use 32-channel tiles instead (rpe_conv_wino explains; rpe_conv_wino24 shares the threshold)
#ifndef WINO_SMALL_WG
#define WINO_SMALL_WG 512LL                       /* (tools/build_variant.sh -DWINO_SMALL_WG=... for A/B runs) */
#endif
// the full tiles, then the 32-channel tail as a launch of its own at co_base: launch(CB, tiles) starts `tiles` tiles of 32 * CB channels
template <class P, class F> static inline void launch_tiles64(P& p, F&& launch) {
    const Tiles64 t = tiles64(p.cout);
    p.co_base = 0;
    if (t.n64 > 0) launch(std::integral_constant<int, 2>{}, t.n64);
    if (t.tail32) { p.co_base = t.n64 * 64; launch(std::integral_constant<int, 1>{}, 1); }
}
// the runtime (epilogue class, pre_norm) as compile-time constants: f(EPI, PRE).  The input normalisation exists with moments alone (2)
// and with the general epilogue (3), which also serves its classes 0 and 1.
template <class F> static inline void dispatch_epi_pre(int epi, bool pre, F&& f) {
    if (pre) { if (epi == 2) f(std::integral_constant<int, 2>{}, std::true_type{}); else f(std::integral_constant<int, 3>{}, std::true_type{}); }
    else if (epi == 0) f(std::integral_constant<int, 0>{}, std::false_type{});
    else if (epi == 1) f(std::integral_constant<int, 1>{}, std::false_type{});
    else if (epi == 2) f(std::integral_constant<int, 2>{}, std::false_type{});
    else f(std::integral_constant<int, 3>{}, std::false_type{});
}

// ---- weight packing: the shared argument checks, then kernel(weight, packed, cout, cin, mid..., total) over `total` elements
template <class K, class T, class... A>
static inline int launch_pack(K kernel, const float* weight, T* packed, int cout, int cin, int cin_step, long long total, void* stream, A... mid) {
    if (!weight || !packed || cout <= 0 || cin <= 0) return RPE_E_BADARG;
    if (cin % cin_step) return RPE_E_UNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, weight, packed, cout, cin, mid..., total);
    return rpe_check_launch();
}
