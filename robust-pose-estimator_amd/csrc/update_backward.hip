// Backward of ONE application of RAFT's update block without its heads (core/RAFT/core/update.py BasicMotionEncoder, SepConvGRU):
//     cor = relu(convc2(relu(convc1(corr))))   flo = relu(convf2(relu(convf1(flow))))   m = relu(conv([cor | flo]))   x = [inp | m | flow]
//     per half (1x5, then 5x1):  z = s(convz([h | x]))  r = s(convr([h | x]))  q = tanh(convq([r h | x]))  h <- (1 - z) h + z q
// Upstream detaches coords1 at the top of every iteration, so corr and flow are constants of the step and the only path through time is h.
// Here: what the step's backward needs beyond raft_backward.hip -- the adjoints of the GRU's gate epilogues and the gates' recomputation
// (rpe_gru_gates_*).  The weight gradients of the 1x5, 5x1 and 7x7 layers are rpe_conv_bwd_weight's (raft_backward.hip); the data gradients
// are FORWARD convolutions on transposed, flipped weights over groups of input channels (ops.py), as in the tail.
// No float atomics; every sum runs in an order fixed by the shapes, so two runs give the same bits; a row's result does not depend on its batch.
#include "rpe_common.h"

// ------------------------------------------------------------------------------------------------------------------- GRU gates, adjoint
// One half:  h' = (1 - z) h + z q,  z = s(z_pre), q = tanh(q_pre), and rh = r h feeds convq, r = s(r_pre).  From d = d loss / d h' and the
// POST-activation values (recomputed by the caller):
//     d z_pre = d (q - h) z (1 - z)      d q_pre = d z (1 - q^2)      d h = d (1 - z)                                   (k_gate_bwd_zq)
// and, once convq's data gradient has given g = d loss / d (rh):
//     d r_pre = g h r (1 - r)            d h += g r                                                                      (k_gate_bwd_r)
// Products in double, one rounding per result: a saturated gate (z, r = 0 or 1, q = +-1 in f32) gives exact zeros, never NaN.
// Everything is a (b,c,hw) channel slice with its own batch stride; grid (blocks, b).
__global__ __launch_bounds__(256) void k_gate_bwd_zq(const float* __restrict__ d, long long dbs, const float* __restrict__ hid, long long hbs,
                                                     const float* __restrict__ z, long long zbs, const float* __restrict__ q, long long qbs,
                                                     size_t per, float* __restrict__ dz, long long dzbs, float* __restrict__ dq, long long dqbs,
                                                     float* __restrict__ dh, long long dhbs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const double g = (double)d[(size_t)bz * dbs + e], hv = (double)hid[(size_t)bz * hbs + e];
        const double zv = (double)z[(size_t)bz * zbs + e], qv = (double)q[(size_t)bz * qbs + e];
        dz[(size_t)bz * dzbs + e] = (float)(g * (qv - hv) * (zv * (1.0 - zv)));
        dq[(size_t)bz * dqbs + e] = (float)(g * zv * (1.0 - qv * qv));
        dh[(size_t)bz * dhbs + e] = (float)(g * (1.0 - zv));
    }
}

// (dh_out may be dh_in or g: every element is read before it is written, by the one thread that owns it)
__global__ __launch_bounds__(256) void k_gate_bwd_r(const float* g, long long gbs, const float* __restrict__ hid, long long hbs,
                                                    const float* __restrict__ r, long long rbs, const float* dh_in, long long dibs, size_t per,
                                                    float* __restrict__ dr, long long drbs, float* dh_out, long long dobs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const double gv = (double)g[(size_t)bz * gbs + e], hv = (double)hid[(size_t)bz * hbs + e], rv = (double)r[(size_t)bz * rbs + e];
        const double acc = (double)dh_in[(size_t)bz * dibs + e];
        dr[(size_t)bz * drbs + e] = (float)(gv * hv * (rv * (1.0 - rv)));
        dh_out[(size_t)bz * dobs + e] = (float)(acc + gv * rv);
    }
}

// The gates again, for the backward: the forward's gate epilogues keep z and r h only, the adjoints need r and q as well.  Pre-activations
// in (bias already added), activations in double and rounded once -- the values the adjoints are evaluated at carry one f32 rounding each.
//     z = s(zr_pre[:c]), r = s(zr_pre[c:]), rh = r h                                                                   (k_gate_fwd_zr)
//     q = tanh(q_pre), h' = (1 - z) h + z q                                                                             (k_gate_fwd_h)
__global__ __launch_bounds__(256) void k_gate_fwd_zr(const float* __restrict__ zr, long long zrbs, const float* __restrict__ hid, long long hbs,
                                                     size_t per, float* __restrict__ z, long long zbs, float* __restrict__ r, long long rbs,
                                                     float* __restrict__ rh, long long rhbs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const double zv = 1.0 / (1.0 + exp(-(double)zr[(size_t)bz * zrbs + e]));
        const float rv = (float)(1.0 / (1.0 + exp(-(double)zr[(size_t)bz * zrbs + per + e])));
        z[(size_t)bz * zbs + e] = (float)zv;
        r[(size_t)bz * rbs + e] = rv;
        rh[(size_t)bz * rhbs + e] = rv * hid[(size_t)bz * hbs + e];
    }
}

__global__ __launch_bounds__(256) void k_gate_fwd_h(const float* __restrict__ qp, long long qpbs, const float* __restrict__ z, long long zbs,
                                                    const float* __restrict__ hid, long long hbs, size_t per, float* __restrict__ q, long long qbs,
                                                    float* __restrict__ hn, long long hnbs) {
    const int bz = blockIdx.y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const float qv = (float)tanh((double)qp[(size_t)bz * qpbs + e]);
        const double zv = (double)z[(size_t)bz * zbs + e];
        q[(size_t)bz * qbs + e] = qv;
        hn[(size_t)bz * hnbs + e] = (float)((1.0 - zv) * (double)hid[(size_t)bz * hbs + e] + zv * (double)qv);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- entry points
extern "C" int rpe_gru_gates_zq_backward(const float* d_h_new, long long d_batch_stride, const float* h, long long h_batch_stride, const float* z,
                                         long long z_batch_stride, const float* q, long long q_batch_stride, int b, int c, int hw, float* d_z_pre,
                                         long long dz_batch_stride, float* d_q_pre, long long dq_batch_stride, float* d_h,
                                         long long dh_batch_stride, void* stream) {
    if (!d_h_new || !h || !z || !q || !d_z_pre || !d_q_pre || !d_h || b < 0 || b > 65535 || c <= 0 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (d_batch_stride < per || h_batch_stride < per || z_batch_stride < per || q_batch_stride < per || dz_batch_stride < per ||
        dq_batch_stride < per || dh_batch_stride < per)
        return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_gate_bwd_zq, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, d_h_new, d_batch_stride, h,
                       h_batch_stride, z, z_batch_stride, q, q_batch_stride, (size_t)per, d_z_pre, dz_batch_stride, d_q_pre, dq_batch_stride, d_h,
                       dh_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_gru_gates_r_backward(const float* d_rh, long long drh_batch_stride, const float* h, long long h_batch_stride, const float* r,
                                        long long r_batch_stride, const float* d_h_in, long long dhi_batch_stride, int b, int c, int hw,
                                        float* d_r_pre, long long dr_batch_stride, float* d_h_out, long long dho_batch_stride, void* stream) {
    if (!d_rh || !h || !r || !d_h_in || !d_r_pre || !d_h_out || b < 0 || b > 65535 || c <= 0 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (drh_batch_stride < per || h_batch_stride < per || r_batch_stride < per || dhi_batch_stride < per || dr_batch_stride < per ||
        dho_batch_stride < per)
        return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_gate_bwd_r, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, d_rh, drh_batch_stride, h,
                       h_batch_stride, r, r_batch_stride, d_h_in, dhi_batch_stride, (size_t)per, d_r_pre, dr_batch_stride, d_h_out,
                       dho_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_gru_gates_zr_recompute(const float* zr_pre, long long zr_batch_stride, const float* h, long long h_batch_stride, int b, int c,
                                          int hw, float* z, long long z_batch_stride, float* r, long long r_batch_stride, float* rh,
                                          long long rh_batch_stride, void* stream) {
    if (!zr_pre || !h || !z || !r || !rh || b < 0 || b > 65535 || c <= 0 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (zr_batch_stride < 2 * per || h_batch_stride < per || z_batch_stride < per || r_batch_stride < per || rh_batch_stride < per)
        return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_gate_fwd_zr, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, zr_pre, zr_batch_stride, h,
                       h_batch_stride, (size_t)per, z, z_batch_stride, r, r_batch_stride, rh, rh_batch_stride);
    return rpe_check_launch();
}

extern "C" int rpe_gru_gates_h_recompute(const float* q_pre, long long qp_batch_stride, const float* z, long long z_batch_stride, const float* h,
                                         long long h_batch_stride, int b, int c, int hw, float* q, long long q_batch_stride, float* h_new,
                                         long long hn_batch_stride, void* stream) {
    if (!q_pre || !z || !h || !q || !h_new || b < 0 || b > 65535 || c <= 0 || hw <= 0) return RPE_E_BADARG;
    const long long per = (long long)c * hw;
    if (qp_batch_stride < per || z_batch_stride < per || h_batch_stride < per || q_batch_stride < per || hn_batch_stride < per) return RPE_E_BADARG;
    if (b == 0) return RPE_OK;
    hipLaunchKernelGGL(k_gate_fwd_h, dim3(min(ceil_div(per, 256), 2048), b), dim3(256), 0, (hipStream_t)stream, q_pre, qp_batch_stride, z,
                       z_batch_stride, h, h_batch_stride, (size_t)per, q, q_batch_stride, h_new, hn_batch_stride);
    return rpe_check_launch();
}
