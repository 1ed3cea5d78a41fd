// RAFT's sequence loss on ground-truth flow and its gradient: what trains the flow network as RAFT itself is trained.
//
//   mask   = valid & !(|gt| >= max_flow)          |gt| the per-pixel Euclidean norm, formed in f64
//   term_k = (1 / M) sum_{b,c,y,x} mask |pred_k - gt|,   M = b 2 H W (the mean runs over ALL elements, as upstream's .mean())
//   loss   = sum_k w_k term_k,   w_k = gamma^(N-1-k) handed in as doubles
//   metrics on the LAST prediction over mask pixels: mean end-point error, the fractions with an error below 1, 3 and 5 px
//
// One deliberate departure from upstream RAFT: a masked pixel contributes exactly zero to the loss and to the gradient, whatever pred
// and gt hold there, NaN and inf included (a select, not upstream's ``valid * i_loss``, which makes 0 * NaN = NaN of it).  A NaN in gt
// under a VALID pixel is not masked (NaN >= max_flow is false): the loss and that pixel's gradient are NaN, and the optimizer's
// non-finite test skips the step.
//
//   k_flow_loss_partial   a workgroup takes FLOW_LOSS_TILE consecutive pixels of the (b, H, W) index space, four per lane, a wave's lanes
//                         on consecutive pixels (every load is one coalesced dword per lane: any H and W, no alignment beyond 4 bytes).
//                         gt and valid are read once per pixel and kept in registers; every prediction is read once.  Differences and
//                         magnitudes in f64; one f64 partial per quantity and workgroup: the N sums of |pred_k - gt|, then the sum of the
//                         end-point errors, the three counts and the mask count (N + 5 quantities).
//   k_flow_loss_finish    a second launch adds every quantity's partials in workgroup order in f64 and writes the record.  No float
//                         atomics, nothing crosses workgroups inside a launch: the same bits on every run.
//   k_flow_loss_backward  d pred_k = float32(w_k g / M) sign(pred_k - gt) on mask pixels (NaN where the difference is NaN), exact 0 on
//                         masked pixels and where pred_k == gt; g = d L / d loss is read from the device.  The mask is formed again from
//                         gt and valid: nothing is kept between forward and backward.
#include "rpe_common.h"

#define FL_THREADS 256
#define FL_PER_LANE 4
#define FL_TILE RPE_FLOW_LOSS_TILE
#define FL_EXTRA 5                         // quantities behind the N sums: epe sum, < 1 px, < 3 px, < 5 px, mask count
#define FL_MAX_PREDS 1024                  // (N + 5) * 4 doubles of LDS per workgroup

static_assert(FL_TILE == FL_THREADS * FL_PER_LANE, "rpe.h: RPE_FLOW_LOSS_TILE");

struct FlPixels {                          // a lane's four pixels: offsets of their x component within a (b,2,H,W) tensor, gt, mask
    long long off[FL_PER_LANE];
    double gx[FL_PER_LANE], gy[FL_PER_LANE];
    bool m[FL_PER_LANE];
};

__device__ __forceinline__ void fl_load(FlPixels& P, const float* gt, const uint8_t* valid, long long pixels, int hw, double max_flow) {
#pragma unroll
    for (int j = 0; j < FL_PER_LANE; ++j) {
        const long long p = (long long)blockIdx.x * FL_TILE + j * FL_THREADS + threadIdx.x;
        P.m[j] = false; P.off[j] = 0; P.gx[j] = 0.0; P.gy[j] = 0.0;
        if (p < pixels) {
            const long long bi = p / hw;
            P.off[j] = bi * 2 * hw + (p - bi * hw);
            const double gx = (double)gt[P.off[j]], gy = (double)gt[P.off[j] + hw];
            P.gx[j] = gx; P.gy[j] = gy;
            P.m[j] = valid[p] != 0 && !(sqrt(gx * gx + gy * gy) >= max_flow);
        }
    }
}

__global__ __launch_bounds__(FL_THREADS) void k_flow_loss_partial(const float* const* preds, int n_preds, const float* gt, const uint8_t* valid,
                                                                  long long pixels, int hw, double max_flow, double* partial) {
    extern __shared__ double red[];                                    // [quantity][wave]
    const int tid = threadIdx.x, wave = tid >> 6, n_blocks = gridDim.x;
    FlPixels P;
    fl_load(P, gt, valid, pixels, hw, max_flow);
    double epe = 0.0, c1 = 0.0, c3 = 0.0, c5 = 0.0, cm = 0.0;
    for (int k = 0; k < n_preds; ++k) {
        const float* pk = preds[k];
        const bool last = k == n_preds - 1;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < FL_PER_LANE; ++j) {
            if (!P.m[j]) continue;                                     // a masked pixel is never read: whatever it holds contributes nothing
            const double dx = (double)pk[P.off[j]] - P.gx[j], dy = (double)pk[P.off[j] + hw] - P.gy[j];
            s += fabs(dx) + fabs(dy);
            if (last) {
                const double e = sqrt(dx * dx + dy * dy);
                epe += e; cm += 1.0;
                c1 += e < 1.0 ? 1.0 : 0.0; c3 += e < 3.0 ? 1.0 : 0.0; c5 += e < 5.0 ? 1.0 : 0.0;
            }
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) red[k * 4 + wave] = s;
    }
    epe = wave_sum(epe); c1 = wave_sum(c1); c3 = wave_sum(c3); c5 = wave_sum(c5); cm = wave_sum(cm);
    if ((tid & 63) == 0) {
        red[(n_preds + 0) * 4 + wave] = epe; red[(n_preds + 1) * 4 + wave] = c1; red[(n_preds + 2) * 4 + wave] = c3;
        red[(n_preds + 3) * 4 + wave] = c5; red[(n_preds + 4) * 4 + wave] = cm;
    }
    __syncthreads();
    for (int q = tid; q < n_preds + FL_EXTRA; q += FL_THREADS)
        partial[(long long)q * n_blocks + blockIdx.x] = ((red[q * 4] + red[q * 4 + 1]) + red[q * 4 + 2]) + red[q * 4 + 3];
}

__global__ __launch_bounds__(FL_THREADS) void k_flow_loss_finish(const double* partial, int n_blocks, int n_preds, const double* weights, double count_all,
                                                                 double* record, float* loss_f32) {
    extern __shared__ double tot[];                                    // [quantity]
    const int tid = threadIdx.x;
    for (int q = tid; q < n_preds + FL_EXTRA; q += FL_THREADS) {
        double t = 0.0;
        for (int i = 0; i < n_blocks; ++i) t += partial[(long long)q * n_blocks + i];          // workgroup order
        tot[q] = t;
    }
    __syncthreads();
    if (tid != 0) return;
    double loss = 0.0;
    for (int k = 0; k < n_preds; ++k) {
        const double term = tot[k] / count_all;
        record[RPE_FLOW_LOSS_TERMS + k] = term;
        loss += weights[k] * term;
    }
    const double cm = tot[n_preds + 4];
    record[RPE_FLOW_LOSS_LOSS] = loss;
    record[RPE_FLOW_LOSS_EPE] = tot[n_preds + 0] / cm;                 // (no mask pixel: 0 / 0 = NaN, as a mean over nothing)
    record[RPE_FLOW_LOSS_1PX] = tot[n_preds + 1] / cm;
    record[RPE_FLOW_LOSS_3PX] = tot[n_preds + 2] / cm;
    record[RPE_FLOW_LOSS_5PX] = tot[n_preds + 3] / cm;
    ((long long*)record)[RPE_FLOW_LOSS_COUNT] = (long long)cm;
    *loss_f32 = (float)loss;
}

__global__ __launch_bounds__(FL_THREADS) void k_flow_loss_backward(const float* const* preds, int n_preds, const float* gt, const uint8_t* valid,
                                                                   long long pixels, int hw, double max_flow, const double* weights, const float* g,
                                                                   double count_all, float* const* grads) {
    FlPixels P;
    fl_load(P, gt, valid, pixels, hw, max_flow);
    const double gd = (double)g[0];
    for (int k = 0; k < n_preds; ++k) {
        const float* pk = preds[k];
        float* dk = grads[k];
        const float c = (float)(weights[k] * gd / count_all);
#pragma unroll
        for (int j = 0; j < FL_PER_LANE; ++j) {
            const long long p = (long long)blockIdx.x * FL_TILE + j * FL_THREADS + threadIdx.x;
            if (p >= pixels) continue;
            float ox = 0.0f, oy = 0.0f;
            if (P.m[j]) {
                const double dx = (double)pk[P.off[j]] - P.gx[j], dy = (double)pk[P.off[j] + hw] - P.gy[j];
                ox = dx > 0.0 ? c : dx < 0.0 ? -c : dx == 0.0 ? 0.0f : __builtin_nanf("");
                oy = dy > 0.0 ? c : dy < 0.0 ? -c : dy == 0.0 ? 0.0f : __builtin_nanf("");
            }
            dk[P.off[j]] = ox;
            dk[P.off[j] + hw] = oy;
        }
    }
}

static bool fl_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the checks both entry points share -> RPE_OK with the pixel count and the number of workgroups
static int fl_check(const void* preds, int n_preds, const void* gt, const void* valid, const void* weights, int b, int h, int w, double max_flow,
                    long long* pixels, int* n_blocks) {
    if (!preds || !gt || !valid || !weights || n_preds < 1 || b < 1 || h < 1 || w < 1 || !(max_flow > 0.0)) return RPE_E_BADARG;
    if (fl_misaligned(preds, 8) || fl_misaligned(gt, 4) || fl_misaligned(weights, 8)) return RPE_E_BADARG;
    if (n_preds > FL_MAX_PREDS) return RPE_E_UNSUPPORTED;
    const long long px = (long long)b * h * w;
    if ((long long)h * w >= (1LL << 30) || px * 2 >= (1LL << 40)) return RPE_E_UNSUPPORTED;
    const long long blocks = (px + FL_TILE - 1) / FL_TILE;
    if (blocks > 0x7fffffffLL) return RPE_E_UNSUPPORTED;
    *pixels = px; *n_blocks = (int)blocks;
    return RPE_OK;
}

extern "C" size_t rpe_flow_sequence_loss_workspace_bytes(int n_preds, int b, int h, int w) {
    if (n_preds < 1 || n_preds > FL_MAX_PREDS || b < 1 || h < 1 || w < 1) return 0;
    const long long blocks = ((long long)b * h * w + FL_TILE - 1) / FL_TILE;
    return (size_t)(n_preds + FL_EXTRA) * (size_t)blocks * sizeof(double);
}

extern "C" int rpe_flow_sequence_loss(const float* const* preds, int n_preds, const float* gt, const uint8_t* valid, const double* weights, int b,
                                      int h, int w, double max_flow, void* workspace, double* record, float* loss_f32, void* stream) {
    long long pixels;
    int n_blocks;
    const int st = fl_check(preds, n_preds, gt, valid, weights, b, h, w, max_flow, &pixels, &n_blocks);
    if (st != RPE_OK) return st;
    if (!workspace || !record || !loss_f32 || fl_misaligned(workspace, 8) || fl_misaligned(record, 8) || fl_misaligned(loss_f32, 4)) return RPE_E_BADARG;
    const size_t lds = (size_t)(n_preds + FL_EXTRA) * 4 * sizeof(double);
    hipLaunchKernelGGL(k_flow_loss_partial, dim3(n_blocks), dim3(FL_THREADS), lds, (hipStream_t)stream, preds, n_preds, gt, valid, pixels, h * w,
                       max_flow, (double*)workspace);
    if (rpe_check_launch() != RPE_OK) return RPE_E_LAUNCH;
    hipLaunchKernelGGL(k_flow_loss_finish, dim3(1), dim3(FL_THREADS), (size_t)(n_preds + FL_EXTRA) * sizeof(double), (hipStream_t)stream,
                       (const double*)workspace, n_blocks, n_preds, weights, (double)(2 * pixels), record, loss_f32);
    return rpe_check_launch();
}

extern "C" int rpe_flow_sequence_loss_backward(const float* const* preds, int n_preds, const float* gt, const uint8_t* valid, const double* weights,
                                               const float* g, int b, int h, int w, double max_flow, float* const* grads, void* stream) {
    long long pixels;
    int n_blocks;
    const int st = fl_check(preds, n_preds, gt, valid, weights, b, h, w, max_flow, &pixels, &n_blocks);
    if (st != RPE_OK) return st;
    if (!g || !grads || fl_misaligned(g, 4) || fl_misaligned(grads, 8)) return RPE_E_BADARG;
    hipLaunchKernelGGL(k_flow_loss_backward, dim3(n_blocks), dim3(FL_THREADS), 0, (hipStream_t)stream, preds, n_preds, gt, valid, pixels, h * w, max_flow,
                       weights, g, (double)(2 * pixels), grads);
    return rpe_check_launch();
}
