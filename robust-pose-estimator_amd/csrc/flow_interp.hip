// Warm start of RAFT's update loop from the previous frame's flow (upstream core/RAFT/core/utils/utils.py::forward_interpolate and
// RAFT.forward's flow_init: coords1 = coords0 + flow_init).
//
// rpe_flow_forward_interpolate: every source pixel (x0, y0) of a 1/8 flow lands at (x0 + dx, y0 + dy) (f64; the sums of an integer and
// an f32 value); the landing points strictly inside the map are the valid ones, and every grid point takes the (dx, dy) of the nearest
// valid one -- squared distance (x - x1)^2 + (y - y1)^2 in f64, the two squares rounded separately and then added (this unit is built
// with -ffp-contract=off), ties to the lowest source index y0 * w + x0.  Exact brute force: a workgroup owns 256 grid points of one
// row and streams the row's landing points through LDS in tiles of 256, in index order, replacing its best match only on a STRICTLY
// smaller distance -- which is what makes the lowest index win a tie.  No atomics, no cross-workgroup state: a row's result does not
// depend on the batch or the launch size.  The outputs are copies of input values (or 0 for a row without a valid point).
#include "rpe_common.h"

namespace {

constexpr int FI_THREADS = 256;

__global__ __launch_bounds__(FI_THREADS) void k_forward_interpolate(const float* __restrict__ flow, int h, int w, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double2 pts[FI_THREADS];
    const int hw = h * w;
    const long long row = blockIdx.y;
    const float* fx = flow + row * 2 * hw;
    const float* fy = fx + hw;
    const int tid = threadIdx.x;
    const int p = blockIdx.x * FI_THREADS + tid;
    const double gx = (double)(p % w), gy = (double)(p / w);
    double best = INFINITY;
    int best_i = -1;
    for (int base = 0; base < hw; base += FI_THREADS) {
        const int q = base + tid;
        double2 pt = make_double2(INFINITY, INFINITY);          // an invalid point lies at infinity: its distance never wins
        int valid = 0;
        if (q < hw) {
            const double x1 = (double)(q % w) + (double)fx[q];
            const double y1 = (double)(q / w) + (double)fy[q];
            if (x1 > 0.0 && x1 < (double)w && y1 > 0.0 && y1 < (double)h) {   // (false for NaN)
                pt = make_double2(x1, y1);
                valid = 1;
            }
        }
        // (the barrier also ends the previous tile's reads of pts)
        if (__syncthreads_count(valid) == 0) continue;
        pts[tid] = pt;
        __syncthreads();
        const int n = min(FI_THREADS, hw - base);
        for (int j = 0; j < n; ++j) {
            const double2 v = pts[j];
            const double ex = gx - v.x, ey = gy - v.y;
            const double d = ex * ex + ey * ey;
            if (d < best) {
                best = d;
                best_i = base + j;
            }
        }
    }
    if (p < hw) {
        float* o = out + row * 2 * hw;
        o[p] = best_i >= 0 ? fx[best_i] : 0.0f;
        o[hw + p] = best_i >= 0 ? fy[best_i] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_flow_seed(const float* __restrict__ fi, int h, int w, float* coords_out, float* flow_out, float* dst1,
                                                   long long dst1_bs, float* dst2, long long dst2_bs) {
    const int hw = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const long long b = blockIdx.y;
    const float dx = fi[b * 2 * hw + p], dy = fi[b * 2 * hw + hw + p];
    if (coords_out) {
        coords_out[b * 2 * hw + p] = rn_add((float)(p % w), dx);
        coords_out[b * 2 * hw + hw + p] = rn_add((float)(p / w), dy);
    }
    if (flow_out) {
        flow_out[b * 2 * hw + p] = dx;
        flow_out[b * 2 * hw + hw + p] = dy;
    }
    if (dst1) {
        dst1[b * dst1_bs + p] = dx;
        dst1[b * dst1_bs + hw + p] = dy;
    }
    if (dst2) {
        dst2[b * dst2_bs + p] = dx;
        dst2[b * dst2_bs + hw + p] = dy;
    }
}

}  // namespace

extern "C" int rpe_flow_forward_interpolate(const float* flow, int b, int h, int w, float* out, void* stream) {
    if (!flow || !out || b <= 0 || h <= 0 || w <= 0 || (long long)h * w > (1LL << 30) / 2 || b > 65535) return RPE_E_BADARG;
    const int hw = h * w;
    hipLaunchKernelGGL(k_forward_interpolate, dim3(ceil_div(hw, FI_THREADS), b), dim3(FI_THREADS), 0, (hipStream_t)stream, flow, h, w, out);
    return rpe_check_launch();
}

extern "C" int rpe_flow_seed(const float* flow_init, int b, int h, int w, float* coords_out, float* flow_out, float* dst1,
                             long long dst1_batch_stride, float* dst2, long long dst2_batch_stride, void* stream) {
    if (!flow_init || b <= 0 || h <= 0 || w <= 0 || (long long)h * w > (1LL << 30) / 2 || b > 65535) return RPE_E_BADARG;
    const long long plane2 = 2LL * h * w;
    if ((dst1 && dst1_batch_stride < plane2) || (dst2 && dst2_batch_stride < plane2)) return RPE_E_BADARG;
    hipLaunchKernelGGL(k_flow_seed, dim3(ceil_div((long long)h * w, 256), b), dim3(256), 0, (hipStream_t)stream, flow_init, h, w, coords_out,
                       flow_out, dst1, dst1_batch_stride, dst2, dst2_batch_stride);
    return rpe_check_launch();
}
