// Solve-quality report of the pose layer on gfx950: at a given pose T, the counts, weighted and unweighted residual sums, objective,
// tangent gradient, Gauss-Newton Hessian and from them the formal covariance C = (2 f / (m - 6)) H^-1 of the weighted fit (include/rpe.h,
// rpe_pose_quality, has the slot table).  Same objective, gates and float64 arithmetic as csrc/pose.hip (core/pose/pose_head.py:12-58 of
// the reference); nothing here is on the solve's path, and nothing of the solve is touched.
//
//   k_pose_quality_reduce : grid (nblk, n), one pixel per thread per step, 35 f64 accumulators, 64-lane butterfly -> LDS -> one partial
//                           row per workgroup.  nblk depends on (h, w) ONLY: a row is partitioned the same way in every batch, so its
//                           result does not depend on the batch, bit for bit.
//   k_pose_quality_finish : one workgroup per row, behind the first launch on the same stream: adds the row's partials in index order,
//                           factors H (Cholesky, f64), inverts it and writes the 64 slots.
// No atomics, no tickets, nothing waits inside a kernel: the launch boundary is the only hand-off.
#include "rpe_common.h"

#define Q_THREADS 256
#define Q_PIXELS_PER_BLOCK 1024   // pixels a workgroup is sized for (4 per thread); at most Q_MAX_BLOCKS workgroups per row
#define Q_MAX_BLOCKS 512
#define Q_NACC 35                 // n2d n3d sw1 sw2 S2w S3w S2u S3u g[6] H[21]
#define Q_PART 40                 // doubles per partial row (Q_NACC + pad)
#define Q_OUT 64

enum { A_N2D = 0, A_N3D, A_SW1, A_SW2, A_S2W, A_S3W, A_S2U, A_S3U, A_G = 8, A_H = 14 };

static int quality_nblk(int h, int w) {
    const int64_t hw = (int64_t)h * w;
    int64_t nblk = (hw + Q_PIXELS_PER_BLOCK - 1) / Q_PIXELS_PER_BLOCK;
    if (nblk < 1) nblk = 1;
    if (nblk > Q_MAX_BLOCKS) nblk = Q_MAX_BLOCKS;
    return (int)nblk;
}

extern "C" size_t rpe_pose_quality_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return (sizeof(double) * Q_PART * (size_t)quality_nblk(h, w) * (size_t)n + 255) / 256 * 256 + 256;
}

__device__ __forceinline__ int qtri(int i, int j) {   // upper-triangle index, i <= j
    return i * 6 - (i * (i - 1)) / 2 + (j - i);
}

struct QualityArgs {
    const float* flow; const float* pcl1; const float* pcl2; const float* w1; const float* w2;
    const uint8_t* m1; const uint8_t* m2; const float* K; const float* lw; const double* T;
    int n, h, w;
};

__global__ __launch_bounds__(Q_THREADS) void k_pose_quality_reduce(QualityArgs A, double* __restrict__ partials) {
    const int row = blockIdx.y, nblk = gridDim.x;
    const int64_t hw = (int64_t)A.h * A.w;
    // the row's constants (wave-uniform loads): R, t from the quaternion as csrc/pose.hip's write_rt, K in f64, the two normalisations
    const double* Tp = A.T + (size_t)row * 7;
    const double qx = Tp[3], qy = Tp[4], qz = Tp[5], qw = Tp[6];
    const double R0 = 1.0 - 2.0 * (qy * qy + qz * qz), R1 = 2.0 * (qx * qy - qz * qw), R2 = 2.0 * (qx * qz + qy * qw);
    const double R3 = 2.0 * (qx * qy + qz * qw), R4 = 1.0 - 2.0 * (qx * qx + qz * qz), R5 = 2.0 * (qy * qz - qx * qw);
    const double R6 = 2.0 * (qx * qz - qy * qw), R7 = 2.0 * (qy * qz + qx * qw), R8 = 1.0 - 2.0 * (qx * qx + qy * qy);
    const double t0 = Tp[0], t1 = Tp[1], t2 = Tp[2];
    double K[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) K[i] = (double)A.K[(size_t)row * 9 + i];
    const double hwd = (double)A.h * (double)A.w;
    const double c2 = (double)A.lw[row * 2 + 1] / hwd / hwd;     // mean then /(h*w)  (pose_head.py:29)
    const double c3 = (double)A.lw[row * 2 + 0] / hwd;           // mean              (pose_head.py:51)
    const double Wd = (double)A.w, Hd = (double)A.h;

    const float* flx = A.flow + (size_t)row * 2 * hw; const float* fly = flx + hw;
    const float* p1 = A.pcl1 + (size_t)row * 3 * hw;
    const float* p2 = A.pcl2 + (size_t)row * 3 * hw;
    const float* w1p = A.w1 + (size_t)row * hw; const float* w2p = A.w2 + (size_t)row * hw;
    const uint8_t* m1p = A.m1 + (size_t)row * hw; const uint8_t* m2p = A.m2 + (size_t)row * hw;

    double acc[Q_NACC];
#pragma unroll
    for (int i = 0; i < Q_NACC; ++i) acc[i] = 0.0;

    for (int64_t i = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; i < hw; i += (int64_t)nblk * Q_THREADS) {
        const int64_t yy = i / A.w;
        const double px = (double)(i - yy * A.w) + 0.5, py = (double)yy + 0.5;
        const double pa = (double)p1[i], pb = (double)p1[hw + i], pc = (double)p1[2 * hw + i];
        const double w1 = (double)w1p[i], w2 = (double)w2p[i];
        const bool m1 = m1p[i] != 0, m2 = m2p[i] != 0;
        // X = R p + t ; ipts = K X ; depth = clamp(iz, 1e-12)   (pinhole_transforms.py:28-30,93-98)
        const double X = R0 * pa + R1 * pb + R2 * pc + t0;
        const double Y = R3 * pa + R4 * pb + R5 * pc + t1;
        const double Z = R6 * pa + R7 * pb + R8 * pc + t2;
        const double ix = K[0] * X + K[1] * Y + K[2] * Z;
        const double iy = K[3] * X + K[4] * Y + K[5] * Z;
        const double iz = K[6] * X + K[7] * Y + K[8] * Z;
        const double dep = iz < 1e-12 ? 1e-12 : iz;               // NaN stays NaN, like torch.clamp
        const double passz = iz >= 1e-12 ? 1.0 : 0.0;
        const double u = ix / dep, v = iy / dep;
        const double fx = px + (double)flx[i], fy = py + (double)fly[i];   // pose_head.py:19
        const double ex = fx - u, ey = fy - v;
        const double e2 = ex * ex + ey * ey;
        const double r2 = e2 * w1;                                // :21-22
        const bool inimg = (fx > 0.0) && (fy > 0.0) && (fx < Wd) && (fy < Hd);   // :24
        const bool bad = isinf(r2) || isnan(r2) || !inimg || !m1; // :25
        const double ex3 = X - (double)p2[i], ey3 = Y - (double)p2[hw + i], ez3 = Z - (double)p2[2 * hw + i];   // :41-43
        const double e3 = ex3 * ex3 + ey3 * ey3 + ez3 * ez3;
        const bool ok3 = m1 && m2;                                // :47
        acc[A_N2D] += bad ? 0.0 : 1.0;
        acc[A_N3D] += ok3 ? 1.0 : 0.0;
        acc[A_SW1] += bad ? 0.0 : w1;
        acc[A_SW2] += ok3 ? w2 : 0.0;
        acc[A_S2W] += bad ? 0.0 : r2;                             // :28-29
        acc[A_S3W] += ok3 ? e3 * w2 : 0.0;
        acc[A_S2U] += bad ? 0.0 : e2;
        acc[A_S3U] += ok3 ? e3 : 0.0;
        // gradient, multiplied out the way autograd does (0 * nan = nan reaches g, as in the reference and in rpe_pose_reduce)
        const double a2 = -2.0 * w1 * (bad ? 0.0 : 1.0) * c2;
        const double gu = a2 * ex, gv = a2 * ey;
        const double a3 = 2.0 * w2 * (ok3 ? 1.0 : 0.0) * c3;
        const double g_ix = gu / dep, g_iy = gv / dep;
        const double g_iz = -(gu * ix + gv * iy) / (dep * dep) * passz;
        const double gX = K[0] * g_ix + K[3] * g_iy + K[6] * g_iz + a3 * ex3;
        const double gY = K[1] * g_ix + K[4] * g_iy + K[7] * g_iz + a3 * ey3;
        const double gZ = K[2] * g_ix + K[5] * g_iy + K[8] * g_iz + a3 * ez3;
        acc[A_G + 0] += gX; acc[A_G + 1] += gY; acc[A_G + 2] += gZ;   // [I | -[X]x]^T gX
        acc[A_G + 3] += Y * gZ - Z * gY;
        acc[A_G + 4] += Z * gX - X * gZ;
        acc[A_G + 5] += X * gY - Y * gX;
        // Gauss-Newton Hessian H = 2 sum c w J^T J.  J = A P with A = d(u, v)/dX (2 x 3; the identity for the 3-D term) and
        // P = [I | -[X]x], so H += P^T M P with M = s2 A^T A + s3 I = [[M, B], [B^T, C]], B = -M [X]x, C = [X]x B (as csrc/pose.hip).
        // A masked-out term contributes exactly nothing, whatever its Jacobian holds (selects, not products with zero).
        const double s2 = bad ? 0.0 : 2.0 * w1 * c2;
        const double s3 = ok3 ? 2.0 * w2 * c3 : 0.0;
        if (s2 == 0.0 && s3 == 0.0) continue;
        const bool on2 = s2 != 0.0;
        const double up = u * passz, vp = v * passz;
        const double au0 = on2 ? (K[0] - up * K[6]) / dep : 0.0, au1 = on2 ? (K[1] - up * K[7]) / dep : 0.0, au2 = on2 ? (K[2] - up * K[8]) / dep : 0.0;
        const double av0 = on2 ? (K[3] - vp * K[6]) / dep : 0.0, av1 = on2 ? (K[4] - vp * K[7]) / dep : 0.0, av2 = on2 ? (K[5] - vp * K[8]) / dep : 0.0;
        const double su0 = s2 * au0, su1 = s2 * au1, su2 = s2 * au2, sv0 = s2 * av0, sv1 = s2 * av1, sv2 = s2 * av2;
        const double m00 = su0 * au0 + sv0 * av0 + s3, m01 = su0 * au1 + sv0 * av1, m02 = su0 * au2 + sv0 * av2;
        const double m11 = su1 * au1 + sv1 * av1 + s3, m12 = su1 * au2 + sv1 * av2;
        const double m22 = su2 * au2 + sv2 * av2 + s3;
        double* Hh = acc + A_H;
        Hh[0] += m00; Hh[1] += m01; Hh[2] += m02; Hh[6] += m11; Hh[7] += m12; Hh[11] += m22;      // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        // B[i][.] = (m_i2 Y - m_i1 Z, m_i0 Z - m_i2 X, m_i1 X - m_i0 Y), m_i = row i of M
        const double b00 = m02 * Y - m01 * Z, b01 = m00 * Z - m02 * X, b02 = m01 * X - m00 * Y;
        const double b10 = m12 * Y - m11 * Z, b11 = m01 * Z - m12 * X, b12 = m11 * X - m01 * Y;
        const double b20 = m22 * Y - m12 * Z, b21 = m02 * Z - m22 * X, b22 = m12 * X - m02 * Y;
        Hh[3] += b00; Hh[4] += b01; Hh[5] += b02;                 // (0,3..5)
        Hh[8] += b10; Hh[9] += b11; Hh[10] += b12;                // (1,3..5)
        Hh[12] += b20; Hh[13] += b21; Hh[14] += b22;              // (2,3..5)
        // C = [X]x B, [X]x = [[0, -Z, Y], [Z, 0, -X], [-Y, X, 0]] (upper triangle)
        Hh[15] += Y * b20 - Z * b10; Hh[16] += Y * b21 - Z * b11; Hh[17] += Y * b22 - Z * b12;   // (3,3..5)
        Hh[18] += Z * b01 - X * b21; Hh[19] += Z * b02 - X * b22;                                 // (4,4) (4,5)
        Hh[20] += X * b12 - Y * b02;                                                              // (5,5)
    }

    __shared__ double red[Q_THREADS / RPE_WAVE][Q_PART];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < Q_NACC; ++i) {
        const double s = wave_sum(acc[i]);
        if (lane == 0) red[wv][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < Q_PART) {
        double s = 0.0;
        if (threadIdx.x < Q_NACC) s = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        partials[((size_t)row * nblk + blockIdx.x) * Q_PART + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void k_pose_quality_finish(const double* __restrict__ partials, int nblk, const float* lw, int h, int w,
                                                            double* __restrict__ out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    __shared__ double vals[Q_PART], o[Q_OUT], L[6][6], Li[6][6];
    if (lane < Q_PART) {
        const double* p = partials + (size_t)row * nblk * Q_PART + lane;
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += p[(size_t)b * Q_PART];       // index order: the order is the contract (it fixes the bits)
        vals[lane] = s;
    }
    o[lane] = 0.0;
    __syncthreads();
    if (lane == 0) {
        const double hwd = (double)h * (double)w;
        const double n2d = vals[A_N2D], n3d = vals[A_N3D];
        const double loss2d = vals[A_S2W] / hwd / hwd, loss3d = vals[A_S3W] / hwd;
        const double f = (double)lw[row * 2 + 1] * loss2d + (double)lw[row * 2 + 0] * loss3d;
        for (int i = 0; i < 6; ++i) o[i] = vals[i];
        o[6] = sqrt(vals[A_S2U] / n2d);                           // 0 / 0 = NaN: a row without kept residuals has no RMS
        o[7] = sqrt(vals[A_S3U] / n3d);
        o[8] = f;
        double gm = 0.0;                                          // torch .abs().max(): NaN propagates
        for (int i = 0; i < 6; ++i) { const double a = fabs(vals[A_G + i]); if (a > gm || isnan(a)) gm = a; if (isnan(gm)) break; }
        o[9] = gm;
        for (int i = 0; i < 6; ++i) o[10 + i] = vals[A_G + i];
        const double m = 2.0 * n2d + 3.0 * n3d;
        // Cholesky H = L L^T (as the Gauss-Newton step of csrc/pose.hip)
        bool ok = true;
        for (int i = 0; i < 6 && ok; ++i) {
            for (int j = 0; j <= i; ++j) {
                double s = vals[A_H + qtri(j, i)];
                for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
                if (i == j) { if (!(s > 0.0) || !isfinite(s)) { ok = false; break; } L[i][i] = sqrt(s); }
                else L[i][j] = s / L[j][j];
            }
        }
        const bool pd = ok && m > 6.0 && isfinite(f);
        if (pd) {
            // Li = L^-1 (lower triangular, column by column), H^-1 = Li^T Li
            for (int c = 0; c < 6; ++c) {
                for (int i = 0; i < 6; ++i) {
                    if (i < c) { Li[i][c] = 0.0; continue; }
                    double s = i == c ? 1.0 : 0.0;
                    for (int k = c; k < i; ++k) s -= L[i][k] * Li[k][c];
                    Li[i][c] = s / L[i][i];
                }
            }
            const double sc = 2.0 * f / (m - 6.0);
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) {
                    double s = 0.0;
                    for (int k = j; k < 6; ++k) s += Li[k][i] * Li[k][j];
                    o[16 + i * 6 + j] = o[16 + j * 6 + i] = sc * s;
                }
        } else {
            for (int i = 0; i < 36; ++i) o[16 + i] = __builtin_nan("");
        }
        o[52] = pd ? 1.0 : 0.0;
        o[53] = m;
    }
    __syncthreads();
    out[(size_t)row * Q_OUT + lane] = o[lane];
}

extern "C" int rpe_pose_quality(const float* flow, const float* pcl1, const float* pcl2, const float* w1, const float* w2,
                                const uint8_t* mask1, const uint8_t* mask2, const float* K, const float* loss_weight,
                                const double* T, int n, int h, int w, double* out, void* workspace, void* stream) {
    if (!flow || !pcl1 || !pcl2 || !w1 || !w2 || !mask1 || !mask2 || !K || !loss_weight || !T || !out || n <= 0 || h <= 0 || w <= 0)
        return RPE_E_BADARG;
    if (!workspace) return RPE_E_BADARG;
    double* partials = (double*)(((uintptr_t)workspace + 255) / 256 * 256);
    const int nblk = quality_nblk(h, w);
    hipStream_t s = (hipStream_t)stream;
    QualityArgs A{flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, T, n, h, w};
    hipLaunchKernelGGL(k_pose_quality_reduce, dim3(nblk, n), dim3(Q_THREADS), 0, s, A, partials);
    hipLaunchKernelGGL(k_pose_quality_finish, dim3(n), dim3(64), 0, s, (const double*)partials, nblk, loss_weight, h, w, out);
    return rpe_check_launch();
}
