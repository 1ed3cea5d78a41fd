// Backward of RAFT's all-pairs correlation (core/RAFT/core/corr.py CorrBlock: build, 2x2 average pooling, radius-4 window lookup), for the
// f32 pyramid route.  Upstream detaches coords1 at the top of every iteration, so the lookup coordinates are constants: the looked-up
// window is LINEAR in the pyramid and the pyramid is BILINEAR in (fmap1, fmap2).  Nothing is truncated and nothing goes into the coordinates.
//
//   G (b, h8 w8, S), S = sum_l h_l w_l (h_l = h8 >> l, w_l = w8 >> l): the gradient volume, d loss / d pyramid.  Row p = the `levels` maps of
//   query p one after the other, each row-major.  Dense f32, zero-filled by the caller.
//
//   k_corr_lookup_bwd  G += the adjoint of ONE lookup: per query and level the 81 window values' gradients are spread over the window's
//                      footprint with the forward's own tap arithmetic (corr_taps.h make_taps: integer taps and fractions per tap, so the
//                      footprint is 11 x 11 cells of which a window without a deviating tap touches 10 x 10).  Gather form: one lane owns a
//                      cell and adds its (at most four non-zero) weight x gradient terms in one fixed order; cells outside the level are
//                      dropped (grid_sample's zero padding).  One wave owns a query's row of G: no atomics, the stream orders the calls.
//   k_cb_pool          F2cat (b, c, S): fmap2 followed by its successively 2x2-pooled copies (floor: a last odd row / column is dropped).
//                      Pooling is linear: avg_pool2d of the correlation over the second image = correlating against the pooled fmap2.
//   k_cb_gemm          the two GEMMs on the f32 matrix cores (v_mfma_f32_32x32x2_f32), bw_gemm.h's tile constants under a main loop of this file's:
//                          d_fmap1 = F2cat G^T / sqrt(c)   (c x S by S x h8 w8: contraction over S)
//                          dF2cat  = fmap1 G / sqrt(c)     (c x h8 w8 by h8 w8 x S: contraction over the queries)
//                      the contraction axis is split by split_chunk(K, 8, 512), a function of the shape alone; every chunk writes a partial
//   k_splitk_reduce    (bw_gemm.h) the partials added in chunk order in f64, times 1 / sqrt(c), rounded once
//   k_cb_unpool        d_fmap2 = dF2cat's level 0 + the pool adjoints of the levels above, applied from the last level down to 0: a quarter
//                      of a value to each of the four cells its pool covered, nothing to a dropped row or column
// No float atomics; every sum's order is fixed by the shapes: two runs give the same bits and a batch row's bits do not depend on the batch.
#include "rpe_common.h"
#include "corr_taps.h"
#include "bw_gemm.h"

#define CB_MAX_LEVELS 4
#define CB_FOOT (WIN + 2)          // cells per axis a window can touch: lo .. lo + 10

struct CbGeom {
    int b, h8, w8, levels, nq, S;
    int h[CB_MAX_LEVELS], w[CB_MAX_LEVELS], off[CB_MAX_LEVELS];      // level sizes (the pyramid's: h8 >> l) and first cell of a level in a row of G
};

// the pyramid's geometry rule (corr.hip make_geom): every level at least 2 x 2
static bool cb_geom(int b, int h8, int w8, int levels, CbGeom& g) {
    if (b <= 0 || h8 <= 0 || w8 <= 0 || levels <= 0 || levels > CB_MAX_LEVELS) return false;
    g.b = b; g.h8 = h8; g.w8 = w8; g.levels = levels;
    if ((long long)h8 * w8 >= (1ll << 30)) return false;
    g.nq = h8 * w8;
    long long off = 0;
    int h = h8, w = w8;
    for (int l = 0; l < CB_MAX_LEVELS; ++l) {
        if (l < levels) {
            if (h < 2 || w < 2) return false;
            g.h[l] = h; g.w[l] = w; g.off[l] = (int)off;
            off += (long long)h * w;
            h /= 2; w /= 2;
        } else { g.h[l] = g.w[l] = 0; g.off[l] = (int)off; }
    }
    g.S = (int)off;
    return true;
}

// --------------------------------------------------------------------------------------------------------------- adjoint of the lookup
#define LB_Q 16                    // queries per workgroup: their d_corr columns are staged once (64-byte runs of the query axis)
#define LB_WAVES 4

// weight of tap i on pixel lo + i + s (s = 0, 1, 2), TapAxis' three-weight form; 0 outside 0 <= i < WIN.  Static indexing only.
__device__ __forceinline__ float tap_weight(const TapAxis& T, int i, int s) {
    float v = 0.0f;
#pragma unroll
    for (int t = 0; t < WIN; ++t) {
        const float a = s == 0 ? T.a0[t] : (s == 1 ? T.a1[t] : T.a2[t]);
        v = t == i ? a : v;
    }
    return v;
}

__global__ __launch_bounds__(64 * LB_WAVES) void k_corr_lookup_bwd(const float* __restrict__ coords, const float* __restrict__ d_corr,
                                                                   float* __restrict__ Gv, CbGeom g) {
    __shared__ float sD[CB_MAX_LEVELS * WIN * WIN * LB_Q];
    const int bz = blockIdx.y, q0 = blockIdx.x * LB_Q;
    const int nch = g.levels * WIN * WIN;
    for (int e = threadIdx.x; e < nch * LB_Q; e += 64 * LB_WAVES) {
        const int ch = e / LB_Q, q = q0 + e % LB_Q;
        sD[e] = q < g.nq ? d_corr[((size_t)bz * nch + ch) * g.nq + q] : 0.0f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int qi = 0; qi < LB_Q / LB_WAVES; ++qi) {
        const int qq = wv * (LB_Q / LB_WAVES) + qi, q = q0 + qq;
        if (q >= g.nq) break;                                           // (no barrier below)
        float* row = Gv + ((size_t)bz * g.nq + q) * g.S;
        for (int l = 0; l < g.levels; ++l) {
            const float inv = 1.0f / (float)(1 << l);
            const float cx = coords[((size_t)bz * 2 + 0) * g.nq + q] * inv;       // coords / 2**l (exact), as the forward
            const float cy = coords[((size_t)bz * 2 + 1) * g.nq + q] * inv;
            TapAxis X, Y;
            make_taps(cx, g.w[l], X);
            make_taps(cy, g.h[l], Y);
            const int hl = g.h[l], wl = g.w[l];
            if (X.lo + CB_FOOT <= 0 || X.lo >= wl || Y.lo + CB_FOOT <= 0 || Y.lo >= hl) continue;      // (wave-uniform) wholly outside
            const float* dq = sD + (size_t)l * WIN * WIN * LB_Q + qq;
            for (int cell = lane; cell < CB_FOOT * CB_FOOT; cell += 64) {
                const int v = cell / CB_FOOT, u = cell - v * CB_FOOT;
                const int x = X.lo + u, y = Y.lo + v;
                if (x < 0 || x >= wl || y < 0 || y >= hl) continue;
                // pixel lo + u is read by tap u (slot 0), tap u - 1 (slot 1) and tap u - 2 (slot 2); channel = i * 9 + j with i along x
                float acc = 0.0f;
#pragma unroll
                for (int sx = 0; sx < 3; ++sx) {
                    const int i = u - sx;
                    const float wx = tap_weight(X, i, sx);
#pragma unroll
                    for (int sy = 0; sy < 3; ++sy) {
                        const int j = v - sy;
                        const float wy = tap_weight(Y, j, sy);
                        const bool ok = i >= 0 && i < WIN && j >= 0 && j < WIN;
                        const float d = dq[(ok ? i * WIN + j : 0) * LB_Q];
                        const float wgt = rn_mul(wx, wy);
                        if (ok && wgt != 0.0f) acc = fmaf(wgt, d, acc);
                    }
                }
                const size_t o = (size_t)g.off[l] + (size_t)y * wl + x;
                row[o] = rn_add(row[o], acc);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- adjoint of the build
// F2cat (b, c, S): level 0 = fmap2, level l = the 2x2 mean (floor) of level l - 1.  One launch per level, in order.
__global__ __launch_bounds__(256) void k_cb_pool(const float* __restrict__ fmap2, float* __restrict__ F, CbGeom g, int l, int planes) {
    const int hl = g.h[l], wl = g.w[l];
    const size_t per = (size_t)hl * wl, total = per * planes;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t pl = e / per;
        const int p = (int)(e - pl * per);
        float* dst = F + pl * g.S + g.off[l];
        if (l == 0) { dst[p] = fmap2[pl * per + p]; continue; }
        const int y = p / wl, x = p - y * wl, wp = g.w[l - 1];
        const float* src = F + pl * g.S + g.off[l - 1] + (size_t)(2 * y) * wp + 2 * x;
        dst[p] = 0.25f * rn_add(rn_add(src[0], src[1]), rn_add(src[wp], src[wp + 1]));
    }
}

// chunk of the contraction axis: at most 8 chunks of whole 32-steps, at least 512 long -- a function of K alone
static inline int cb_chunk(int K) { return (int)split_chunk(K, 8, 512); }
static inline int cb_chunks(int K) { return split_chunks(K, 8, 512); }

// part[bz][chunk][m][n] = sum_{k in chunk} A[bz][m][k] B[bz][n][k]:  A[m][k] at A[m lda + k];  B[n][k] at B[n ldb + k] (BT = false: d_fmap1,
// B = G, k = the cell) or at B[k ldb + n] (BT = true: dF2cat, B = G, k = the query).  Staging: A, and B along k, as thread
// t's k column t & 31 of rows (t >> 5) + 8 r; B across k as its column t & 127 at k = (t >> 7) + 2 r, coalesced along n.  A row / column / k
// outside the problem is read from a clamped address and selected to zero.  The tile and the
// multiply are bw_gemm_body's (bw_gemm.h), restated here: see that header for why.
template <bool BT>
__global__ __launch_bounds__(256) void k_cb_gemm(const float* __restrict__ A, long long abs_, int lda, const float* __restrict__ B, long long bbs,
                                                 int ldb, int M, int N, int K, int kc, int chunks, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sA[BW_BM * BW_LD];
    __shared__ __attribute__((aligned(16))) float sB[BW_BN * BW_LD];
    const int bz = blockIdx.z / chunks, ch = blockIdx.z - bz * chunks;
    A += (size_t)bz * abs_;
    B += (size_t)bz * bbs;
    const int n0 = blockIdx.x * BW_BN, m0 = blockIdx.y * BW_BM;
    const int kbeg = ch * kc, kend = kbeg + kc < K ? kbeg + kc : K;
    const int tid = threadIdx.x, kl = tid & 31, r0 = tid >> 5, nl = tid & 127, kh = tid >> 7;
    float ra[16], rb[16];
    auto load = [&](int ks) {
        const int k = ks + kl;
        const bool kv = k < kend;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + r0 + 8 * r;
            const bool av = kv && m < M;
            const float a = A[av ? (size_t)m * lda + k : 0];
            ra[r] = av ? a : 0.0f;
            if (!BT) {
                const int n = n0 + r0 + 8 * r;
                const bool bv = kv && n < N;
                const float v = B[bv ? (size_t)n * ldb + k : 0];
                rb[r] = bv ? v : 0.0f;
            } else {
                const int kk = ks + kh + 2 * r, n = n0 + nl;
                const bool bv = kk < kend && n < N;
                const float v = B[bv ? (size_t)kk * ldb + n : 0];
                rb[r] = bv ? v : 0.0f;
            }
        }
    };
    const int lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int li = lane & 31, lh = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][c][e] = 0.0f;
    load(kbeg);
    for (int ks = kbeg; ks < kend; ks += BW_BK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sA[(r0 + 8 * r) * BW_LD + kl] = ra[r];
            if (!BT) sB[(r0 + 8 * r) * BW_LD + kl] = rb[r];
            else sB[nl * BW_LD + kh + 2 * r] = rb[r];
        }
        __syncthreads();
        if (ks + BW_BK < kend) load(ks + BW_BK);
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            float fa[2][4], fb[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float4 va = *(const float4*)&sA[(wm * 64 + a * 32 + li) * BW_LD + lh * 16 + t4 * 4];
                const float4 vb = *(const float4*)&sB[(wn * 64 + a * 32 + li) * BW_LD + lh * 16 + t4 * 4];
                fa[a][0] = va.x; fa[a][1] = va.y; fa[a][2] = va.z; fa[a][3] = va.w;
                fb[a][0] = vb.x; fb[a][1] = vb.y; fb[a][2] = vb.z; fb[a][3] = vb.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a][e], fb[c][e], acc[a][c], 0, 0, 0);
        }
        __syncthreads();
    }
    // C / D layout of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* out = part + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n = n0 + wn * 64 + c * 32 + li;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m < M && n < N) out[(size_t)m * N + n] = acc[a][c][e];
            }
        }
}

// d_fmap2 (b c planes of h8 x w8) from dF2cat (planes of S).  Gather form of "levels applied from the last down to 0": cell (y, x) of level 0
// lies under cell (y >> l, x >> l) of level l when every pool on the way covered it (a dropped row / column is under nothing), and
//     t_L = D_L;   t_l = D_l + t_{l+1} / 4 under a covering cell, D_l otherwise;   d_fmap2 = t_0.
__global__ __launch_bounds__(256) void k_cb_unpool(const float* __restrict__ D, float* __restrict__ out, CbGeom g, int planes) {
    const size_t per = (size_t)g.nq, total = per * planes;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t pl = e / per;
        const int p = (int)(e - pl * per);
        const int y = p / g.w8, x = p - y * g.w8;
        const float* d = D + pl * g.S;
        int top = 0;                                                    // the last level that covers this cell
        while (top + 1 < g.levels && (y >> (top + 1)) < g.h[top + 1] && (x >> (top + 1)) < g.w[top + 1]) ++top;
        float t = 0.0f;
        for (int l = top; l >= 1; --l) t = 0.25f * rn_add(d[g.off[l] + (y >> l) * g.w[l] + (x >> l)], t);
        out[e] = rn_add(d[p], t);
    }
}

// workspace: F2cat | dF2cat | partials, each rounded up to 256 bytes
static size_t r256(size_t v) { return (v + 255) / 256 * 256; }
static size_t cb_part_floats(const CbGeom& g, int c) {
    const size_t p1 = (size_t)g.b * cb_chunks(g.S) * c * g.nq, p2 = (size_t)g.b * cb_chunks(g.nq) * c * g.S;
    return p1 > p2 ? p1 : p2;
}

// ---------------------------------------------------------------------------------------------------------------------- entry points
extern "C" size_t rpe_corr_grad_volume_floats(int b, int h8, int w8, int levels) {
    CbGeom g;
    if (!cb_geom(b, h8, w8, levels, g)) return 0;
    return (size_t)b * g.nq * g.S;
}

extern "C" int rpe_corr_lookup_backward(const float* coords, const float* d_corr, int b, int h8, int w8, int levels, int radius, float* grad_volume,
                                        void* stream) {
    CbGeom g;
    if (!coords || !d_corr || !grad_volume || radius != RADIUS || b > 65535 || !cb_geom(b, h8, w8, levels, g)) return RPE_E_BADARG;
    hipLaunchKernelGGL(k_corr_lookup_bwd, dim3(ceil_div(g.nq, LB_Q), b), dim3(64 * LB_WAVES), 0, (hipStream_t)stream, coords, d_corr, grad_volume, g);
    return rpe_check_launch();
}

extern "C" size_t rpe_corr_build_backward_workspace_bytes(int b, int c, int h8, int w8, int levels) {
    CbGeom g;
    if (c <= 0 || c > 256 || c % 4 != 0 || !cb_geom(b, h8, w8, levels, g)) return 0;
    return 2 * r256((size_t)b * c * g.S * 4) + r256(cb_part_floats(g, c) * 4);
}

extern "C" int rpe_corr_build_backward(const float* grad_volume, const float* fmap1, const float* fmap2, int b, int c, int h8, int w8, int levels,
                                       float* d_fmap1, float* d_fmap2, float* d_f2cat, void* workspace, void* stream) {
    CbGeom g;
    if (!grad_volume || !fmap1 || !fmap2 || !d_fmap1 || !d_fmap2 || !workspace || c <= 0 || c > 256 || c % 4 != 0 || !cb_geom(b, h8, w8, levels, g))
        return RPE_E_BADARG;
    const int ch1 = cb_chunks(g.S), ch2 = cb_chunks(g.nq);
    if ((long long)b * ch1 > 65535 || (long long)b * ch2 > 65535 || b > 65535) return RPE_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* F = (float*)ws;
    float* D = d_f2cat ? d_f2cat : (float*)(ws + r256((size_t)b * c * g.S * 4));
    float* part = (float*)(ws + 2 * r256((size_t)b * c * g.S * 4));
    const int planes = b * c;
    for (int l = 0; l < g.levels; ++l)
        hipLaunchKernelGGL(k_cb_pool, dim3(min(ceil_div((long long)planes * g.h[l] * g.w[l], 256), 4096)), dim3(256), 0, s, fmap2, F, g, l, planes);
    const double scale = 1.0 / sqrt((double)c);
    const long long gbs = (long long)g.nq * g.S;
    // d_fmap1 = F2cat G^T: M = c, N = queries, K = S
    hipLaunchKernelGGL((k_cb_gemm<false>), dim3(ceil_div(g.nq, BW_BN), ceil_div(c, BW_BM), b * ch1), dim3(256), 0, s, F, (long long)c * g.S, g.S,
                       grad_volume, gbs, g.S, c, g.nq, g.S, cb_chunk(g.S), ch1, part);
    splitk_reduce_launch(part, b, ch1, (long long)c * g.nq, scale, d_fmap1, s);
    // dF2cat = fmap1 G: M = c, N = S, K = queries
    hipLaunchKernelGGL((k_cb_gemm<true>), dim3(ceil_div(g.S, BW_BN), ceil_div(c, BW_BM), b * ch2), dim3(256), 0, s, fmap1, (long long)c * g.nq, g.nq,
                       grad_volume, gbs, g.S, c, g.S, g.nq, cb_chunk(g.nq), ch2, part);
    splitk_reduce_launch(part, b, ch2, (long long)c * g.S, scale, D, s);
    hipLaunchKernelGGL(k_cb_unpool, dim3(min(ceil_div((long long)planes * g.nq, 256), 4096)), dim3(256), 0, s, D, d_fmap2, g, planes);
    return rpe_check_launch();
}
