// RAFT correlation WITHOUT the all-pairs volume (upstream's ``alternate_corr``): the radius-4 window of every query is recomputed from the
// two feature maps at every lookup.  Same output contract as rpe_corr_lookup (corr.hip): channel (level, i, j) = x offset i - r, y offset
// j - r (the transposed window of core/RAFT/core/corr.py), zero for taps outside the level's map, bilinear weights and integer taps from
// make_taps (corr_taps.h) -- the arithmetic rpe_corr_lookup and rpe_corr_lookup_taps use.
//
// Pooling the correlation over its target axes and pooling fmap2 are the same linear map: pool(corr)[q, y, x] = f1[q] . pool(f2)[y, x].
// So the scratch holds, pixel-major (a pixel's c channels contiguous, 4 c bytes apart):
//     F1    (b, h8 * w8, c)      fmap1 / sqrt(c)
//     F2_l  (b, h_l * w_l, c)    fmap2 pooled l times (2x2 mean, stride 2, sizes floored: F.avg_pool2d), l = 0 .. levels - 1
// each block rounded up to 256 bytes: b c h8 w8 4 (1 + 1 + 1/4 + 1/16 + 1/64) bytes against the pyramid's b (h8 w8)^2 4 (1 + 1/4 + ...).
//
// k_alt_lookup: one workgroup (4 waves) = one (pair, level, 8 x 8 tile of queries).  Per ROUND the workgroup anchors a box of at most
// 20 x 19 pixels of the level on the pending queries (topmost window row; among the queries within 8 rows of it the leftmost window
// column), multiplies Q (64 queries x c) by Box (c x P pixels, P <= 380) on the f32 matrix cores -- operands straight from the pixel-major
// scratch (16 bytes per lane and 8 channels; the matrix instructions, not the loads, bound the loop), products to LDS -- and every query
// whose 11 x 11 window lies in the box blends its 81 outputs out of its own row of the product.  Smooth flow serves the 64 queries in one
// round (constant flow: 18 x 18 pixels at level 0, about 3x the minimal products); queries whose windows are further apart (divergent
// flow) are served by further rounds of the SAME code with the box re-anchored, down to one query per round.  There is deliberately no
// second, scalar path: a product value is one matrix-unit accumulation chain over the channels in a fixed order (lanes 0-31 take channels
// 8t .. 8t+3, lanes 32-63 channels 8t+4 .. 8t+7, step by step), which depends on the query's row of F1 and the pixel's row of F2_l only --
// not on the box, the round or the neighbours' flow --, so a query's 81 outputs are bit-identical however its neighbours move and
// whichever batch it sits in.  No atomics: every output has one writer.
//
// RPE_F16 features (rpe_corr_alt_prepare_ex / rpe_corr_alt_lookup_dt; upstream's AlternateCorrBlock under autocast): the same scratch in
// fp16, a pixel's c channels 2 c bytes apart, blocks still rounded to 256 bytes and in the same order.  F1 = half(fmap1) and F2_0 =
// half(fmap2), round to nearest even and UNSCALED; F2_l = half(0.25 * (sum of the four STORED fp16 values of F2_{l-1}, in f32, k_alt_pool's
// order)): one rounding per level, upstream's fp16 avg_pool2d level after level.  The lookup is the same kernel (a template on the operand
// type) with the products on v_mfma_f32_32x32x16_f16 -- lane (l31, lh) holds channels 16t + 8 lh .. + 7 of its row, one 16-byte load per
// operand and 16 channels -- f32 accumulation in the fixed order t = 0, 1, .., and 1 / sqrt(c) applied in f32 where the accumulators go
// to the LDS product (so a c that is no power of 4 costs the features nothing).  Rounds, boxes, blend and addressing are shared code.
#include "rpe_common.h"
#include "corr_taps.h"

#define ALT_LEVELS 4
#define ALT_ALIGN 256                   // bytes every block of the scratch is rounded up to (include/rpe.h: RPE_CORR_ALT_PAD covers it)
#define ALT_TQ 8                        // the query tile is ALT_TQ x ALT_TQ
#define ALT_BW 20                       // box columns
#define ALT_BH 19                       // box rows
#define ALT_NBLK 12                     // 32-pixel column blocks of the product: 384 >= ALT_BW * ALT_BH
#define ALT_PP (ALT_NBLK * 32 + 1)      // product row pitch (floats): odd, so the 64 queries' reads at one box offset hit 64 banks
#define ALT_WINP (WIN + 2)              // window pixels per axis (taps i, i + 1, i + 2)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the 16-byte piece of a pixel's channels a lane loads per operand: V channels of type T
template <typename T> struct AltVec;
template <> struct AltVec<float> { typedef f32x4 type; static constexpr int V = 4; };
template <> struct AltVec<_Float16> { typedef f16x8 type; static constexpr int V = 8; };

struct AltGeom {
    int b, c, h8, w8, levels;
    int h[ALT_LEVELS], w[ALT_LEVELS];
    long long f2[ALT_LEVELS];           // element offset of F2_l (F1 is at 0)
    long long total;                    // elements (floats, or halves with esize = 2)
};

static bool alt_geom(int b, int c, int h8, int w8, int levels, AltGeom& G, int esize = 4) {
    if (c <= 0 || c > 256 || c % 16 != 0) return false;                                  // rpe_corr_build's channel rule
    if (rpe_corr_pyramid_bytes_ex(b, h8, w8, levels, RPE_F32) == 0) return false;       // the pyramid route's geometry rule
    G.b = b; G.c = c; G.h8 = h8; G.w8 = w8; G.levels = levels;
    const long long al = ALT_ALIGN / esize;
    long long off = ((long long)b * h8 * w8 * c + al - 1) / al * al;
    int h = h8, w = w8;
    for (int l = 0; l < ALT_LEVELS; ++l) {
        G.h[l] = l < levels ? h : 0; G.w[l] = l < levels ? w : 0; G.f2[l] = off;
        if (l < levels) off += ((long long)b * h * w * c + al - 1) / al * al;
        h /= 2; w /= 2;
    }
    G.total = off;
    return true;
}

extern "C" size_t rpe_corr_alt_bytes(int b, int c, int h8, int w8, int levels) {
    AltGeom G;
    return alt_geom(b, c, h8, w8, levels, G) ? (size_t)G.total * 4 : 0;
}

extern "C" size_t rpe_corr_alt_bytes_ex(int b, int c, int h8, int w8, int levels, int feature_dtype) {
    if (feature_dtype == RPE_F32) return rpe_corr_alt_bytes(b, c, h8, w8, levels);
    AltGeom G;
    return feature_dtype == RPE_F16 && alt_geom(b, c, h8, w8, levels, G, 2) ? (size_t)G.total * 2 : 0;
}

// ------------------------------------------------------------------------------------------------ prepare
// (b, C, n) -> (b, n, C) * scale through a 32 x 32 LDS tile: reads and writes both run along their fastest axis
// (T = _Float16: the product rounded to nearest even, like tensor.half(); the caller passes scale 1)
template <typename T>
__global__ __launch_bounds__(256) void k_alt_pack(const float* __restrict__ f, T* __restrict__ out, int C, int n, float scale) {
    __shared__ float tile[32][33];
    const int bz = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* src = f + (size_t)bz * C * n;
    T* dst = out + (size_t)bz * n * C;
    for (int r = ty; r < 32; r += 8) {
        const int ch = c0 + r, p = p0 + tx;
        tile[r][tx] = (ch < C && p < n) ? src[(size_t)ch * n + p] : 0.0f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, ch = c0 + tx;
        if (p < n && ch < C) dst[(size_t)p * C + ch] = (T)(tile[tx][r] * scale);
    }
}

// 2x2 mean, stride 2, floored sizes, in F.avg_pool2d's order of operations (row-major sum of the window, then the division)
// (T = _Float16: the four stored values summed in f32 in that order, times 0.25, rounded once to fp16; C4 = c / 8, a thread's 16 bytes)
template <typename T>
__global__ __launch_bounds__(256) void k_alt_pool(const T* __restrict__ src, T* __restrict__ dst, int C4, int hs, int ws, int hd, int wd, long long total) {
    typedef typename AltVec<T>::type vec;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;           // (b, y, x, c / 4)
    if (e >= total) return;
    const int c4 = (int)(e % C4);
    const long long p = e / C4;
    const int x = (int)(p % wd), y = (int)((p / wd) % hd);
    const long long bz = p / ((long long)wd * hd);
    const vec* s = (const vec*)src + ((bz * hs + 2 * y) * ws + 2 * x) * C4 + c4;
    const vec v00 = s[0], v01 = s[C4], v10 = s[(long long)ws * C4], v11 = s[(long long)ws * C4 + C4];
    vec o;
#pragma unroll
    for (int k = 0; k < AltVec<T>::V; ++k) o[k] = (T)rn_mul(rn_add(rn_add(rn_add((float)v00[k], (float)v01[k]), (float)v10[k]), (float)v11[k]), 0.25f);
    ((vec*)dst)[e] = o;
}

template <typename T>
static int alt_prepare(const float* fmap1, const float* fmap2, const AltGeom& G, float scale1, T* base, hipStream_t s) {
    const int b = G.b, c = G.c, nq = G.h8 * G.w8, V = AltVec<T>::V;
    const dim3 grid(ceil_div(nq, 32), ceil_div(c, 32), b);
    hipLaunchKernelGGL(k_alt_pack<T>, grid, dim3(256), 0, s, fmap1, base, c, nq, scale1);
    hipLaunchKernelGGL(k_alt_pack<T>, grid, dim3(256), 0, s, fmap2, base + G.f2[0], c, nq, 1.0f);
    for (int l = 1; l < G.levels; ++l) {
        const long long total = (long long)b * G.h[l] * G.w[l] * (c / V);
        hipLaunchKernelGGL(k_alt_pool<T>, dim3(ceil_div(total, 256)), dim3(256), 0, s, (const T*)(base + G.f2[l - 1]), base + G.f2[l], c / V, G.h[l - 1],
                           G.w[l - 1], G.h[l], G.w[l], total);
    }
    return rpe_check_launch();
}

extern "C" int rpe_corr_alt_prepare(const float* fmap1, const float* fmap2, int b, int c, int h8, int w8, int levels, void* scratch, void* stream) {
    AltGeom G;
    if (!fmap1 || !fmap2 || !scratch || (((uintptr_t)scratch) & 15) || !alt_geom(b, c, h8, w8, levels, G)) return RPE_E_BADARG;
    if (b > 65535) return RPE_E_UNSUPPORTED;
    return alt_prepare<float>(fmap1, fmap2, G, 1.0f / sqrtf((float)c), (float*)scratch, (hipStream_t)stream);
}

extern "C" int rpe_corr_alt_prepare_ex(const float* fmap1, const float* fmap2, int b, int c, int h8, int w8, int levels, int feature_dtype, void* scratch,
                                       void* stream) {
    if (feature_dtype == RPE_F32) return rpe_corr_alt_prepare(fmap1, fmap2, b, c, h8, w8, levels, scratch, stream);
    AltGeom G;
    if (feature_dtype != RPE_F16 || !fmap1 || !fmap2 || !scratch || (((uintptr_t)scratch) & 15) || !alt_geom(b, c, h8, w8, levels, G, 2)) return RPE_E_BADARG;
    if (b > 65535) return RPE_E_UNSUPPORTED;
    return alt_prepare<_Float16>(fmap1, fmap2, G, 1.0f, (_Float16*)scratch, (hipStream_t)stream);      // unscaled: the lookup applies 1 / sqrt(c)
}

// ------------------------------------------------------------------------------------------------ lookup
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, RPE_WAVE); v = o < v ? o : v; }
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, RPE_WAVE); v = o > v ? o : v; }
    return __builtin_amdgcn_readfirstlane(v);
}

// Q (64 x c) . Box (c x 32 NB) for this wave's NB column blocks; a[m] / bp[n]: this lane's row of F1 / F2_l, already offset by its half's
// four channels.  THE summation order of the route: per 8 channels four matrix steps, step j adding channel 8t + j (lanes 0-31's operand)
// and then channel 8t + 4 + j (lanes 32-63's) to the accumulator.
// T = _Float16: the pointers are offset by the half's EIGHT channels and one v_mfma_f32_32x32x16_f16 adds the 16 channels of step t (operand
// element j of lane half h = channel 16t + 8h + j, the same for both operands) -- the order over t is the route's order; ``scale`` =
// 1 / sqrt(c) multiplies the finished accumulators (f32: F1 carries it, the accumulators are stored as they are).
template <typename T, int NB>
__device__ __forceinline__ void alt_products(const T* const (&a)[2], const T* const (&bp)[3], int c, float* prod, const int (&col)[3], int l31, int lh, float scale) {
    typedef typename AltVec<T>::type vec;
    constexpr bool F16 = sizeof(T) == 2;
    f32x16 acc[2][NB];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
    if constexpr (F16) {
#pragma unroll 4
        for (int t = 0; t < c; t += 16) {
            f16x8 av[2], bv[NB];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = *(const f16x8*)(a[m] + t);
#pragma unroll
            for (int n = 0; n < NB; ++n) bv[n] = *(const f16x8*)(bp[n] + t);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[m], bv[n], acc[m][n], 0, 0, 0);
        }
    } else {
#pragma unroll 2
        for (int t = 0; t < c; t += 8) {
            f32x4 av[2], bv[NB];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = *(const f32x4*)(a[m] + t);
#pragma unroll
            for (int n = 0; n < NB; ++n) bv[n] = *(const f32x4*)(bp[n] + t);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][j], bv[n][j], acc[m][n], 0, 0, 0);
        }
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                prod[(m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * ALT_PP + col[n] + l31] = F16 ? rn_mul(acc[m][n][r], scale) : acc[m][n][r];
}

// map_h x map_w: the maps coords and out live in, of which the top-left h8 x w8 is read / written (rpe_corr_alt_lookup_ex: the update loop's
// padded workspace; = h8 x w8 for dense tensors).  The feature maps and every tap keep the true (h8, w8).
// T: the scratch's element type (float, or _Float16 with ``scale`` = 1 / sqrt(c); see alt_products).
template <typename T>
__global__ __launch_bounds__(256, 1) void k_alt_lookup(const T* __restrict__ scratch, const float* __restrict__ coords, float* __restrict__ out, AltGeom G,
                                                       int tiles_x, int map_h, int map_w, float scale) {
    constexpr int V = AltVec<T>::V;
    __shared__ float prod[64 * ALT_PP];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int l = blockIdx.y, bz = blockIdx.z;
    const int ty0 = (blockIdx.x / tiles_x) * ALT_TQ, tx0 = (blockIdx.x % tiles_x) * ALT_TQ;
    const int nq = G.h8 * G.w8, c = G.c, hl = G.h[l], wl = G.w[l];
    const T* f1 = scratch + (size_t)bz * nq * c;
    const T* f2 = scratch + G.f2[l] + (size_t)bz * hl * wl * c;

    // every wave holds the 64 queries of the tile, lane = query, and plans the rounds for itself: same inputs, same instructions, same plan
    const int qy = ty0 + (lane >> 3), qx = tx0 + (lane & 7);
    const bool qok = qy < G.h8 && qx < G.w8;
    const int q = qok ? qy * map_w + qx : ty0 * map_w + tx0;          // (the tile's first query always exists)
    const size_t mp = (size_t)map_h * map_w;
    const float inv = 1.0f / (float)(1 << l);
    const float cx = coords[((size_t)bz * 2 + 0) * mp + q] * inv;     // coords / 2**l  (exact)
    const float cy = coords[((size_t)bz * 2 + 1) * mp + q] * inv;
    TapAxis X, Y;
    make_taps(cx, wl, X);
    make_taps(cy, hl, Y);
    // a window wholly outside its map (or coordinates that are not finite) needs no products: every weight is cleared and the zeros are
    // stored in the first round
    const bool empty = !qok || X.lo + WIN + 1 < 0 || X.lo >= wl || Y.lo + WIN + 1 < 0 || Y.lo >= hl;
    if (empty) {
#pragma unroll
        for (int i = 0; i < WIN; ++i) { X.a0[i] = X.a1[i] = X.a2[i] = 0.0f; Y.a0[i] = Y.a1[i] = Y.a2[i] = 0.0f; }
    }
    // A operands: rows m * 32 + l31 of the tile
    const T* a[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int r = m * 32 + l31, ay = ty0 + (r >> 3), ax = tx0 + (r & 7);
        const bool ok = ay < G.h8 && ax < G.w8;
        a[m] = f1 + (size_t)(ok ? ay * G.w8 + ax : ty0 * G.w8 + tx0) * c + V * lh;
    }
    float* obase = out + ((size_t)bz * G.levels + l) * (WIN * WIN) * mp + q;

    const int big = 0x3fffffff;
    bool pending = !empty;
    bool first = true;
    for (;;) {
        // ---- the round's box: anchored on the topmost pending window row, then on the leftmost window column among the queries whose
        // rows fit; that query is always served, so every round retires at least one query
        const int y0 = wave_min_i(pending ? Y.lo : big);
        const bool cand = pending && Y.lo - y0 + ALT_WINP <= ALT_BH;
        const int x0 = wave_min_i(cand ? X.lo : big);
        const bool fits = cand && X.lo - x0 + ALT_WINP <= ALT_BW;
        const bool any = x0 != big;                                       // (false only when every query of the tile is empty)
        int bx_lo = 0, by_lo = 0, bw = 0, bh = 0;
        if (any) {
            const int nx = wave_max_i(fits ? X.lo - x0 + ALT_WINP : 0), ny = wave_max_i(fits ? Y.lo - y0 + ALT_WINP : 0);
            bx_lo = x0 > 0 ? x0 : 0; by_lo = y0 > 0 ? y0 : 0;
            const int bx_hi = x0 + nx < wl ? x0 + nx : wl, by_hi = y0 + ny < hl ? y0 + ny : hl;
            bw = bx_hi - bx_lo; bh = by_hi - by_lo;                       // 1 .. ALT_BW, 1 .. ALT_BH: a served window overlaps its map
        }
        const int P = bw * bh, nblk = (P + 31) >> 5;                      // <= ALT_NBLK
        // ---- products: wave wv takes column blocks wv, wv + 4, wv + 8
        const int nmine = nblk > wv ? (nblk - wv + 3) >> 2 : 0;
        if (nmine > 0) {
            const T* bp[3];
            int col[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                col[n] = (wv + 4 * n) * 32;
                int p = col[n] + l31;
                p = p < P ? p : 0;                                        // (padding columns: computed, never read)
                const int py = p / bw, px = p - py * bw;
                bp[n] = f2 + ((size_t)(by_lo + py) * wl + (bx_lo + px)) * c + V * lh;
            }
            if (nmine == 1) alt_products<T, 1>(a, bp, c, prod, col, l31, lh, scale);
            else if (nmine == 2) alt_products<T, 2>(a, bp, c, prod, col, l31, lh, scale);
            else alt_products<T, 3>(a, bp, c, prod, col, l31, lh, scale);
        }
        __syncthreads();
        // ---- blend: lane = query, wave wv takes the window rows j = wv, wv + 4, wv + 8.  Window pixel (cc, rr) of the query is box pixel
        // (ox + cc, oy + rr); pixels outside the box are outside the map (the box is only ever clipped by the map): they count as zero.
        if (qok && (fits || (first && empty))) {
            const int ox = X.lo - bx_lo, oy = Y.lo - by_lo;
            const float* mine = prod + lane * ALT_PP;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                if ((j & 3) != wv) continue;
                float hc[3][WIN];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int yy = oy + j + d;
                    const bool yok = fits && yy >= 0 && yy < bh;
                    float A[ALT_WINP];
#pragma unroll
                    for (int cc = 0; cc < ALT_WINP; ++cc) {
                        const int xx = ox + cc;
                        const bool ok = yok && xx >= 0 && xx < bw;
                        A[cc] = ok ? mine[ok ? yy * bw + xx : 0] : 0.0f;
                    }
#pragma unroll
                    for (int i = 0; i < WIN; ++i) hc[d][i] = A[i] * X.a0[i] + A[i + 1] * X.a1[i] + A[i + 2] * X.a2[i];
                }
#pragma unroll
                for (int i = 0; i < WIN; ++i)                             // channel i * 9 + j: x offset i - r, y offset j - r
                    obase[(size_t)(i * WIN + j) * mp] = hc[0][i] * Y.a0[j] + hc[1][i] * Y.a1[j] + hc[2][i] * Y.a2[j];
            }
        }
        pending = pending && !fits;
        first = false;
        if (!__any(pending)) break;
        __syncthreads();                                                  // the next round overwrites the product
    }
}

template <typename T>
static int alt_lookup(const void* scratch, const float* coords, const AltGeom& G, int map_h, int map_w, float scale, float* out, void* stream) {
    const int tiles_x = ceil_div(G.w8, ALT_TQ), tiles_y = ceil_div(G.h8, ALT_TQ);
    hipLaunchKernelGGL(k_alt_lookup<T>, dim3(tiles_x * tiles_y, G.levels, G.b), dim3(256), 0, (hipStream_t)stream, (const T*)scratch, coords, out, G, tiles_x,
                       map_h, map_w, scale);
    return rpe_check_launch();
}

extern "C" int rpe_corr_alt_lookup(const void* scratch, const float* coords, int b, int c, int h8, int w8, int levels, int radius, float* out, void* stream) {
    AltGeom G;
    if (!scratch || !coords || !out || radius != RADIUS || (((uintptr_t)scratch) & 15) || !alt_geom(b, c, h8, w8, levels, G)) return RPE_E_BADARG;
    if (b > 65535) return RPE_E_UNSUPPORTED;
    return alt_lookup<float>(scratch, coords, G, h8, w8, 1.0f, out, stream);
}

extern "C" int rpe_corr_alt_lookup_ex(const void* scratch, const float* coords, int b, int c, int h8, int w8, int levels, int radius, int map_h, int map_w,
                                      float* out, void* stream) {
    AltGeom G;
    if (!scratch || !coords || !out || radius != RADIUS || map_h < h8 || map_w < w8 || (((uintptr_t)scratch) & 15) || !alt_geom(b, c, h8, w8, levels, G))
        return RPE_E_BADARG;
    if (b > 65535) return RPE_E_UNSUPPORTED;
    return alt_lookup<float>(scratch, coords, G, map_h, map_w, 1.0f, out, stream);
}

extern "C" int rpe_corr_alt_lookup_dt(const void* scratch, const float* coords, int b, int c, int h8, int w8, int levels, int radius, int map_h, int map_w,
                                      int feature_dtype, float* out, void* stream) {
    if (feature_dtype == RPE_F32) return rpe_corr_alt_lookup_ex(scratch, coords, b, c, h8, w8, levels, radius, map_h, map_w, out, stream);
    AltGeom G;
    if (feature_dtype != RPE_F16 || !scratch || !coords || !out || radius != RADIUS || map_h < h8 || map_w < w8 || (((uintptr_t)scratch) & 15) ||
        !alt_geom(b, c, h8, w8, levels, G, 2))
        return RPE_E_BADARG;
    if (b > 65535) return RPE_E_UNSUPPORTED;
    return alt_lookup<_Float16>(scratch, coords, G, map_h, map_w, 1.0f / sqrtf((float)c), out, stream);
}
