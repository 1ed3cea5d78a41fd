// Input side of the path: the per-frame preprocessing the reference runs with numpy / cv2 /
// torchvision on the CPU before PoseEstimator sees a frame.
//
// Replaces:
//   dataset/stereo_dataset.py:12-16  mask_specularities  (brightness threshold, AND with the tool mask, 11x11 erosion)
//   dataset/transforms.py:20-39      ResizeStereo        (bilinear / nearest resize that conserves the aspect ratio,
//                                                         then centre crop; torchvision 0.14: antialias off,
//                                                         align_corners=False)
//   dataset/video_dataset.py:59-61, stereo_dataset.py:35-37   uint8 HWC -> float32 CHW
// All of it is HBM-bound byte work: one read of the decoded frame, one write of the network input.
#include "rpe_common.h"

// torch rounds every operation of the bilinear formula separately; HIP's __fmul_rn / __fadd_rn are plain * and + (still
// contractable into FMAs) unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so contraction is switched off for this file.
#pragma clang fp contract(off)

#define ER 5                                   // 11x11 structuring element
#define TW 64
#define TH 16

// out = erode_11x11((r + g + b < thr) & mask).  cv2.erode's default border is +inf: pixels outside the image never erode.
__global__ __launch_bounds__(256) void k_mask_specularities(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int h, int w,
                                                            int thr, uint8_t* __restrict__ out) {
    __shared__ uint8_t tile[TH + 2 * ER][TW + 2 * ER + 2];
    __shared__ uint8_t hmin[TH + 2 * ER][TW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int i = threadIdx.x; i < (TH + 2 * ER) * (TW + 2 * ER); i += blockDim.x) {
        const int ty = i / (TW + 2 * ER), tx = i % (TW + 2 * ER);
        const int y = y0 + ty - ER, x = x0 + tx - ER;
        uint8_t v = 1;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const uint8_t* p = img + ((size_t)y * w + x) * 3;
            const int s = (int)p[0] + (int)p[1] + (int)p[2];
            v = (s < thr) && (!mask || mask[(size_t)y * w + x] != 0);
        }
        tile[ty][tx] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (TH + 2 * ER) * TW; i += blockDim.x) {
        const int ty = i / TW, tx = i % TW;
        uint8_t m = 1;
#pragma unroll
        for (int d = 0; d <= 2 * ER; ++d) m &= tile[ty][tx + d];
        hmin[ty][tx] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * TW; i += blockDim.x) {
        const int ty = i / TW, tx = i % TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= h || x >= w) continue;
        uint8_t m = 1;
#pragma unroll
        for (int d = 0; d <= 2 * ER; ++d) m &= hmin[ty + d][tx];
        out[(size_t)y * w + x] = m;
    }
}

// Source position of torch's upsample_bilinear2d (align_corners=False): scale * (dst + 0.5) - 0.5, clamped at 0.
__device__ __forceinline__ void bil(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float src = rn_sub(rn_mul(scale, rn_add((float)dst, 0.5f)), 0.5f);     // as torch rounds it: no FMA
    src = src < 0.0f ? 0.0f : src;
    i0 = (int)src;
    i0 = i0 > in_size - 1 ? in_size - 1 : i0;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = rn_sub(src, (float)i0);
    l0 = rn_sub(1.0f, l1);
}

// torch: h0lambda * (w0lambda * p00 + w1lambda * p01) + h1lambda * (w0lambda * p10 + w1lambda * p11)
// (one correctly-rounded operation at a time: no FMA contraction, so both input formats give the same bits)
__device__ __forceinline__ float bil_blend(float wx0, float wx1, float hy0, float hy1, float p00, float p01, float p10, float p11) {
    const float r0 = rn_add(rn_mul(wx0, p00), rn_mul(wx1, p01)), r1 = rn_add(rn_mul(wx0, p10), rn_mul(wx1, p11));
    return rn_add(rn_mul(hy0, r0), rn_mul(hy1, r1));
}

// out (c, oh, ow) f32 = centre crop (top, left) of bilinear resize of the input to (rh, rw).
// U8HWC: input uint8 (h, w, c) as decoded; else float32 (c, h, w).
template <bool U8HWC>
__global__ __launch_bounds__(256) void k_resize_crop(const void* __restrict__ in, int c, int h, int w, int rh, int rw, int top, int left,
                                                     int oh, int ow, float* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const float sh = rn_div((float)h, (float)rh), sw = rn_div((float)w, (float)rw);   // area_pixel_compute_scale<float>
    int y0, y1, x0, x1; float hy0, hy1, wx0, wx1;
    bil(y + top, sh, h, y0, y1, hy0, hy1);
    bil(x + left, sw, w, x0, x1, wx0, wx1);
    for (int ch = 0; ch < c; ++ch) {
        float p00, p01, p10, p11;
        if (U8HWC) {
            const uint8_t* p = (const uint8_t*)in;
            p00 = p[((size_t)y0 * w + x0) * c + ch]; p01 = p[((size_t)y0 * w + x1) * c + ch];
            p10 = p[((size_t)y1 * w + x0) * c + ch]; p11 = p[((size_t)y1 * w + x1) * c + ch];
        } else {
            const float* p = (const float*)in + (size_t)ch * h * w;
            p00 = p[(size_t)y0 * w + x0]; p01 = p[(size_t)y0 * w + x1]; p10 = p[(size_t)y1 * w + x0]; p11 = p[(size_t)y1 * w + x1];
        }
        out[((size_t)ch * oh + y) * ow + x] = bil_blend(wx0, wx1, hy0, hy1, p00, p01, p10, p11);
    }
}

// torch 'nearest': source index floor(dst * scale), scale = in / out in f32, clamped to the last pixel.  (Host and device: the fused
// ingest sizes its LDS tile on the host with the same arithmetic.)
__host__ __device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    const int s = (int)floorf((float)dst * scale);           // one multiplication: nothing to contract
    return s > in_size - 1 ? in_size - 1 : s;
}

// Nearest resize + centre crop of a one-channel byte mask: torch 'nearest' = floor(dst * scale), scale = in / out in f32.
__global__ __launch_bounds__(256) void k_resize_crop_nearest(const uint8_t* __restrict__ in, int h, int w, int rh, int rw, int top, int left,
                                                             int oh, int ow, uint8_t* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const float sh = rn_div((float)h, (float)rh), sw = rn_div((float)w, (float)rw);
    out[(size_t)y * ow + x] = in[(size_t)nearest_src(y + top, sh, h) * w + nearest_src(x + left, sw, w)];
}

extern "C" int rpe_mask_specularities(const uint8_t* img_hwc, const uint8_t* mask, int h, int w, int sum_threshold, uint8_t* out,
                                      void* stream) {
    if (!img_hwc || !out || h <= 0 || w <= 0) return RPE_E_BADARG;
    hipLaunchKernelGGL(k_mask_specularities, dim3(ceil_div(w, TW), ceil_div(h, TH)), dim3(256), 0, (hipStream_t)stream, img_hwc, mask, h, w,
                       sum_threshold, out);
    return rpe_check_launch();
}

static bool crop_ok(int rh, int rw, int top, int left, int oh, int ow) {
    return rh > 0 && rw > 0 && top >= 0 && left >= 0 && oh > 0 && ow > 0 && top + oh <= rh && left + ow <= rw;
}

extern "C" int rpe_resize_crop(const void* in, int in_is_u8_hwc, int c, int h, int w, int resized_h, int resized_w, int top, int left,
                               int out_h, int out_w, float* out, void* stream) {
    if (!in || !out || c <= 0 || h <= 0 || w <= 0 || !crop_ok(resized_h, resized_w, top, left, out_h, out_w)) return RPE_E_BADARG;
    dim3 grid(ceil_div(out_w, 256), out_h), block(256);
    if (in_is_u8_hwc) hipLaunchKernelGGL(k_resize_crop<true>, grid, block, 0, (hipStream_t)stream, in, c, h, w, resized_h, resized_w, top, left, out_h, out_w, out);
    else hipLaunchKernelGGL(k_resize_crop<false>, grid, block, 0, (hipStream_t)stream, in, c, h, w, resized_h, resized_w, top, left, out_h, out_w, out);
    return rpe_check_launch();
}

extern "C" int rpe_resize_crop_mask(const uint8_t* in, int h, int w, int resized_h, int resized_w, int top, int left, int out_h, int out_w,
                                    uint8_t* out, void* stream) {
    if (!in || !out || h <= 0 || w <= 0 || !crop_ok(resized_h, resized_w, top, left, out_h, out_w)) return RPE_E_BADARG;
    hipLaunchKernelGGL(k_resize_crop_nearest, dim3(ceil_div(out_w, 256), out_h), dim3(256), 0, (hipStream_t)stream, in, h, w, resized_h,
                       resized_w, top, left, out_h, out_w, out);
    return rpe_check_launch();
}

// ---- rectification (dataset/preprocess/stereo_rectify.py:44-51: cv2.remap(img, map1, map2, INTER_NEAREST), default border =
// constant 0).  cv2 rounds the float maps with cvRound (round half to even) and saturates to int16; a source pixel outside the
// image gives 0.  Planar (c,h,w) input of T = u8 / f32, maps (out_h,out_w) f32; HBM-bound gather, one thread per output pixel,
// all channels (the index is shared).
// cvRound + saturate_cast<short>: NaN / out-of-range land outside every image
__device__ __forceinline__ void remap_round(float fx, float fy, int& sx, int& sy) {
    const float cx = fminf(fmaxf(fx, -32768.0f), 32767.0f), cy = fminf(fmaxf(fy, -32768.0f), 32767.0f);
    sx = (fx == fx) ? __float2int_rn(cx) : -32768; sy = (fy == fy) ? __float2int_rn(cy) : -32768;
}

template <typename T>
__global__ __launch_bounds__(256) void k_remap_nearest(const T* __restrict__ src, int c, int h, int w, const float* __restrict__ mapx,
                                                       const float* __restrict__ mapy, int oh, int ow, T* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const size_t o = (size_t)y * ow + x;
    const float fx = __builtin_nontemporal_load(mapx + o), fy = __builtin_nontemporal_load(mapy + o);
    int sx, sy;
    remap_round(fx, fy, sx, sy);
    const bool in = sx >= 0 && sx < w && sy >= 0 && sy < h;
    const size_t si = in ? (size_t)sy * w + sx : 0;
    for (int ch = 0; ch < c; ++ch) {
        const T v = in ? src[(size_t)ch * h * w + si] : (T)0;
        __builtin_nontemporal_store(v, dst + (size_t)ch * oh * ow + o);
    }
}

extern "C" int rpe_remap_nearest(const void* src, int src_is_u8, int c, int h, int w, const float* mapx, const float* mapy, int out_h, int out_w,
                                 void* dst, void* stream) {
    if (!src || !dst || !mapx || !mapy || c <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return RPE_E_BADARG;
    dim3 grid(ceil_div(out_w, 256), out_h), block(256);
    if (src_is_u8) hipLaunchKernelGGL(k_remap_nearest<uint8_t>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)src, c, h, w, mapx, mapy, out_h, out_w, (uint8_t*)dst);
    else hipLaunchKernelGGL(k_remap_nearest<float>, grid, block, 0, (hipStream_t)stream, (const float*)src, c, h, w, mapx, mapy, out_h, out_w, (float*)dst);
    return rpe_check_launch();
}

// Pseudo-rectification (dataset/preprocess/stereo_rectify.py:52-59 pseudo_rectify_2d, used by dataset/rectification.py:55-58 for
// mode='pseudo'): cv2.warpAffine(img, [[1, 0, tx], [0, 1, ty]], (w, h)) with its defaults INTER_LINEAR / BORDER_CONSTANT(0).
// OpenCV 4.x imgwarp.cpp, restated: the matrix is inverted (source = dst - t), source coordinates are fixed point with
// AB_BITS = 10 and rounded to 1/32 pixel -- X = (cvRound(-tx * 1024) + 16 + 1024 x) >> 5, integer part X >> 5, fraction X & 31 --
// and the four taps are blended with the 5-bit bilinear table: integer weights (32-a)(32-b), a(32-b), (32-a)b, ab times 32
// (sum 2^15), result (sum + 2^14) >> 15 for uint8; float images use the table's float weights and a float sum.  Taps outside
// the image contribute the border value 0.  host side passes X0 = cvRound(-tx*1024) + 16, Y0c = the per-row constants' -ty term:
// Y0(y) = cvRound((y - ty) * 1024) + 16 is computed per row in double, as OpenCV does.
// source pixel (sx, sy) and 1/32-pixel fractions (ax, ay) of output pixel (x, y)
__device__ __forceinline__ void shift_coords(int x, int y, int X0, double mty, int& sx, int& sy, int& ax, int& ay) {
    const int Y0 = (int)__double2ll_rn(((double)y + mty) * 1024.0) + 16;       // saturate_cast<int>(double) = cvRound: round half to even
    const int X = (X0 + x * 1024) >> 5, Y = Y0 >> 5;                           // arithmetic shifts: floor
    sx = X >> 5; sy = Y >> 5;
    sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx); sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);   // saturate_cast<short>
    ax = X & 31; ay = Y & 31;
}

// float images: the table's float weights and a float sum
__device__ __forceinline__ float shift_blend_f32(float p00, float p01, float p10, float p11, int ax, int ay) {
    const float fx = (float)ax * (1.0f / 32.0f), fy = (float)ay * (1.0f / 32.0f);
    const float w00 = (1.0f - fy) * (1.0f - fx), w01 = (1.0f - fy) * fx, w10 = fy * (1.0f - fx), w11 = fy * fx;
    // (rn_*: __fmul_rn / __fadd_rn are contractable where they are inlined; the sum stays four products and three additions)
    return rn_add(rn_add(rn_add(rn_mul(p00, w00), rn_mul(p01, w01)), rn_mul(p10, w10)), rn_mul(p11, w11));
}

// X0 = cvRound(-tx * 1024) + 16 and mty = -ty in double as warpAffine inverts the matrix; RPE_E_UNSUPPORTED beyond the fixed point's range
static int shift_setup(float tx, float ty, int* X0, double* mty) {
    const double mtx = -(double)tx;
    *mty = -(double)ty;
    const double sx = mtx * 1024.0;
    if (!(fabs(sx) < 2.0e9) || !(fabs(*mty) < 1.0e6)) return RPE_E_UNSUPPORTED;
    *X0 = (int)llrint(sx) + 16;                                               // cvRound: round half to even (default FP environment)
    return RPE_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void k_shift_bilinear(const T* __restrict__ src, int c, int h, int w, int X0, double mty, T* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    int sx, sy, ax, ay;
    shift_coords(x, y, X0, mty, sx, sy, ax, ay);
    const bool x0ok = sx >= 0 && sx < w, x1ok = sx + 1 >= 0 && sx + 1 < w, y0ok = sy >= 0 && sy < h, y1ok = sy + 1 >= 0 && sy + 1 < h;
    const size_t o = (size_t)y * w + x;
    for (int ch = 0; ch < c; ++ch) {
        const T* p = src + (size_t)ch * h * w;
        const T p00 = (x0ok && y0ok) ? p[(size_t)sy * w + sx] : (T)0, p01 = (x1ok && y0ok) ? p[(size_t)sy * w + sx + 1] : (T)0;
        const T p10 = (x0ok && y1ok) ? p[(size_t)(sy + 1) * w + sx] : (T)0, p11 = (x1ok && y1ok) ? p[(size_t)(sy + 1) * w + sx + 1] : (T)0;
        if constexpr (sizeof(T) == 1) {
            const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
            const int v = (w00 * (int)p00 + w01 * (int)p01 + w10 * (int)p10 + w11 * (int)p11 + (1 << 14)) >> 15;
            dst[(size_t)ch * h * w + o] = (T)(v < 0 ? 0 : (v > 255 ? 255 : v));
        } else {
            dst[(size_t)ch * h * w + o] = shift_blend_f32(p00, p01, p10, p11, ax, ay);
        }
    }
}

extern "C" int rpe_shift_bilinear(const void* src, int src_is_u8, int c, int h, int w, float tx, float ty, void* dst, void* stream) {
    if (!src || !dst || c <= 0 || h <= 0 || w <= 0 || !(tx == tx) || !(ty == ty)) return RPE_E_BADARG;
    // the inverse of [[1,0,tx],[0,1,ty]] in double, as warpAffine computes it: b1 = -tx, b2 = -ty (exact)
    int X0; double mty;
    if (int st = shift_setup(tx, ty, &X0, &mty)) return st;
    dim3 grid(ceil_div(w, 256), h), block(256);
    if (src_is_u8) hipLaunchKernelGGL(k_shift_bilinear<uint8_t>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)src, c, h, w, X0, mty, (uint8_t*)dst);
    else hipLaunchKernelGGL(k_shift_bilinear<float>, grid, block, 0, (hipStream_t)stream, (const float*)src, c, h, w, X0, mty, (float*)dst);
    return rpe_check_launch();
}

// ---- one-call ingest: n decoded stereo frames -> the tracker's inputs.  The chain mask_specularities -> ResizeStereo ->
// StereoRectifier (dataset/video_dataset.py:55-66, dataset/stereo_dataset.py:27-41) evaluated per OUTPUT pixel, bit for bit:
//   image: the rectification (a nearest gather, or the pseudo shift's four taps) picks pixels of the resized-and-cropped image,
//          each of which is one bilinear sample of the decoded frame (bil / bil_blend); pixels outside that image are 0;
//   mask:  never rectified; the nearest resize picks source pixel (ys, xs), whose eroded value is the AND of the predicate
//          (r + g + b < thr) & user_mask over the 11x11 window around it (pixels outside the image never erode).
// One workgroup per 64x16 output tile.  The predicate of the tile's source footprint (the picked pixels plus the 5-pixel halo) is
// staged in LDS from whole-dword loads of the 3-byte pixels; the erosion runs there as a separable AND, evaluated only at the
// columns and rows the resize picks.  The only global memory written is the three outputs.
#define RPE_INGEST_LDS_MAX (64 * 1024)

struct ingest_args {
    const uint8_t *lbase, *rbase;              // left / right eye: pixel p of frame i is at base + 3 * (i * frame_px + off_px + p)
    long long frame_px, roff_px;               //   stacked: same base, frame_px = 2 h w, roff_px = h w; two pointers: h w and 0
    long long lbytes, rbytes;                  // bytes behind each base (wide loads stop there), 0: base not dword aligned, byte loads only
    const uint8_t* umask;                      // (n, h, w) or null
    int h, w, bgr, thr;
    int rh, rw, top, left, oh, ow;
    int mode;
    const float *lmapx, *lmapy, *rmapx, *rmapy;
    int X0; double mty;                        // pseudo: shift_setup
    int fw, fh;                                // LDS tile: widest / tallest source footprint of any workgroup (ingest_footprint)
    float *limg, *rimg; uint8_t* mask;
};

// Pixels L and L + dx (dx = 0 / 1) of an HWC uint8 buffer as (r, g, b) floats: three aligned dwords cover both, the bytes are
// picked with 64-bit shifts.  Falls back to byte loads where the dwords would cross the end of the buffer.
__device__ __forceinline__ void load_px2(const uint8_t* __restrict__ base, long long bytes, long long L, int dx, int bgr, float p0[3], float p1[3]) {
    const long long b = 3 * L;
    const long long a = b & ~3LL;
    if (a + 12 <= bytes) {
        const uint32_t* q = (const uint32_t*)(base + a);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        const int o0 = (int)(b & 3), o1 = o0 + 3 * dx;
        const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w1 | ((uint64_t)w2 << 32);
        const uint32_t v0 = (uint32_t)(lo >> (8 * o0));
        const uint32_t v1 = (uint32_t)((o1 < 4 ? lo : hi) >> (8 * (o1 & 3)));
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int s = 8 * (bgr ? 2 - ch : ch);
            p0[ch] = (float)((v0 >> s) & 255u); p1[ch] = (float)((v1 >> s) & 255u);
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int s = bgr ? 2 - ch : ch;
            p0[ch] = (float)base[b + s]; p1[ch] = (float)base[b + 3 * dx + s];
        }
    }
}

// One pixel (yr, xr) of the resized-and-cropped (oh, ow) image, all three channels; 0 outside it.
__device__ __forceinline__ void ingest_sample(const uint8_t* __restrict__ base, long long bytes, long long px0, const ingest_args& a, float sh,
                                              float sw, int yr, int xr, float v[3]) {
    if (yr < 0 || yr >= a.oh || xr < 0 || xr >= a.ow) { v[0] = v[1] = v[2] = 0.0f; return; }
    int y0, y1, x0, x1; float hy0, hy1, wx0, wx1;
    bil(yr + a.top, sh, a.h, y0, y1, hy0, hy1);
    bil(xr + a.left, sw, a.w, x0, x1, wx0, wx1);
    float p00[3], p01[3], p10[3], p11[3];
    load_px2(base, bytes, px0 + (long long)y0 * a.w + x0, x1 - x0, a.bgr, p00, p01);
    load_px2(base, bytes, px0 + (long long)y1 * a.w + x0, x1 - x0, a.bgr, p10, p11);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = bil_blend(wx0, wx1, hy0, hy1, p00[ch], p01[ch], p10[ch], p11[ch]);
}

// Output pixel (y, x) of one eye after rectification.
__device__ __forceinline__ void ingest_pixel(const uint8_t* __restrict__ base, long long bytes, long long px0, const ingest_args& a, float sh,
                                             float sw, const float* __restrict__ mapx, const float* __restrict__ mapy, bool shift, int y, int x,
                                             float v[3]) {
    if (a.mode == RPE_INGEST_RECT_MAPS) {
        int sx, sy;
        remap_round(mapx[(size_t)y * a.ow + x], mapy[(size_t)y * a.ow + x], sx, sy);
        ingest_sample(base, bytes, px0, a, sh, sw, sy, sx, v);
    } else if (shift) {
        int sx, sy, ax, ay;
        shift_coords(x, y, a.X0, a.mty, sx, sy, ax, ay);
        float p00[3], p01[3], p10[3], p11[3];
        ingest_sample(base, bytes, px0, a, sh, sw, sy, sx, p00); ingest_sample(base, bytes, px0, a, sh, sw, sy, sx + 1, p01);
        ingest_sample(base, bytes, px0, a, sh, sw, sy + 1, sx, p10); ingest_sample(base, bytes, px0, a, sh, sw, sy + 1, sx + 1, p11);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = shift_blend_f32(p00[ch], p01[ch], p10[ch], p11[ch], ax, ay);
    } else {
        ingest_sample(base, bytes, px0, a, sh, sw, y, x, v);
    }
}

__global__ __launch_bounds__(256) void k_ingest_stereo(const ingest_args a) {
    extern __shared__ __align__(16) uint8_t ingest_lds[];
    const int fwp = (a.fw + 3) & ~3;                            // row pitch of the predicate tile
    uint8_t* tile = ingest_lds;                                 // [fh][fwp]  predicate of the source footprint
    uint8_t* hmin = ingest_lds + (size_t)a.fh * fwp;            // [fh][TW]   its AND over the 11 columns around each picked column
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, n = blockIdx.z;
    const int xl = min(x0 + TW, a.ow) - 1, yl = min(y0 + TH, a.oh) - 1;
    const float sh = rn_div((float)a.h, (float)a.rh), sw = rn_div((float)a.w, (float)a.rw);   // area_pixel_compute_scale<float>
    const long long lpx0 = (long long)n * a.frame_px, rpx0 = lpx0 + a.roff_px;

    // ---- mask: predicate of the footprint -> LDS
    const int fx0 = nearest_src(x0 + a.left, sw, a.w) - ER, fy0 = nearest_src(y0 + a.top, sh, a.h) - ER;
    const int fw = min(nearest_src(xl + a.left, sw, a.w) - fx0 + 1 + ER, a.fw), fh = min(nearest_src(yl + a.top, sh, a.h) - fy0 + 1 + ER, a.fh);
    for (int i = threadIdx.x; i < a.fh * fwp / 4; i += blockDim.x) ((uint32_t*)tile)[i] = 0x01010101u;      // outside the image: never erodes
    __syncthreads();
    const int cx0 = max(fx0, 0), cx1 = min(fx0 + fw, a.w);      // the footprint's columns inside the image
    if (cx1 > cx0) {
        const int groups = (cx1 - cx0 + 3) / 4 + 1;             // aligned groups of 4 pixels (12 bytes) a row of the footprint can touch
        for (int i = threadIdx.x; i < fh * groups; i += blockDim.x) {
            const int r = i / groups, sy = fy0 + r;
            if (sy < 0 || sy >= a.h) continue;
            const long long Lrow = lpx0 + (long long)sy * a.w;
            const long long g = ((Lrow + cx0) >> 2) + (i - r * groups);
            if (4 * g >= Lrow + cx1) continue;
            int s[4];
            if (12 * g + 12 <= a.lbytes) {
                const uint32_t* q = (const uint32_t*)(a.lbase + 12 * g);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
                s[0] = (w0 & 255u) + ((w0 >> 8) & 255u) + ((w0 >> 16) & 255u);
                s[1] = (w0 >> 24) + (w1 & 255u) + ((w1 >> 8) & 255u);
                s[2] = ((w1 >> 16) & 255u) + (w1 >> 24) + (w2 & 255u);
                s[3] = ((w2 >> 8) & 255u) + ((w2 >> 16) & 255u) + (w2 >> 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long long L = 4 * g + j;
                    s[j] = (L >= Lrow + cx0 && L < Lrow + cx1) ? (int)a.lbase[3 * L] + (int)a.lbase[3 * L + 1] + (int)a.lbase[3 * L + 2] : 0;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = (int)(4 * g + j - Lrow);
                if (x < cx0 || x >= cx1) continue;
                tile[r * fwp + (x - fx0)] = (s[j] < a.thr) && (!a.umask || a.umask[((size_t)n * a.h + sy) * a.w + x] != 0);
            }
        }
    }
    __syncthreads();
    // AND over the 11 columns around the column each output column picks
    for (int i = threadIdx.x; i < fh * TW; i += blockDim.x) {
        const int r = i / TW, tx = i % TW;
        if (x0 + tx > xl) continue;
        const uint8_t* t = tile + r * fwp + (nearest_src(x0 + tx + a.left, sw, a.w) - ER - fx0);
        uint8_t m = 1;
#pragma unroll
        for (int d = 0; d <= 2 * ER; ++d) m &= t[d];
        hmin[r * TW + tx] = m;
    }
    __syncthreads();

    // ---- four consecutive output pixels of one row per thread: 16-byte stores of the images, a 4-byte store of the mask
    const int tx = (threadIdx.x % (TW / 4)) * 4, ty = threadIdx.x / (TW / 4);
    const int x = x0 + tx, y = y0 + ty;
    if (y > yl || x > xl) return;
    const bool vec = (a.ow & 3) == 0;                           // rows stay 16-byte aligned (the outputs' bases are: checked on the host)
    const int cnt = min(4, a.ow - x);
    {
        const int ry = nearest_src(y + a.top, sh, a.h) - ER - fy0;
        uint8_t m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = 1;
            if (j < cnt) {
#pragma unroll
                for (int d = 0; d <= 2 * ER; ++d) m[j] &= hmin[(ry + d) * TW + tx + j];
            }
        }
        uint8_t* o = a.mask + ((size_t)n * a.oh + y) * a.ow + x;
        if (vec) *(uint32_t*)o = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
        else for (int j = 0; j < cnt; ++j) o[j] = m[j];
    }
#pragma unroll
    for (int eye = 0; eye < 2; ++eye) {
        const uint8_t* base = eye ? a.rbase : a.lbase;
        const long long bytes = eye ? a.rbytes : a.lbytes, px0 = eye ? rpx0 : lpx0;
        const float *mapx = eye ? a.rmapx : a.lmapx, *mapy = eye ? a.rmapy : a.lmapy;
        float v[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) ingest_pixel(base, bytes, px0, a, sh, sw, mapx, mapy, eye == 1 && a.mode == RPE_INGEST_RECT_SHIFT, y, x + j, v[j]);
            else v[j][0] = v[j][1] = v[j][2] = 0.0f;
        float* o = (eye ? a.rimg : a.limg) + (((size_t)n * 3) * a.oh + y) * a.ow + x;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch, o += (size_t)a.oh * a.ow) {
            if (vec) *(float4*)o = make_float4(v[0][ch], v[1][ch], v[2][ch], v[3][ch]);
            else for (int j = 0; j < cnt; ++j) o[j] = v[j][ch];
        }
    }
}

// Widest source footprint (picked pixels + halo) of any tile along one axis, with the kernel's own arithmetic.
static int ingest_footprint(int out, int off, int in, int resized, int tile) {
    const float scale = (float)in / (float)resized;
    int m = 0;
    for (int o0 = 0; o0 < out; o0 += tile) {
        const int ol = (o0 + tile < out ? o0 + tile : out) - 1;
        const int f = nearest_src(ol + off, scale, in) - nearest_src(o0 + off, scale, in) + 1 + 2 * ER;
        m = f > m ? f : m;
    }
    return m;
}

extern "C" int rpe_ingest_stereo(const uint8_t* frames, const uint8_t* right, int n, int h, int w, int bgr, const uint8_t* user_mask,
                                 int sum_threshold, int resized_h, int resized_w, int top, int left, int out_h, int out_w, int rect_mode,
                                 const float* lmapx, const float* lmapy, const float* rmapx, const float* rmapy, float tx, float ty,
                                 float* limg, float* rimg, uint8_t* mask, void* stream) {
    if (!frames || !limg || !rimg || !mask || n <= 0 || n > 65535 || h <= 0 || w <= 0 || !crop_ok(resized_h, resized_w, top, left, out_h, out_w))
        return RPE_E_BADARG;
    if (rect_mode != RPE_INGEST_RECT_NONE && rect_mode != RPE_INGEST_RECT_MAPS && rect_mode != RPE_INGEST_RECT_SHIFT) return RPE_E_BADARG;
    if (rect_mode == RPE_INGEST_RECT_MAPS && (!lmapx || !lmapy || !rmapx || !rmapy)) return RPE_E_BADARG;
    if (rect_mode == RPE_INGEST_RECT_SHIFT && (!(tx == tx) || !(ty == ty))) return RPE_E_BADARG;
    if ((long long)h * w > (1LL << 28)) return RPE_E_UNSUPPORTED;
    ingest_args a = {};
    const long long hw = (long long)h * w;
    a.lbase = frames; a.rbase = right ? right : frames;
    a.frame_px = right ? hw : 2 * hw; a.roff_px = right ? 0 : hw;
    // whole-dword loads need a dword-aligned base; a 4-pixel group is then 12 aligned bytes wherever the rows start
    a.lbytes = ((uintptr_t)a.lbase & 3) ? 0 : 3 * a.frame_px * n;
    a.rbytes = ((uintptr_t)a.rbase & 3) ? 0 : 3 * a.frame_px * n;
    a.umask = user_mask; a.h = h; a.w = w; a.bgr = bgr != 0; a.thr = sum_threshold;
    a.rh = resized_h; a.rw = resized_w; a.top = top; a.left = left; a.oh = out_h; a.ow = out_w;
    a.mode = rect_mode; a.lmapx = lmapx; a.lmapy = lmapy; a.rmapx = rmapx; a.rmapy = rmapy;
    if (rect_mode == RPE_INGEST_RECT_SHIFT)
        if (int st = shift_setup(tx, ty, &a.X0, &a.mty)) return st;
    a.fw = ingest_footprint(out_w, left, w, resized_w, TW); a.fh = ingest_footprint(out_h, top, h, resized_h, TH);
    const size_t lds = (size_t)a.fh * ((a.fw + 3) & ~3) + (size_t)a.fh * TW;
    if (lds > RPE_INGEST_LDS_MAX) return RPE_E_UNSUPPORTED;        // a reduction of more than about 8:1 per axis
    if ((out_w & 3) == 0 && ((((uintptr_t)limg | (uintptr_t)rimg) & 15) || ((uintptr_t)mask & 3))) return RPE_E_BADARG;
    a.limg = limg; a.rimg = rimg; a.mask = mask;
    hipLaunchKernelGGL(k_ingest_stereo, dim3(ceil_div(out_w, TW), ceil_div(out_h, TH), n), dim3(256), lds, (hipStream_t)stream, a);
    return rpe_check_launch();
}
