// Surfel map of frame-to-model tracking (reference core/fusion/surfel_map.py): init, render, fuse + prune, transform.
//
// The map is SoA f32 (struct rpe_surfel_map, include/rpe.h): opts (3,cap), rgb (3,cap), conf (cap), t_created (cap), the count n in
// a device word.  Every kernel reads n from that word and is launched over a host-side upper bound; nothing here synchronises the host.
// Compactions (init, fuse's append + prune, prune) are order-preserving and deterministic: per-block counts -> one-block scan ->
// scatter with an in-block scan, never atomic slot grabs, so the map's order is the reference's (boolean-mask gathers + torch.cat).
// Compactions write from a source map into a different destination map (the caller ping-pongs two buffers): an in-place compaction
// would let a block overwrite items an earlier block has not read yet.
//
// Arithmetic follows the reference's operation order one rounding at a time (this unit is compiled with -ffp-contract=off):
//   reproject  p = depth * (Kinv . (x + .5, y + .5, 1))          pinhole_transforms.py:79-87 (Kinv: torch.linalg.inv on the host)
//   transform  R p + t, R p = p + w uv + v x uv, uv = 2 v x p    lietorch act (homogeneous w = 1 is exact)
//   project    (K . p).xy / clamp((K . p).z, 1e-12)              pinhole_transforms.py:90-100 (clamp keeps NaN)
#include "rpe_common.h"
#include "se3_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 4;                                   // consecutive items per thread in the compactions
constexpr int kTile = kThreads * kItems;                    // items per block

struct MapPtrs {
    float *opts, *rgb, *conf, *t_created;
    int64_t cap;
    int32_t *count, *overflow;
};

MapPtrs map_ptrs(const rpe_surfel_map *m) {
    MapPtrs p;
    p.opts = m->opts; p.rgb = m->rgb; p.conf = m->conf; p.t_created = m->t_created; p.cap = m->cap; p.count = m->count; p.overflow = m->overflow;
    return p;
}

__device__ __forceinline__ V3<float> mat3_mul(const float *K, const V3<float> &p) {        // row . p, left to right
    return v3<float>(K[0] * p.x + K[1] * p.y + K[2] * p.z, K[3] * p.x + K[4] * p.y + K[5] * p.z, K[6] * p.x + K[7] * p.y + K[8] * p.z);
}

// torch.clamp(z, 1e-12): NaN stays NaN (fmaxf would return 1e-12)
__device__ __forceinline__ float clamp_depth(float z) { return (z != z) ? z : (z < 1e-12f ? 1e-12f : z); }
// torch.clamp(c, 0, 1)
__device__ __forceinline__ float clamp01(float c) { return (c != c) ? c : (c < 0.f ? 0.f : (c > 1.f ? 1.f : c)); }

// image coordinates of p under K (project(): xy / clamped z)
__device__ __forceinline__ void project(const float *K, const V3<float> &p, float &u, float &v) {
    V3<float> q = mat3_mul(K, p);
    float d = clamp_depth(q.z);
    u = q.x / d;
    v = q.y / d;
}

// world point of frame pixel pix: pose . (depth * Kinv . (x + .5, y + .5, 1))
__device__ __forceinline__ V3<float> frame_point(const float *depth, const float *Kinv, const Pose<float> &P, int pix, int w) {
    float x = (float)(pix % w) + 0.5f, y = (float)(pix / w) + 0.5f;
    V3<float> r = mat3_mul(Kinv, v3<float>(x, y, 1.f));
    float d = depth[pix];
    return se3_act(P, v3<float>(d * r.x, d * r.y, d * r.z));
}

__device__ __forceinline__ V3<float> load_pt(const float *opts, int64_t cap, int64_t i) { return v3<float>(opts[i], opts[cap + i], opts[2 * cap + i]); }

// Sort key of a confidence in torch.sort's ascending order: -inf < ... < -0 == +0 < ... < +inf < NaN (all NaNs equal).  0 is never a key.
__device__ __forceinline__ uint32_t conf_key(float c) {
    if (c != c) return 0xFFFFFFFFu;
    if (c == 0.f) c = 0.f;                                  // -0 sorts with +0
    uint32_t b = __float_as_uint(c);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ------------------------------------------------------------------------------------------ compaction (init, fuse append + prune, prune)
// Items [0, n) are the source map's surfels, items [n, n + hw) the frame's pixels (append candidates).
struct CompactArgs {
    MapPtrs src;            // src.count == nullptr: no source map (init)
    MapPtrs dst;
    int64_t n_bound;        // host upper bound of *src.count
    // frame (hw == 0: no pixel items)
    const float *depth, *img, *confidence;
    const uint8_t *mask, *matched;
    int h, w;
    const float *kinv, *pose;
    float conf_thr;         // new surfel conf = confidence / conf_thr (confidence == nullptr: 1 / conf_thr)
    float t_new;            // t_created of appended surfels
    int prune;              // keep only conf >= 1 | (tick - t_created) < t_max
    float tick, t_max;
    int *block_counts;      // workspace
};

__device__ __forceinline__ int64_t src_count(const CompactArgs &a) { return a.src.count ? (int64_t)*a.src.count : 0; }

__device__ __forceinline__ bool prune_keep(const CompactArgs &a, float conf, float t) {
    return !a.prune || (conf >= 1.0f) || ((a.tick - t) < a.t_max);
}

__device__ __forceinline__ float new_conf(const CompactArgs &a, int64_t p) { return a.confidence ? a.confidence[p] / a.conf_thr : 1.0f / a.conf_thr; }

__device__ __forceinline__ bool keep_item(const CompactArgs &a, int64_t i, int64_t n) {
    if (i < n) return prune_keep(a, a.src.conf[i], a.src.t_created[i]);
    int64_t p = i - n;
    if (p >= (int64_t)a.h * a.w) return false;
    if (!a.mask[p] || (a.matched && a.matched[p])) return false;
    return prune_keep(a, new_conf(a, p), a.t_new);
}

__global__ void __launch_bounds__(kThreads) k_compact_count(CompactArgs a) {
    __shared__ int wsum[kThreads / RPE_WAVE];
    const int64_t n = src_count(a);
    const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x * kItems;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) c += keep_item(a, base + k, n);
    c = wave_sum(c);
    if ((threadIdx.x & (RPE_WAVE - 1)) == 0) wsum[threadIdx.x / RPE_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < kThreads / RPE_WAVE; ++k) s += wsum[k];
        a.block_counts[blockIdx.x] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && n > a.n_bound) atomicOr(a.dst.overflow, 2);      // the host bound was wrong: items lost
}

// One block: exclusive scan of the block counts in place (sequential per thread, then across threads), total -> *dst.count.
__global__ void __launch_bounds__(1024) k_compact_scan(CompactArgs a, int nblocks) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int lo = t * per, hi = min(nblocks, lo + per);
    int64_t s = 0;
    for (int b = lo; b < hi; ++b) s += a.block_counts[b];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int k = 0; k < 1024; ++k) { int64_t v = part[k]; part[k] = run; run += v; }
        if (run > a.dst.cap) { atomicOr(a.dst.overflow, 1); run = a.dst.cap; }
        *a.dst.count = (int32_t)run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int b = lo; b < hi; ++b) { int64_t v = a.block_counts[b]; a.block_counts[b] = (int)min(run, (int64_t)INT32_MAX); run += v; }
}

__global__ void __launch_bounds__(kThreads) k_compact_scatter(CompactArgs a) {
    __shared__ int wsum[kThreads / RPE_WAVE];
    const int64_t n = src_count(a);
    const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x * kItems;
    bool keep[kItems];
    int c = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) { keep[k] = keep_item(a, base + k, n); c += keep[k]; }
    // inclusive scan of c across the wave, then across the block's waves
    const int lane = threadIdx.x & (RPE_WAVE - 1), wave = threadIdx.x / RPE_WAVE;
    int inc = c;
#pragma unroll
    for (int off = 1; off < RPE_WAVE; off <<= 1) {
        int y = __shfl_up(inc, off, RPE_WAVE);
        if (lane >= off) inc += y;
    }
    if (lane == RPE_WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wave; ++k) before += wsum[k];
    int64_t j = (int64_t)a.block_counts[blockIdx.x] + before + inc - c;
    const int hw = a.h * a.w;
    Pose<float> P;
    if (hw) P = pose_load(a.pose);
    const float *Kinv = a.kinv;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (!keep[k]) continue;
        if (j >= a.dst.cap) { atomicOr(a.dst.overflow, 1); break; }
        const int64_t i = base + k;
        const int64_t dc = a.dst.cap;
        if (i < n) {
            const int64_t sc = a.src.cap;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                a.dst.opts[ch * dc + j] = a.src.opts[ch * sc + i];
                a.dst.rgb[ch * dc + j] = a.src.rgb[ch * sc + i];
            }
            a.dst.conf[j] = a.src.conf[i];
            a.dst.t_created[j] = a.src.t_created[i];
        } else {
            const int64_t p = i - n;
            V3<float> o = frame_point(a.depth, Kinv, P, (int)p, a.w);
            a.dst.opts[j] = o.x; a.dst.opts[dc + j] = o.y; a.dst.opts[2 * dc + j] = o.z;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) a.dst.rgb[ch * dc + j] = a.img[ch * (int64_t)hw + p];
            a.dst.conf[j] = new_conf(a, p);
            a.dst.t_created[j] = a.t_new;
        }
        ++j;
    }
}

int compact(CompactArgs a, int64_t items_bound, hipStream_t st) {
    const int64_t nb64 = (items_bound + kTile - 1) / kTile;
    if (nb64 > INT32_MAX / 2) return RPE_E_BADARG;
    const int nb = (int)(nb64 > 0 ? nb64 : 1);
    hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, a, nb);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kThreads), 0, st, a);
    return rpe_check_launch();
}

// ------------------------------------------------------------------------------------------ fuse: association + update (surfel_map.py:73-146)
struct FuseArgs {
    MapPtrs m;
    const float *depth, *img;
    const uint8_t *mask;
    uint8_t *matched;
    int h, w;
    const float *kmat, *kinv, *pose;
    float d_thresh, ccor;
    int average;
};

__global__ void __launch_bounds__(kThreads) k_fuse_update(FuseArgs a, int64_t n_bound) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_bound || i >= (int64_t)*a.m.count) return;
    const int64_t cap = a.m.cap;
    const Pose<float> P = pose_load(a.pose);
    const Pose<float> Pinv = se3_inv(P);
    V3<float> s = load_pt(a.m.opts, cap, i);
    float u, v;
    project(a.kmat, se3_act(Pinv, s), u, v);
    if (!(u >= 0.f && v >= 0.f && u < (float)(a.w - 1) && v < (float)(a.h - 1))) return;       // :108 (note the -1)
    // :111 get_match_indices: round(ipts - .5) (half to even), flattened in f32, .long()
    const float qx = rintf(u - 0.5f), qy = rintf(v - 0.5f);
    const int pix = (int)(qy * (float)a.w + qx);
    const V3<float> f = frame_point(a.depth, a.kinv, P, pix, a.w);
    if (!(fabsf(f.z - s.z) < a.d_thresh)) return;                   // :114 filter_surfels_by_correspondence
    if (!a.mask[pix]) return;                                        // :117-118
    const float c = a.m.conf[i], cc = a.ccor;
    if (a.average) {                                                 // :125-127 (c * old + cc * new) / (c + cc)
        const float den = c + cc;
        const float fv[3] = {f.x, f.y, f.z}, sv[3] = {s.x, s.y, s.z};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            a.m.opts[ch * cap + i] = (c * sv[ch] + cc * fv[ch]) / den;
            float *rgb = a.m.rgb + ch * cap + i;
            *rgb = (c * *rgb + cc * a.img[(int64_t)ch * a.h * a.w + pix]) / den;
        }
    }
    a.m.conf[i] = clamp01(c + cc);                                   // :128
    a.matched[pix] = 1;                                              // :131-132 (every writer stores 1)
}

// ------------------------------------------------------------------------------------------ render (surfel_map.py:230-264)
struct RenderArgs {
    MapPtrs m;
    int64_t n_bound;
    const float *kmat, *T;
    int depth_transformed;       // 1: depth = z of T . p (transform_cpy(T).render()); 0: depth = z of p (render(extrinsics=T))
    int h, w;
    unsigned long long *keys;    // (h*w) workspace, zeroed
    float *img, *depth, *confidence;
    uint8_t *mask;
    float gk[25];                // SparseImgInterpolator(5, 2, 0) kernel
};

__global__ void __launch_bounds__(kThreads) k_render_splat(RenderArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n_bound || i >= (int64_t)*a.m.count) return;
    float u, v;
    project(a.kmat, se3_act(pose_load(a.T), load_pt(a.m.opts, a.m.cap, i)), u, v);
    if (!(v < (float)a.h && u < (float)a.w && v >= 0.f && u >= 0.f)) return;     // project2image's valid
    const int pix = (int)v * a.w + (int)u;                                         // .long(): truncation
    // the reference scatters in argsort(conf) order, last write wins; here: largest conf, ties -> largest index (a stable sort's order)
    const unsigned long long key = ((unsigned long long)conf_key(a.m.conf[i]) << 32) | (unsigned long long)(uint32_t)i;
    atomicMax(a.keys + pix, key);
}

// value of plane c (0..2 colour, 3 depth) at pixel pix before interpolation; NaN -> 0 (the interpolator's prior) when zero_nan
__device__ __forceinline__ float rendered(const RenderArgs &a, int pix, int c, const Pose<float> &T) {
    const unsigned long long key = a.keys[pix];
    if (!key) return 0.f;
    const int64_t i = (int64_t)(uint32_t)key;
    if (c < 3) return a.m.rgb[c * a.m.cap + i];
    if (!a.depth_transformed) return a.m.opts[2 * a.m.cap + i];
    return se3_act(T, load_pt(a.m.opts, a.m.cap, i)).z;
}

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ void __launch_bounds__(kThreads) k_render_resolve(RenderArgs a) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const int hw = a.h * a.w;
    if (pix >= hw) return;
    const Pose<float> T = pose_load(a.T);
    const unsigned long long key = a.keys[pix];
    const float conf = key ? a.m.conf[(uint32_t)key] : 0.f;
    a.confidence[pix] = conf;
    a.mask[pix] = conf != 0.f;
    const int y = pix / a.w, x = pix % a.w;
    for (int c = 0; c < 4; ++c) {
        float val = rendered(a, pix, c, T);
        if (val != val) {                                            // SparseImgInterpolator: NaN -> 5x5 Gauss of the reflect-padded map
            float s = 0.f;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    float nv = rendered(a, reflect(y + dy, a.h) * a.w + reflect(x + dx, a.w), c, T);
                    if (nv != nv) nv = 0.f;
                    s += a.gk[(dy + 2) * 5 + dx + 2] * nv;
                }
            val = s;
        }
        if (c < 3) a.img[(int64_t)c * hw + pix] = val;
        else a.depth[pix] = val;
    }
}

// ------------------------------------------------------------------------------------------ transform (surfel_map.py:205-219)
__global__ void __launch_bounds__(kThreads) k_transform(const float *in, int64_t in_cap, float *out, int64_t out_cap, const int32_t *count,
                                                        int64_t n_bound, const float *T) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_bound || i >= (int64_t)*count) return;
    V3<float> p = se3_act(pose_load(T), load_pt(in, in_cap, i));
    out[i] = p.x; out[out_cap + i] = p.y; out[2 * out_cap + i] = p.z;
}

bool map_ok(const rpe_surfel_map *m) {
    return m && m->opts && m->rgb && m->conf && m->t_created && m->count && m->overflow && m->cap > 0 && m->cap <= INT32_MAX;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// SparseImgInterpolator.gauss_2d(5, 2): outer product of exp(-x^2 / 8), x = -2..2, centre 0, normalised
void gauss_kernel(float *g) {
    float g1[5], s = 0.f;
    for (int k = 0; k < 5; ++k) { float x = (float)k - 2.f; g1[k] = expf(-(x * x) / 8.f); }
    for (int r = 0; r < 5; ++r)
        for (int c = 0; c < 5; ++c) g[r * 5 + c] = (r == 2 && c == 2) ? 0.f : g1[r] * g1[c];
    for (int k = 0; k < 25; ++k) s += g[k];
    for (int k = 0; k < 25; ++k) g[k] /= s;
}

}  // namespace

extern "C" {

size_t rpe_surfel_workspace_bytes(int64_t n_bound, int h, int w) {
    if (n_bound < 0 || h <= 0 || w <= 0) return 0;
    const int64_t hw = (int64_t)h * w;
    const size_t blocks = (size_t)((n_bound + hw + kTile - 1) / kTile) + 1;
    const size_t fuse = align256((size_t)hw) + align256(blocks * sizeof(int));
    const size_t render = (size_t)hw * sizeof(unsigned long long);
    return fuse > render ? fuse : render;
}

int rpe_surfel_init(const float *depth, const float *img, const uint8_t *mask, const float *confidence, int h, int w, const float *kinv,
                    const float *pmat, float conf_thr, const rpe_surfel_map *dst, void *workspace, void *stream) {
    if (!depth || !img || !mask || !confidence || !kinv || !pmat || !map_ok(dst) || !workspace || h <= 0 || w <= 0) return RPE_E_BADARG;
    if ((int64_t)h * w > INT32_MAX / 2) return RPE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    CompactArgs a = {};
    a.dst = map_ptrs(dst);
    a.depth = depth; a.img = img; a.confidence = confidence; a.mask = mask; a.matched = nullptr;
    a.h = h; a.w = w; a.kinv = kinv; a.pose = pmat; a.conf_thr = conf_thr; a.t_new = 0.f; a.prune = 0;
    a.block_counts = (int *)workspace;
    return compact(a, (int64_t)h * w, st);
}

int rpe_surfel_fuse(const rpe_surfel_map *src, int64_t n_bound, const float *depth, const float *img, const uint8_t *mask, int h, int w,
                    const float *kmat, const float *kinv, const float *pose, float d_thresh, int average_pts, int upscale, float conf_thr,
                    int tick, int t_max, const rpe_surfel_map *dst, void *workspace, void *stream) {
    if (!map_ok(src) || !map_ok(dst) || src->opts == dst->opts || src->count == dst->count || !depth || !img || !mask || !kmat || !kinv ||
        !pose || !workspace || h <= 0 || w <= 0 || n_bound < 0 || n_bound > src->cap)
        return RPE_E_BADARG;
    if ((int64_t)h * w > INT32_MAX / 2) return RPE_E_BADARG;
    if (upscale != 1) return RPE_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w;
    uint8_t *matched = (uint8_t *)workspace;
    int *block_counts = (int *)((char *)workspace + align256((size_t)hw));
    if (hipMemsetAsync(matched, 0, (size_t)hw, st) != hipSuccess) return RPE_E_LAUNCH;
    const float ccor = 1.0f / conf_thr;                              // torch.ones_like(depth) / conf_thr
    if (n_bound > 0) {
        FuseArgs f = {};
        f.m = map_ptrs(src);
        f.depth = depth; f.img = img; f.mask = mask; f.matched = matched; f.h = h; f.w = w;
        f.kmat = kmat; f.kinv = kinv; f.pose = pose; f.d_thresh = d_thresh; f.ccor = ccor; f.average = average_pts;
        hipLaunchKernelGGL(k_fuse_update, dim3(ceil_div(n_bound, kThreads)), dim3(kThreads), 0, st, f, n_bound);
    }
    CompactArgs a = {};
    a.src = map_ptrs(src); a.dst = map_ptrs(dst); a.n_bound = n_bound;
    a.depth = depth; a.img = img; a.confidence = nullptr; a.mask = mask; a.matched = matched;
    a.h = h; a.w = w; a.kinv = kinv; a.pose = pose; a.conf_thr = conf_thr; a.t_new = (float)tick;
    a.prune = 1; a.tick = (float)(tick + 1); a.t_max = (float)t_max;          // :147 tick += 1, then :150-158
    a.block_counts = block_counts;
    return compact(a, n_bound + hw, st);
}

int rpe_surfel_prune(const rpe_surfel_map *src, int64_t n_bound, int tick, int t_max, const rpe_surfel_map *dst, void *workspace, void *stream) {
    if (!map_ok(src) || !map_ok(dst) || src->opts == dst->opts || src->count == dst->count || !workspace || n_bound < 0 || n_bound > src->cap)
        return RPE_E_BADARG;
    CompactArgs a = {};
    a.src = map_ptrs(src); a.dst = map_ptrs(dst); a.n_bound = n_bound;
    a.prune = 1; a.tick = (float)tick; a.t_max = (float)t_max;
    a.block_counts = (int *)workspace;
    return compact(a, n_bound, (hipStream_t)stream);
}

int rpe_surfel_render(const rpe_surfel_map *m, int64_t n_bound, const float *kmat, const float *T, int depth_transformed, int h, int w,
                      float *img, float *depth, float *confidence, uint8_t *mask, void *workspace, void *stream) {
    if (!map_ok(m) || !kmat || !T || !img || !depth || !confidence || !mask || !workspace || h < 3 || w < 3 || n_bound < 0 ||
        n_bound > m->cap || (int64_t)h * w > INT32_MAX / 2)
        return RPE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    RenderArgs a = {};
    a.m = map_ptrs(m); a.n_bound = n_bound; a.kmat = kmat; a.T = T; a.depth_transformed = depth_transformed ? 1 : 0;
    a.h = h; a.w = w; a.keys = (unsigned long long *)workspace;
    a.img = img; a.depth = depth; a.confidence = confidence; a.mask = mask;
    gauss_kernel(a.gk);
    const int hw = h * w;
    if (hipMemsetAsync(a.keys, 0, (size_t)hw * sizeof(unsigned long long), st) != hipSuccess) return RPE_E_LAUNCH;
    if (n_bound > 0) hipLaunchKernelGGL(k_render_splat, dim3(ceil_div(n_bound, kThreads)), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_render_resolve, dim3(ceil_div(hw, kThreads)), dim3(kThreads), 0, st, a);
    return rpe_check_launch();
}

int rpe_surfel_transform(const float *opts_in, int64_t in_cap, float *opts_out, int64_t out_cap, const int32_t *count, int64_t n_bound,
                         const float *T, void *stream) {
    if (!opts_in || !opts_out || !count || !T || in_cap <= 0 || out_cap <= 0 || n_bound < 0 || n_bound > in_cap || n_bound > out_cap)
        return RPE_E_BADARG;
    if (n_bound == 0) return RPE_OK;
    hipLaunchKernelGGL(k_transform, dim3(ceil_div(n_bound, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, opts_in, in_cap, opts_out,
                       out_cap, count, n_bound, T);
    return rpe_check_launch();
}

}  // extern "C"
