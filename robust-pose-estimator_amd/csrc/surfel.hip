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
#include <string.h>

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

// The kernel bodies below take the block index within their map (blk): the single-map kernels pass blockIdx.x, the batched ones
// (rpe_surfel_*_many) the block's offset inside its map's segment of the grid, so both run the same code per map.
__device__ __forceinline__ void compact_count(const CompactArgs &a, int blk) {
    __shared__ int wsum[kThreads / RPE_WAVE];
    const int64_t n = src_count(a);
    const int64_t base = (int64_t)blk * kTile + threadIdx.x * kItems;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) c += keep_item(a, base + k, n);
    c = wave_sum(c);
    if ((threadIdx.x & (RPE_WAVE - 1)) == 0) wsum[threadIdx.x / RPE_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < kThreads / RPE_WAVE; ++k) s += wsum[k];
        a.block_counts[blk] = s;
    }
    if (blk == 0 && threadIdx.x == 0 && n > a.n_bound) atomicOr(a.dst.overflow, 2);      // the host bound was wrong: items lost
}

// One block: exclusive scan of the block counts in place (sequential per thread, then across threads), total -> *dst.count.
__device__ __forceinline__ void compact_scan(const CompactArgs &a, int nblocks) {
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

__device__ __forceinline__ void compact_scatter(const CompactArgs &a, int blk) {
    __shared__ int wsum[kThreads / RPE_WAVE];
    const int64_t n = src_count(a);
    const int64_t base = (int64_t)blk * kTile + threadIdx.x * kItems;
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
    int64_t j = (int64_t)a.block_counts[blk] + before + inc - c;
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

__global__ void __launch_bounds__(kThreads) k_compact_count(CompactArgs a) { compact_count(a, blockIdx.x); }
__global__ void __launch_bounds__(1024) k_compact_scan(CompactArgs a, int nblocks) { compact_scan(a, nblocks); }
__global__ void __launch_bounds__(kThreads) k_compact_scatter(CompactArgs a) { compact_scatter(a, blockIdx.x); }

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

__device__ __forceinline__ void fuse_update(const FuseArgs &a, int64_t n_bound, int blk) {
    const int64_t i = (int64_t)blk * kThreads + threadIdx.x;
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

__global__ void __launch_bounds__(kThreads) k_fuse_update(FuseArgs a, int64_t n_bound) { fuse_update(a, n_bound, blockIdx.x); }

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

__device__ __forceinline__ void render_splat(const RenderArgs &a, int blk) {
    const int64_t i = (int64_t)blk * kThreads + threadIdx.x;
    if (i >= a.n_bound || i >= (int64_t)*a.m.count) return;
    float u, v;
    project(a.kmat, se3_act(pose_load(a.T), load_pt(a.m.opts, a.m.cap, i)), u, v);
    if (!(v < (float)a.h && u < (float)a.w && v >= 0.f && u >= 0.f)) return;     // project2image's valid
    const int pix = (int)v * a.w + (int)u;                                         // .long(): truncation
    // the reference scatters in argsort(conf) order, last write wins; here: largest conf, ties -> largest index (a stable sort's order)
    const unsigned long long key = ((unsigned long long)conf_key(a.m.conf[i]) << 32) | (unsigned long long)(uint32_t)i;
    atomicMax(a.keys + pix, key);
}

__global__ void __launch_bounds__(kThreads) k_render_splat(RenderArgs a) { render_splat(a, blockIdx.x); }

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

__device__ __forceinline__ void render_resolve(const RenderArgs &a, int blk) {
    const int pix = blk * kThreads + threadIdx.x;
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

__global__ void __launch_bounds__(kThreads) k_render_resolve(RenderArgs a) { render_resolve(a, blockIdx.x); }

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

// ------------------------------------------------------------------------------------------ K maps per launch (rpe_surfel_*_many)
// Each stage of the single-map calls becomes one launch over all maps.  The maps' argument structs (the single-map kernels' own:
// CompactArgs, FuseArgs, RenderArgs) and the prefix of their block counts form a table at the head of the workspace, written there by
// k_put launches that carry it by value: no host-to-device copy, so the calls stay graph-capturable.  A block of a per-surfel or
// compaction kernel finds its map by binary search in the prefix and runs the single-map body with its block index inside the map's
// segment of the grid: every map gets exactly the arithmetic, the counts and the order of the single-map call.
constexpr int kMaxMaps = RPE_SURFEL_MAX_MAPS;

struct ManyHead {
    int nmaps;
    int off_a[kMaxMaps + 1];     // per-surfel kernels (render splat, fuse update): prefix of the maps' block counts
    int off_b[kMaxMaps + 1];     // compactions: prefix of the maps' block counts = the maps' segments of block_counts
    int64_t bound[kMaxMaps];     // fuse update: n_bound of each map
};

constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
constexpr size_t cmax(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t kStageBytes = align16(sizeof(ManyHead)) + kMaxMaps * cmax(align16(sizeof(RenderArgs)), align16(sizeof(FuseArgs)) + align16(sizeof(CompactArgs))) + 64;
constexpr size_t kTableBytes = (kStageBytes + 255) & ~(size_t)255;                  // the workspace's head; the single-map layouts follow

// host image of the table; arrays are appended after the head at 16-byte alignment
struct Staging {
    alignas(16) unsigned char bytes[kStageBytes];
    size_t used = align16(sizeof(ManyHead));
    Staging() { memset(bytes, 0, used); }
    ManyHead &head() { return *reinterpret_cast<ManyHead *>(bytes); }
    template <typename T> size_t add(int n) {
        const size_t at = align16(used);
        used = at + sizeof(T) * (size_t)n;
        return at;
    }
    template <typename T> T *at(size_t off) { return reinterpret_cast<T *>(bytes + off); }
};

constexpr int kPutWords = 256;                                 // 2 KiB of kernel arguments per k_put launch
struct PutChunk { uint64_t w[kPutWords]; };

__global__ void __launch_bounds__(kPutWords) k_put(uint64_t *dst, PutChunk c, int nwords) {
    if ((int)threadIdx.x < nwords) dst[threadIdx.x] = c.w[threadIdx.x];
}

int put_table(const Staging &s, void *workspace, hipStream_t st) {
    const size_t words = (s.used + 7) / 8;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(s.bytes);
    for (size_t w0 = 0; w0 < words; w0 += kPutWords) {
        PutChunk c;
        const int nw = (int)(words - w0 < (size_t)kPutWords ? words - w0 : kPutWords);
        memcpy(c.w, src + w0, sizeof(uint64_t) * nw);
        hipLaunchKernelGGL(k_put, dim3(1), dim3(kPutWords), 0, st, (uint64_t *)workspace + w0, c, nw);
    }
    return rpe_check_launch();
}

// the map whose segment [off[k], off[k+1]) holds block b (empty segments are skipped)
__device__ __forceinline__ int find_map(const int *off, int nmaps, int b) {
    int lo = 0, hi = nmaps - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads) k_render_splat_many(const ManyHead *h, const RenderArgs *r) {
    const int k = find_map(h->off_a, h->nmaps, blockIdx.x);
    render_splat(r[k], blockIdx.x - h->off_a[k]);
}
__global__ void __launch_bounds__(kThreads) k_render_resolve_many(const RenderArgs *r) { render_resolve(r[blockIdx.y], blockIdx.x); }
__global__ void __launch_bounds__(kThreads) k_fuse_update_many(const ManyHead *h, const FuseArgs *f) {
    const int k = find_map(h->off_a, h->nmaps, blockIdx.x);
    fuse_update(f[k], h->bound[k], blockIdx.x - h->off_a[k]);
}
__global__ void __launch_bounds__(kThreads) k_compact_count_many(const ManyHead *h, const CompactArgs *c) {
    const int k = find_map(h->off_b, h->nmaps, blockIdx.x);
    compact_count(c[k], blockIdx.x - h->off_b[k]);
}
// one workgroup per map segment
__global__ void __launch_bounds__(1024) k_compact_scan_many(const ManyHead *h, const CompactArgs *c) {
    compact_scan(c[blockIdx.x], h->off_b[blockIdx.x + 1] - h->off_b[blockIdx.x]);
}
__global__ void __launch_bounds__(kThreads) k_compact_scatter_many(const ManyHead *h, const CompactArgs *c) {
    const int k = find_map(h->off_b, h->nmaps, blockIdx.x);
    compact_scatter(c[k], blockIdx.x - h->off_b[k]);
}

// the compaction blocks of a map with items_bound items (compact()'s count); false when the grid would be too large
bool compact_blocks(int64_t items_bound, int64_t &total, int &nb) {
    const int64_t nb64 = (items_bound + kTile - 1) / kTile;
    nb = (int)(nb64 > 0 ? (nb64 < INT32_MAX / 2 ? nb64 : INT32_MAX / 2) : 1);
    total += nb;
    return nb64 <= INT32_MAX / 2 && total <= INT32_MAX / 2;
}

int compact_many(Staging &s, size_t cmp_at, void *workspace, hipStream_t st) {
    const ManyHead &hd = s.head();
    const int nmaps = hd.nmaps, total = hd.off_b[nmaps];
    const ManyHead *h = (const ManyHead *)workspace;
    const CompactArgs *c = (const CompactArgs *)((char *)workspace + cmp_at);
    hipLaunchKernelGGL(k_compact_count_many, dim3(total), dim3(kThreads), 0, st, h, c);
    hipLaunchKernelGGL(k_compact_scan_many, dim3(nmaps), dim3(1024), 0, st, h, c);
    hipLaunchKernelGGL(k_compact_scatter_many, dim3(total), dim3(kThreads), 0, st, h, c);
    return rpe_check_launch();
}

// no two of the n maps share storage (the batched kernels of one launch would race on it)
bool maps_disjoint(const rpe_surfel_map *a, const rpe_surfel_map *b, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const rpe_surfel_map *x[2] = {&a[i], b ? &b[i] : nullptr}, *y[2] = {&a[j], b ? &b[j] : nullptr};
            for (int p = 0; p < 2; ++p)
                for (int q = 0; q < 2; ++q) {
                    if (!x[p] || !y[q] || (i == j && p == q)) continue;
                    if (x[p]->opts == y[q]->opts || x[p]->count == y[q]->count) return false;
                }
        }
    return true;
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

size_t rpe_surfel_workspace_bytes_many(int nmaps, const int64_t *n_bounds, int h, int w) {
    if (nmaps <= 0 || nmaps > kMaxMaps || !n_bounds) return 0;
    size_t s = kTableBytes;
    for (int k = 0; k < nmaps; ++k) {
        const size_t b = rpe_surfel_workspace_bytes(n_bounds[k], h, w);
        if (!b) return 0;
        s += b;
    }
    return s;
}

int rpe_surfel_init_many(int nmaps, const float *depth, const float *img, const uint8_t *mask, const float *confidence, int h, int w,
                         const float *const *kinv, const float *pmat, float conf_thr, const rpe_surfel_map *dst, void *workspace,
                         void *stream) {
    if (nmaps < 0 || nmaps > kMaxMaps) return RPE_E_BADARG;
    if (nmaps == 0) return RPE_OK;
    if (!depth || !img || !mask || !confidence || !kinv || !pmat || !dst || !workspace || h <= 0 || w <= 0) return RPE_E_BADARG;
    if ((int64_t)h * w > INT32_MAX / 2) return RPE_E_BADARG;
    for (int k = 0; k < nmaps; ++k)
        if (!kinv[k] || !map_ok(&dst[k])) return RPE_E_BADARG;
    if (!maps_disjoint(dst, nullptr, nmaps)) return RPE_E_BADARG;
    const int64_t hw = (int64_t)h * w;
    Staging s;
    ManyHead &hd = s.head();
    hd.nmaps = nmaps;
    const size_t cmp_at = s.add<CompactArgs>(nmaps);
    CompactArgs *c = s.at<CompactArgs>(cmp_at);
    int *block_counts = (int *)((char *)workspace + kTableBytes);
    int64_t total = 0;
    hd.off_b[0] = 0;
    for (int k = 0; k < nmaps; ++k) {
        int nb;
        if (!compact_blocks(hw, total, nb)) return RPE_E_BADARG;
        hd.off_b[k + 1] = (int)total;
        CompactArgs a = {};
        a.dst = map_ptrs(&dst[k]);
        a.depth = depth + k * hw; a.img = img + 3 * k * hw; a.confidence = confidence + k * hw; a.mask = mask + k * hw; a.matched = nullptr;
        a.h = h; a.w = w; a.kinv = kinv[k]; a.pose = pmat + 7 * k; a.conf_thr = conf_thr; a.t_new = 0.f; a.prune = 0;
        a.block_counts = block_counts + hd.off_b[k];
        c[k] = a;
    }
    hipStream_t st = (hipStream_t)stream;
    if (put_table(s, workspace, st) != RPE_OK) return RPE_E_LAUNCH;
    return compact_many(s, cmp_at, workspace, st);
}

int rpe_surfel_fuse_many(int nmaps, const rpe_surfel_map *src, const int64_t *n_bounds, const rpe_surfel_map *dst, const int32_t *ticks,
                         const int32_t *rows, int batch, const float *depth, const float *img, const uint8_t *mask, int h, int w,
                         const float *const *kmat, const float *const *kinv, const float *pose, float d_thresh, int average_pts, int upscale,
                         float conf_thr, int t_max, void *workspace, void *stream) {
    if (nmaps < 0 || nmaps > kMaxMaps) return RPE_E_BADARG;
    if (nmaps == 0) return RPE_OK;
    if (!src || !n_bounds || !dst || !ticks || !rows || !depth || !img || !mask || !kmat || !kinv || !pose || !workspace || batch <= 0 ||
        h <= 0 || w <= 0 || (int64_t)h * w > INT32_MAX / 2)
        return RPE_E_BADARG;
    for (int k = 0; k < nmaps; ++k)
        if (!map_ok(&src[k]) || !map_ok(&dst[k]) || n_bounds[k] < 0 || n_bounds[k] > src[k].cap || rows[k] < 0 || rows[k] >= batch ||
            !kmat[k] || !kinv[k])
            return RPE_E_BADARG;
    if (!maps_disjoint(src, dst, nmaps)) return RPE_E_BADARG;
    if (upscale != 1) return RPE_E_UNSUPPORTED;
    const int64_t hw = (int64_t)h * w;
    Staging s;
    ManyHead &hd = s.head();
    hd.nmaps = nmaps;
    const size_t upd_at = s.add<FuseArgs>(nmaps), cmp_at = s.add<CompactArgs>(nmaps);
    FuseArgs *f = s.at<FuseArgs>(upd_at);
    CompactArgs *c = s.at<CompactArgs>(cmp_at);
    uint8_t *matched = (uint8_t *)workspace + kTableBytes;
    int *block_counts = (int *)(matched + align256((size_t)(nmaps * hw)));
    const float ccor = 1.0f / conf_thr;                              // torch.ones_like(depth) / conf_thr
    int64_t total_a = 0, total_b = 0;
    hd.off_a[0] = hd.off_b[0] = 0;
    for (int k = 0; k < nmaps; ++k) {
        const int64_t r = rows[k], nbd = n_bounds[k];
        total_a += ceil_div(nbd, kThreads);
        int nb;
        if (total_a > INT32_MAX / 2 || !compact_blocks(nbd + hw, total_b, nb)) return RPE_E_BADARG;
        hd.off_a[k + 1] = (int)total_a;
        hd.off_b[k + 1] = (int)total_b;
        hd.bound[k] = nbd;
        FuseArgs u = {};
        u.m = map_ptrs(&src[k]);
        u.depth = depth + r * hw; u.img = img + 3 * r * hw; u.mask = mask + r * hw; u.matched = matched + k * hw; u.h = h; u.w = w;
        u.kmat = kmat[k]; u.kinv = kinv[k]; u.pose = pose + 7 * r; u.d_thresh = d_thresh; u.ccor = ccor; u.average = average_pts;
        f[k] = u;
        CompactArgs a = {};
        a.src = map_ptrs(&src[k]); a.dst = map_ptrs(&dst[k]); a.n_bound = nbd;
        a.depth = u.depth; a.img = u.img; a.confidence = nullptr; a.mask = u.mask; a.matched = u.matched;
        a.h = h; a.w = w; a.kinv = kinv[k]; a.pose = u.pose; a.conf_thr = conf_thr; a.t_new = (float)ticks[k];
        a.prune = 1; a.tick = (float)(ticks[k] + 1); a.t_max = (float)t_max;          // :147 tick += 1, then :150-158
        a.block_counts = block_counts + hd.off_b[k];
        c[k] = a;
    }
    hipStream_t st = (hipStream_t)stream;
    if (put_table(s, workspace, st) != RPE_OK) return RPE_E_LAUNCH;
    if (hipMemsetAsync(matched, 0, (size_t)(nmaps * hw), st) != hipSuccess) return RPE_E_LAUNCH;
    if (total_a > 0)
        hipLaunchKernelGGL(k_fuse_update_many, dim3((int)total_a), dim3(kThreads), 0, st, (const ManyHead *)workspace,
                           (const FuseArgs *)((char *)workspace + upd_at));
    return compact_many(s, cmp_at, workspace, st);
}

int rpe_surfel_render_many(int nmaps, const rpe_surfel_map *maps, const int64_t *n_bounds, const float *kmat, const float *T,
                           int depth_transformed, int h, int w, float *img, float *depth, float *confidence, uint8_t *mask, void *workspace,
                           void *stream) {
    if (nmaps < 0 || nmaps > kMaxMaps) return RPE_E_BADARG;
    if (nmaps == 0) return RPE_OK;
    if (!maps || !n_bounds || !kmat || !T || !img || !depth || !confidence || !mask || !workspace || h < 3 || w < 3 ||
        (int64_t)h * w > INT32_MAX / 2)
        return RPE_E_BADARG;
    for (int k = 0; k < nmaps; ++k)
        if (!map_ok(&maps[k]) || n_bounds[k] < 0 || n_bounds[k] > maps[k].cap) return RPE_E_BADARG;
    const int64_t hw = (int64_t)h * w;
    Staging s;
    ManyHead &hd = s.head();
    hd.nmaps = nmaps;
    const size_t ren_at = s.add<RenderArgs>(nmaps);
    RenderArgs *r = s.at<RenderArgs>(ren_at);
    unsigned long long *keys = (unsigned long long *)((char *)workspace + kTableBytes);
    float gk[25];
    gauss_kernel(gk);
    int64_t total = 0;
    hd.off_a[0] = 0;
    for (int k = 0; k < nmaps; ++k) {
        total += ceil_div(n_bounds[k], kThreads);
        if (total > INT32_MAX / 2) return RPE_E_BADARG;
        hd.off_a[k + 1] = (int)total;
        RenderArgs a = {};
        a.m = map_ptrs(&maps[k]); a.n_bound = n_bounds[k]; a.kmat = kmat + 9 * k; a.T = T + 7 * k; a.depth_transformed = depth_transformed ? 1 : 0;
        a.h = h; a.w = w; a.keys = keys + k * hw;
        a.img = img + 3 * k * hw; a.depth = depth + k * hw; a.confidence = confidence + k * hw; a.mask = mask + k * hw;
        memcpy(a.gk, gk, sizeof(gk));
        r[k] = a;
    }
    hipStream_t st = (hipStream_t)stream;
    if (put_table(s, workspace, st) != RPE_OK) return RPE_E_LAUNCH;
    if (hipMemsetAsync(keys, 0, (size_t)(nmaps * hw) * sizeof(unsigned long long), st) != hipSuccess) return RPE_E_LAUNCH;
    const RenderArgs *rd = (const RenderArgs *)((char *)workspace + ren_at);
    if (total > 0) hipLaunchKernelGGL(k_render_splat_many, dim3((int)total), dim3(kThreads), 0, st, (const ManyHead *)workspace, rd);
    hipLaunchKernelGGL(k_render_resolve_many, dim3(ceil_div(hw, kThreads), nmaps), dim3(kThreads), 0, st, rd);
    return rpe_check_launch();
}

}  // extern "C"
