// The training step's update on the device: gradient clipping by the global norm and AdamW, two launches for any number of tensors.
//
// Both kernels walk a device-resident table, one rpe_optim_row {param, grad, exp_avg, exp_avg_sq, numel} per tensor, through a chunk list
// {row, offset} that the host builds with rpe_optim_chunk_offsets: every tensor is cut into pieces of RPE_OPTIM_CHUNK elements (the last
// one shorter), one workgroup per piece.  The split depends on the tensor sizes alone, so the sums below group alike on every device.
//
//   k_grad_norm   one f64 partial sum of squares (a product of two floats is exact in f64) and one count of non-finite elements per chunk;
//                 the workgroup that draws the last ticket adds the partials IN INDEX ORDER in f64 and writes the record {norm f64, norm f32,
//                 non-finite count}.  No float atomics: which workgroup is last changes who adds, never the order, so the record is
//                 bit-identical from run to run.
//   k_adamw       reads the record; with a non-finite gradient (and skip_nonfinite) it touches no parameter, no moment and not the step
//                 counter and counts the step as skipped; otherwise torch.optim.AdamW's arithmetic (amsgrad = False, maximize = False) on
//                 c * g, c = min(1, max_norm / (norm + 1e-6)) being torch.nn.utils.clip_grad_norm_'s coefficient.  The gradients are read only.
//
// The partials cross workgroups inside the launch, possibly between XCDs whose L2s are not coherent: device-scope stores (written
// through), every storing wave's vmcnt(0), the barrier, then one device-scope ticket per workgroup; the last workgroup reads them with
// device-scope loads -- the hand-off of pose.hip's reduce tail.  Nothing waits on another workgroup, so nothing here can spin.
//
// Pointers need 4-byte alignment only.  Where a chunk's pointers share their phase within 16 bytes, the elements in front of the first
// 16-byte boundary and behind the last go one by one and the rest as float4; where they do not (a parameter view beside moments
// allocated elsewhere), the whole chunk goes one by one -- one dword per lane is still a coalesced access.
// The file is built with -ffp-contract=off and names its fused multiply-adds: the update takes the roundings of torch.optim.AdamW's GPU
// kernels, so that a model stepped here and one stepped there from the same gradients hold the same weights, bit for bit.
#include "rpe_common.h"

#define OPT_CHUNK RPE_OPTIM_CHUNK
#define OPT_THREADS 256
#define OPT_WAIT_VMCNT0 0x0f70            // s_waitcnt simm16 (gfx9 family): vmcnt = 0, expcnt and lgkmcnt left free (pose.hip's RPE_WAIT_VMCNT0)
#define OPT_HEAD_BYTES 16                 // the workspace's head: the two tickets, padded

static_assert(sizeof(rpe_optim_row) == 40 && sizeof(rpe_optim_chunk) == 8 && sizeof(rpe_optim_record) == 32, "rpe.h layouts");

__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// elements of a chunk in front of the first 16-byte boundary of ``p`` (at most 3, at most ``len``)
__device__ __forceinline__ int head_len(const void* p, int len) {
    const int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return h < len ? h : len;
}

// one ticket per workgroup, after every wave's stores have been acknowledged: true in the workgroup that drew the last one
__device__ __forceinline__ bool last_workgroup(unsigned* ticket, int n_blocks, bool* flag) {
    __builtin_amdgcn_s_waitcnt(OPT_WAIT_VMCNT0);
    __syncthreads();
    if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(n_blocks - 1);
    __syncthreads();
    return *flag;
}

__global__ __launch_bounds__(OPT_THREADS) void k_grad_norm(const rpe_optim_row* table, const rpe_optim_chunk* chunks, int n_chunks, unsigned* ticket,
                                                           double* partial, int* nonfin, rpe_optim_record* rec) {
    __shared__ double red[OPT_THREADS];
    __shared__ int redn[OPT_THREADS];
    __shared__ bool is_last;
    const int tid = threadIdx.x;
    const rpe_optim_chunk ck = chunks[blockIdx.x];
    const rpe_optim_row row = table[ck.row];
    const long long left = row.numel - (long long)ck.offset;
    const int len = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    const float* g = row.grad + ck.offset;
    const int head = head_len(g, len), quads = (len - head) >> 2, tail0 = head + 4 * quads;
    double s = 0.0;
    int bad = 0;
    auto take = [&](float v) { s += (double)v * (double)v; bad += non_finite(v) ? 1 : 0; };
    if (tid < head) take(g[tid]);
    const float4* g4 = (const float4*)(g + head);
    for (int q = tid; q < quads; q += OPT_THREADS) {
        const float4 v = g4[q];
        take(v.x); take(v.y); take(v.z); take(v.w);
    }
    if (tail0 + tid < len) take(g[tail0 + tid]);
    s = wave_sum(s);
    bad = wave_sum(bad);
    if ((tid & 63) == 0) { red[tid >> 6] = s; redn[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(partial + blockIdx.x, ((red[0] + red[1]) + red[2]) + red[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(nonfin + blockIdx.x, (redn[0] + redn[1]) + (redn[2] + redn[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_workgroup(ticket, n_chunks, &is_last)) return;
    if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // for the next call
    double total = 0.0;                                                                              // (thread 0's)
    long long count = 0;
    for (int base = 0; base < n_chunks; base += OPT_THREADS) {
        const int n = n_chunks - base < OPT_THREADS ? n_chunks - base : OPT_THREADS;
        __syncthreads();
        if (tid < n) {
            red[tid] = __hip_atomic_load(partial + base + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            redn[tid] = __hip_atomic_load(nonfin + base + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < n; ++i) { total += red[i]; count += redn[i]; }                       // index order
    }
    if (tid == 0) {
        const double norm = sqrt(total);
        rec->norm = norm;
        rec->norm_f32 = (float)norm;
        rec->reserved = 0;
        rec->nonfinite = count;
        rec->reserved2 = 0;
    }
}

struct AdamScalars { float decay, w1, b2, w2, bc2_sqrt, eps, neg_step, clip; int go; };

__global__ __launch_bounds__(OPT_THREADS) void k_adamw(const rpe_optim_row* table, const rpe_optim_chunk* chunks, int n_chunks, unsigned* ticket,
                                                       const rpe_optim_record* rec, long long* state, double lr, double beta1, double beta2, double eps,
                                                       double weight_decay, double max_norm, int skip_nonfinite) {
    __shared__ AdamScalars sh;
    __shared__ bool is_last;
    const int tid = threadIdx.x;
    if (tid == 0) {
        // state[0] (the step counter) is written by the LAST workgroup of a launch only, after every workgroup has read it here
        const long long step = state[0] + 1;
        const double norm = rec->norm;
        sh.go = !(skip_nonfinite && rec->nonfinite != 0);
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        double c = 1.0;
        if (max_norm > 0.0) { c = max_norm / (norm + 1e-6); if (c > 1.0) c = 1.0; }                   // (a NaN norm stays NaN, as in torch)
        sh.clip = (float)c;
        sh.decay = (float)(1.0 - lr * weight_decay);
        sh.w1 = (float)(1.0 - beta1); sh.b2 = (float)beta2; sh.w2 = (float)(1.0 - beta2);
        sh.bc2_sqrt = (float)sqrt(bc2); sh.eps = (float)eps; sh.neg_step = (float)(-(lr / bc1));
    }
    __syncthreads();
    const AdamScalars A = sh;
    if (A.go) {
        const rpe_optim_chunk ck = chunks[blockIdx.x];
        const rpe_optim_row row = table[ck.row];
        const long long left = row.numel - (long long)ck.offset;
        const int len = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
        float* p = row.param + ck.offset;
        const float* g = row.grad + ck.offset;
        float* m = row.exp_avg + ck.offset;
        float* v = row.exp_avg_sq + ck.offset;
        auto update = [&](float& pp, float gg, float& mm, float& vv) {
            gg = A.clip * gg;                                             // clip_grad_norm_: grad.mul_(coefficient), also when it is 1
            // torch.optim.AdamW's roundings on the GPU (its default, multi-tensor route), one operation at a time: the three
            // accumulations are fused multiply-adds there, the products and the quotient in front of them round on their own
            pp = pp * A.decay;                                            // param.mul_(1 - lr * weight_decay)
            mm = __builtin_fmaf(A.w1, gg - mm, mm);                       // exp_avg.lerp_(grad, 1 - beta1)
            vv = __builtin_fmaf(A.w2, gg * gg, vv * A.b2);                // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
            const float denom = sqrtf(vv) / A.bc2_sqrt + A.eps;           // (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)
            pp = __builtin_fmaf(A.neg_step, mm / denom, pp);              // param.addcdiv_(exp_avg, denom, value = -lr / bc1)
        };
        const unsigned phase = (unsigned)(((uintptr_t)p ^ (uintptr_t)g) | ((uintptr_t)p ^ (uintptr_t)m) | ((uintptr_t)p ^ (uintptr_t)v)) & 15u;
        const int head = phase == 0 ? head_len(p, len) : len;
        const int quads = (len - head) >> 2, tail0 = head + 4 * quads;
        for (int i = tid; i < head; i += OPT_THREADS) update(p[i], g[i], m[i], v[i]);
        float4* p4 = (float4*)(p + head);
        const float4* g4 = (const float4*)(g + head);
        float4* m4 = (float4*)(m + head);
        float4* v4 = (float4*)(v + head);
        for (int q = tid; q < quads; q += OPT_THREADS) {
            float4 pq = p4[q], mq = m4[q], vq = v4[q];
            const float4 gq = g4[q];
            update(pq.x, gq.x, mq.x, vq.x); update(pq.y, gq.y, mq.y, vq.y); update(pq.z, gq.z, mq.z, vq.z); update(pq.w, gq.w, mq.w, vq.w);
            p4[q] = pq; m4[q] = mq; v4[q] = vq;
        }
        if (tail0 + tid < len) update(p[tail0 + tid], g[tail0 + tid], m[tail0 + tid], v[tail0 + tid]);
    }
    if (!last_workgroup(ticket, n_chunks, &is_last)) return;
    if (tid == 0) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        state[A.go ? 0 : 1] += 1;                                         // the step counter, or the count of skipped steps
    }
}

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" size_t rpe_optim_chunk_floats(void) { return OPT_CHUNK; }

extern "C" size_t rpe_optim_workspace_bytes(int n_chunks) {
    if (n_chunks <= 0) return 0;
    return ((OPT_HEAD_BYTES + (size_t)n_chunks * 4 + 15) / 16 * 16 + (size_t)n_chunks * 8 + 15) / 16 * 16;      // tickets | counts | partials
}

extern "C" int rpe_optim_chunk_offsets(const long long* numel, int n_rows, rpe_optim_chunk* out, int cap) {
    if (n_rows < 0 || (n_rows > 0 && !numel) || cap < 0) return RPE_E_BADARG;
    long long total = 0;
    for (int r = 0; r < n_rows; ++r) {
        if (numel[r] < 1) return RPE_E_BADARG;
        if (numel[r] >= (1LL << 31)) return RPE_E_UNSUPPORTED;          // element offsets are 32 bits
        total += (numel[r] + OPT_CHUNK - 1) / OPT_CHUNK;
        if (total > 0x7fffffffLL) return RPE_E_UNSUPPORTED;
    }
    if (!out) return (int)total;
    if ((long long)cap < total) return RPE_E_BADARG;
    int at = 0;
    for (int r = 0; r < n_rows; ++r)
        for (long long off = 0; off < numel[r]; off += OPT_CHUNK) out[at++] = rpe_optim_chunk{r, (int)off};
    return (int)total;
}

static int check_common(const rpe_optim_row* table, int n_rows, const rpe_optim_chunk* chunks, int n_chunks, void* workspace, const void* record) {
    if (n_rows < 0 || n_chunks < 0) return RPE_E_BADARG;
    if (!table || !chunks || !workspace || !record) return RPE_E_BADARG;
    if (misaligned(table, 8) || misaligned(chunks, 4) || misaligned(workspace, 16) || misaligned(record, 8)) return RPE_E_BADARG;
    if (n_chunks < n_rows) return RPE_E_BADARG;                         // every row has at least one chunk
    return RPE_OK;
}

extern "C" int rpe_grad_norm(const rpe_optim_row* table, int n_rows, const rpe_optim_chunk* chunks, int n_chunks, void* workspace,
                             rpe_optim_record* record, void* stream) {
    const int st = check_common(table, n_rows, chunks, n_chunks, workspace, record);
    if (st != RPE_OK) return st;
    if (n_rows == 0 || n_chunks == 0) return RPE_OK;
    unsigned* ticket = (unsigned*)workspace;
    int* nonfin = (int*)((char*)workspace + OPT_HEAD_BYTES);
    double* partial = (double*)((char*)workspace + (OPT_HEAD_BYTES + (size_t)n_chunks * 4 + 15) / 16 * 16);
    hipLaunchKernelGGL(k_grad_norm, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, chunks, n_chunks, ticket, partial, nonfin, record);
    return rpe_check_launch();
}

extern "C" int rpe_adamw_step(const rpe_optim_row* table, int n_rows, const rpe_optim_chunk* chunks, int n_chunks, void* workspace,
                              const rpe_optim_record* record, long long* state, double lr, double beta1, double beta2, double eps,
                              double weight_decay, double max_norm, int skip_nonfinite, void* stream) {
    const int st = check_common(table, n_rows, chunks, n_chunks, workspace, record);
    if (st != RPE_OK) return st;
    if (!state || misaligned(state, 8)) return RPE_E_BADARG;
    if (n_rows == 0 || n_chunks == 0) return RPE_OK;
    hipLaunchKernelGGL(k_adamw, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, chunks, n_chunks, (unsigned*)workspace + 1, record,
                       state, lr, beta1, beta2, eps, weight_decay, max_norm, skip_nonfinite);
    return rpe_check_launch();
}
