// Beam search on gfx950 (include/afhip.h): candidate selection over nb x V continuations per prompt (afhip_beam_select) and the
// KV-cache slot gather that reorders the beams between steps (afhip_kv_gather).
//
// afhip_beam_select, three launches over 8192-id chunks (one workgroup per chunk and row, like sample_filter.hip):
//   1. bs_stats: the chunk's maximum and sum exp(x - chunk max);
//   2. bs_chunk: every workgroup combines its row's chunk statistics in chunk order (so every workgroup of a row holds the same
//      m_r, log s_r), forms logp = (x - m_r) - log s_r and cand = logp + running[r] in f32 as torch does (no contraction), writes
//      logp when asked, and keeps the chunk's own top K of cand;
//   3. bs_merge: one workgroup per prompt selects the K largest of the nb x n_chunks x K survivors and sorts them.
// Candidates travel as 64-bit keys (order-preserving bits of cand << 32 | ~flat index): unique per prompt, larger key = earlier in
// the stated order (value descending, smaller flat index first), so "top K" is a plain radix select with no tie rule of its own.
// Selection is on cand itself: rounding in the add can make different logits equal, which a top K of the logits would miss.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int BS_THREADS = 256;
constexpr int BS_PER_THREAD = 32;
constexpr int BS_CHUNK = BS_THREADS * BS_PER_THREAD;
constexpr int BS_MAX_K = 128;
constexpr int BS_MAX_NB = 32;
constexpr int BS_MAX_V = 1 << 23;                  // nb * V < 2^28: the flat index fits the low 32 bits of a key

struct BP {
    const float* logits;
    const float* running;
    int R, nb, V, ld, nc, K;
    float* cmax;            // [R, nc] chunk maximum
    float* csum;            // [R, nc] sum exp(x - chunk maximum)
    u64* cand;              // [B, nb, nc, K] each chunk's top K keys (0 = empty slot)
    float* values;
    int64_t* indices;
    float* scores;
    int lds;
};

__device__ __forceinline__ uint32_t fkey(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float kval(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <bool RB>
__device__ __forceinline__ float model_round(float x) {
    if (RB) return (float)(bf16)x;
    return x;
}

// the chunk's values (strided: id c * 8192 + it * 256 + tid), -inf past V
template <bool RB>
__device__ __forceinline__ void load_chunk(const BP& p, int r, int c, float (&x)[BS_PER_THREAD]) {
    const float* row = p.logits + (long long)r * p.ld;
#pragma unroll
    for (int it = 0; it < BS_PER_THREAD; ++it) {
        const int i = c * BS_CHUNK + it * BS_THREADS + threadIdx.x;
        x[it] = i < p.V ? model_round<RB>(row[i]) : -INFINITY;
    }
}

// block-wide reductions in a fixed order (lane tree, then the four waves in order): deterministic for a given chunk
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float out = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return out;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float out = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return out;
}

// The need-th largest key among those `visit` hands out (keys unique, 1 <= need <= their count): radix select over 8-bit digits, one
// LDS histogram per digit.  Every thread of the block calls it and gets the same key.
template <class Visit>
__device__ u64 block_kth_largest(Visit visit, uint32_t need) {
    __shared__ uint32_t suf[256];
    __shared__ u64 s_prefix;
    __shared__ uint32_t s_need;
    const int tid = threadIdx.x;
    u64 prefix = 0;
    for (int d = 0; d < 8; ++d) {
        const int sh = 56 - 8 * d;
        suf[tid] = 0u;
        __syncthreads();
        visit([&](u64 key) {
            if (d == 0 || (key >> (sh + 8)) == prefix) atomicAdd(&suf[(key >> sh) & 255u], 1u);
        });
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                  // suffix sums: suf[q] = keys of the bucket with digit >= q
            const uint32_t add = tid + o < 256 ? suf[tid + o] : 0u;
            __syncthreads();
            suf[tid] += add;
            __syncthreads();
        }
        const uint32_t here = suf[tid], next = tid < 255 ? suf[tid + 1] : 0u;
        if (here >= need && next < need) {
            s_prefix = (prefix << 8) | (u64)tid;
            s_need = need - next;
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
        __syncthreads();
    }
    return prefix;
}

// ---- 1: chunk maximum and sum exp(x - chunk maximum)
template <bool RB>
__global__ __launch_bounds__(BS_THREADS) void bs_stats(BP p) {
    __shared__ float red[4];
    const int c = blockIdx.x, r = blockIdx.y;
    float x[BS_PER_THREAD];
    load_chunk<RB>(p, r, c, x);
    float m = -INFINITY;
#pragma unroll
    for (int it = 0; it < BS_PER_THREAD; ++it) m = fmaxf(m, x[it]);
    m = block_max(m, red);
    float s = 0.f;
    if (m > -INFINITY) {
#pragma unroll
        for (int it = 0; it < BS_PER_THREAD; ++it) s += expf(x[it] - m);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        p.cmax[(long long)r * p.nc + c] = m;
        p.csum[(long long)r * p.nc + c] = s;
    }
}

// ---- 2: log-probs, cand, and the chunk's top K keys
template <bool RB>
__global__ __launch_bounds__(BS_THREADS) void bs_chunk(BP p) {
#pragma clang fp contract(off)
    __shared__ uint32_t s_slot;
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    float x[BS_PER_THREAD];
    load_chunk<RB>(p, r, c, x);
    // the row's statistics, combined in chunk order by every thread (the same floats in every workgroup of the row)
    const float* cm = p.cmax + (long long)r * p.nc;
    const float* cs = p.csum + (long long)r * p.nc;
    float m = -INFINITY;
    for (int j = 0; j < p.nc; ++j) m = fmaxf(m, cm[j]);
    float s = 0.f;
    for (int j = 0; j < p.nc; ++j)
        if (cm[j] > -INFINITY) s += cs[j] * expf(cm[j] - m);
    const float ls = logf(s);
    const float run = p.running[r];
    const uint32_t flat0 = (uint32_t)(r % p.nb) * (uint32_t)p.V;
    float* out = p.scores ? p.scores + (long long)r * p.lds : nullptr;
    u64 key[BS_PER_THREAD];
#pragma unroll
    for (int it = 0; it < BS_PER_THREAD; ++it) {
        const int i = c * BS_CHUNK + it * BS_THREADS + tid;
        const float lp = (x[it] - m) - ls;
        const float cv = lp + run;
        if (out && i < p.V) out[i] = lp;
        key[it] = i < p.V ? ((u64)fkey(cv) << 32) | (u64)(~(flat0 + (uint32_t)i)) : 0ull;
    }
    const int valid = min(BS_CHUNK, p.V - c * BS_CHUNK);
    const int keep = min(p.K, valid);
    const u64 t = block_kth_largest([&](auto f) {
#pragma unroll
        for (int it = 0; it < BS_PER_THREAD; ++it) f(key[it]);
    }, (uint32_t)keep);
    if (tid == 0) s_slot = 0u;
    __syncthreads();
    // exactly `keep` keys are >= t; their order in the slab does not matter (the merge selects and sorts by key)
    u64* slab = p.cand + ((long long)r * p.nc + c) * p.K;
#pragma unroll
    for (int it = 0; it < BS_PER_THREAD; ++it)
        if (key[it] != 0ull && key[it] >= t) {
            const uint32_t q = atomicAdd(&s_slot, 1u);
            if (q < (uint32_t)keep) slab[q] = key[it];
        }
    for (int j = keep + tid; j < p.K; j += BS_THREADS) slab[j] = 0ull;
}

// ---- 3: per prompt, the K largest keys of its nb x nc slabs, sorted
__global__ __launch_bounds__(BS_THREADS) void bs_merge(BP p) {
    __shared__ u64 sel[BS_MAX_K];
    __shared__ uint32_t s_slot;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = p.nb * p.nc * p.K;
    const u64* src = p.cand + (long long)b * n;
    const u64 t = block_kth_largest([&](auto f) {
        for (int i = tid; i < n; i += BS_THREADS) f(src[i]);
    }, (uint32_t)p.K);
    if (tid == 0) s_slot = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += BS_THREADS) {
        const u64 k = src[i];
        if (k != 0ull && k >= t) {
            const uint32_t q = atomicAdd(&s_slot, 1u);
            if (q < (uint32_t)p.K) sel[q] = k;
        }
    }
    __syncthreads();
    if (tid < p.K) {
        const u64 k = sel[tid];
        int rank = 0;
        for (int j = 0; j < p.K; ++j) rank += sel[j] > k;
        p.values[(long long)b * p.K + rank] = kval((uint32_t)(k >> 32));
        p.indices[(long long)b * p.K + rank] = (int64_t)(uint32_t)~(uint32_t)k;
    }
}

struct BsLayout {
    size_t cmax, csum, cand, total;
    int nc;
};

BsLayout bs_layout(int B, int nb, int V, int K) {
    BsLayout l;
    l.nc = cdiv(V, BS_CHUNK);
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += (b + 255) / 256 * 256; return at; };
    const size_t R = (size_t)B * nb, NC = (size_t)l.nc;
    l.cmax = take(R * NC * 4);
    l.csum = take(R * NC * 4);
    l.cand = take(R * NC * (size_t)K * 8);
    l.total = o;
    return l;
}

// ---- afhip_kv_gather: one thread per 16 bytes of a row, KVG_UNITS of them per thread
constexpr int KVG_THREADS = 256;
constexpr int KVG_UNITS = 4;

struct KP {
    const char* sk; const char* sv;
    char* dk; char* dv;
    char* ws;
    const int32_t* parent; const int32_t* row0; const int32_t* row1;
    int nkv, cap, Bs, Bd, U, max_rows, in_place;
};

// is slot q of the (in-place) cache overwritten by this call?
__device__ __forceinline__ bool overwritten(const KP& p, int q) {
    const int pq = p.parent[q];
    return pq != q && pq >= 0 && pq < p.Bs;
}

// STAGE: in place, copy the rows of every slot whose parent is itself overwritten into the workspace (keyed by the READING slot).
// !STAGE: write every moved slot, from the workspace when it was staged, else straight from src.
template <bool STAGE>
__global__ __launch_bounds__(KVG_THREADS) void kvg_copy(KP p) {
    const int r = blockIdx.z, lh = blockIdx.y >> 1, kv = blockIdx.y & 1, tid = threadIdx.x;
    const int par = p.parent[r];
    if (par < 0 || par >= p.Bs) return;
    if (p.in_place && par == r) return;                       // its own parent: nothing to do
    const bool staged = p.in_place && overwritten(p, par);
    if (STAGE && !staged) return;
    const int t0 = max(p.row0[r], 0);
    const int t1 = min(min(p.row1[r], p.cap), t0 + p.max_rows);
    const int n = (t1 - t0) * p.U;                            // 16-byte units of the range
    const int l = lh / p.nkv, h = lh - l * p.nkv;
    const long long rowsz = (long long)p.U;                   // in uint4
    const long long src_row0 = (((long long)l * p.Bs + par) * p.nkv + h) * p.cap + t0;
    const long long dst_row0 = (((long long)l * p.Bd + r) * p.nkv + h) * p.cap + t0;
    const long long ws_row0 = (((long long)l * p.Bd + r) * p.nkv + h) * p.max_rows;         // workspace [2][n_layers][Bd][nkv][max_rows]
    const long long ws_kv = (long long)(gridDim.y >> 1) * p.Bd * p.max_rows * rowsz;   // one of K / V in the workspace
    const uint4* ws_in = (const uint4*)p.ws + kv * ws_kv + ws_row0 * rowsz;
    const uint4* from;
    uint4* to;
    if (STAGE) {
        from = (const uint4*)(kv ? p.sv : p.sk) + src_row0 * rowsz;
        to = (uint4*)p.ws + kv * ws_kv + ws_row0 * rowsz;
    } else {
        from = staged ? ws_in : (const uint4*)(kv ? p.sv : p.sk) + src_row0 * rowsz;
        to = (uint4*)(kv ? p.dv : p.dk) + dst_row0 * rowsz;
    }
    const int e0 = blockIdx.x * KVG_THREADS * KVG_UNITS + tid;
    uint4 v[KVG_UNITS];
#pragma unroll
    for (int u = 0; u < KVG_UNITS; ++u) {
        const int e = e0 + u * KVG_THREADS;
        if (e < n) v[u] = from[e];
    }
#pragma unroll
    for (int u = 0; u < KVG_UNITS; ++u) {
        const int e = e0 + u * KVG_THREADS;
        if (e < n) to[e] = v[u];
    }
}

}  // namespace

extern "C" size_t afhip_beam_select_workspace_bytes(int B, int nb, int V, int K) {
    if (B <= 0 || nb <= 0 || nb > BS_MAX_NB || V <= 0 || V >= BS_MAX_V || K <= 0 || K > BS_MAX_K) return 0;
    return bs_layout(B, nb, V, K).total;
}

extern "C" int afhip_beam_select(const afhip_beam_select_args* a, void* ws, size_t ws_bytes, void* stream) {
    AFHIP_CHECK(a != nullptr, "afhip_beam_select: null args");
    AFHIP_CHECK(a->logits != nullptr && a->running != nullptr, "afhip_beam_select: null logits or running");
    AFHIP_CHECK(a->values != nullptr && a->indices != nullptr, "afhip_beam_select: null values or indices");
    AFHIP_CHECK(a->nb >= 1 && a->nb <= BS_MAX_NB, "afhip_beam_select: nb=%d must be in [1,%d]", a->nb, BS_MAX_NB);
    AFHIP_CHECK(a->B >= 1 && (long long)a->B * a->nb <= 65535, "afhip_beam_select: bad shape B=%d (B * nb <= 65535)", a->B);
    AFHIP_CHECK(a->V > 0 && a->V < BS_MAX_V && a->ld >= a->V, "afhip_beam_select: bad shape V=%d ld=%d (0 < V < 2^23, ld >= V)", a->V, a->ld);
    AFHIP_CHECK(a->K >= 1 && a->K <= BS_MAX_K && (long long)a->K <= (long long)a->nb * a->V, "afhip_beam_select: K=%d must be in [1,%d] and <= nb * V",
                a->K, BS_MAX_K);
    AFHIP_CHECK(a->model_dtype == AFHIP_F32 || a->model_dtype == AFHIP_BF16, "afhip_beam_select: bad model_dtype");
    AFHIP_CHECK(a->scores == nullptr || a->ld_scores >= a->V, "afhip_beam_select: ld_scores=%d < V", a->ld_scores);
    const BsLayout l = bs_layout(a->B, a->nb, a->V, a->K);
    AFHIP_CHECK(ws != nullptr && ((uintptr_t)ws & 255u) == 0, "afhip_beam_select: workspace must be non-null and 256-byte aligned");
    AFHIP_CHECK(ws_bytes >= l.total, "afhip_beam_select: workspace %zu bytes < %zu (afhip_beam_select_workspace_bytes)", ws_bytes, l.total);
    char* w = (char*)ws;
    BP p;
    p.logits = a->logits; p.running = a->running;
    p.R = a->B * a->nb; p.nb = a->nb; p.V = a->V; p.ld = a->ld; p.nc = l.nc; p.K = a->K;
    p.cmax = (float*)(w + l.cmax); p.csum = (float*)(w + l.csum); p.cand = (u64*)(w + l.cand);
    p.values = a->values; p.indices = a->indices; p.scores = a->scores; p.lds = a->ld_scores;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(l.nc, p.R), blk(BS_THREADS);
    if (a->model_dtype == AFHIP_BF16) {
        hipLaunchKernelGGL(bs_stats<true>, grid, blk, 0, s, p);
        hipLaunchKernelGGL(bs_chunk<true>, grid, blk, 0, s, p);
    } else {
        hipLaunchKernelGGL(bs_stats<false>, grid, blk, 0, s, p);
        hipLaunchKernelGGL(bs_chunk<false>, grid, blk, 0, s, p);
    }
    hipLaunchKernelGGL(bs_merge, dim3(a->B), blk, 0, s, p);
    AFHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t afhip_kv_gather_workspace_bytes(int n_layers, int B, int n_kv, int hd, int max_rows, int dtype) {
    if (n_layers <= 0 || B <= 0 || n_kv <= 0 || hd <= 0 || max_rows < 0 || (dtype != AFHIP_F32 && dtype != AFHIP_BF16)) return 0;
    return 2ull * n_layers * B * n_kv * (size_t)max_rows * hd * dtype_size(dtype);
}

extern "C" int afhip_kv_gather(const afhip_kv_cache* src, const afhip_kv_cache* dst, int n_layers, int n_kv, int hd, int dtype,
                               const int32_t* parent, const int32_t* row0, const int32_t* row1, int max_rows, void* ws, size_t ws_bytes,
                               void* stream) {
    AFHIP_CHECK(src != nullptr && dst != nullptr, "afhip_kv_gather: null cache");
    AFHIP_CHECK(src->k && src->v && dst->k && dst->v, "afhip_kv_gather: null cache tensor");
    AFHIP_CHECK(parent && row0 && row1, "afhip_kv_gather: null parent / row0 / row1");
    AFHIP_CHECK(dtype == AFHIP_F32 || dtype == AFHIP_BF16, "afhip_kv_gather: bad dtype");
    AFHIP_CHECK(n_layers > 0 && n_kv > 0 && hd > 0 && (long long)n_layers * n_kv * 2 <= 65535, "afhip_kv_gather: bad shape n_layers=%d n_kv=%d hd=%d",
                n_layers, n_kv, hd);
    AFHIP_CHECK(hd * dtype_size(dtype) % 16 == 0, "afhip_kv_gather: hd * element size must be a multiple of 16 bytes");
    AFHIP_CHECK(src->cap == dst->cap && src->cap > 0, "afhip_kv_gather: caches differ in cap (%d vs %d)", src->cap, dst->cap);
    AFHIP_CHECK(src->B > 0 && dst->B > 0 && dst->B <= 65535, "afhip_kv_gather: bad B (src %d, dst %d)", src->B, dst->B);
    AFHIP_CHECK(max_rows >= 0, "afhip_kv_gather: max_rows < 0");
    const bool in_place = src->k == dst->k;
    AFHIP_CHECK((src->v == dst->v) == in_place, "afhip_kv_gather: k and v must both be in place or both out of place");
    AFHIP_CHECK(!in_place || src->B == dst->B, "afhip_kv_gather: an in-place gather needs src->B == dst->B");
    const int U = hd * (int)dtype_size(dtype) / 16;
    AFHIP_CHECK((long long)max_rows * U < (1ll << 31), "afhip_kv_gather: max_rows=%d too large", max_rows);
    const size_t need = in_place ? afhip_kv_gather_workspace_bytes(n_layers, dst->B, n_kv, hd, max_rows, dtype) : 0;
    AFHIP_CHECK(need == 0 || (ws != nullptr && ((uintptr_t)ws & 15u) == 0), "afhip_kv_gather: in place needs a 16-byte aligned workspace");
    AFHIP_CHECK(ws_bytes >= need, "afhip_kv_gather: workspace %zu bytes < %zu (afhip_kv_gather_workspace_bytes)", ws_bytes, need);
    if (max_rows == 0) return 0;
    KP p;
    p.sk = (const char*)src->k; p.sv = (const char*)src->v; p.dk = (char*)dst->k; p.dv = (char*)dst->v; p.ws = (char*)ws;
    p.parent = parent; p.row0 = row0; p.row1 = row1;
    p.nkv = n_kv; p.cap = src->cap; p.Bs = src->B; p.Bd = dst->B; p.U = U; p.max_rows = max_rows; p.in_place = in_place;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(max_rows * U, KVG_THREADS * KVG_UNITS), n_layers * n_kv * 2, dst->B), blk(KVG_THREADS);
    if (in_place) hipLaunchKernelGGL(kvg_copy<true>, grid, blk, 0, s, p);
    hipLaunchKernelGGL(kvg_copy<false>, grid, blk, 0, s, p);
    AFHIP_LAUNCH_CHECK();
    return 0;
}
