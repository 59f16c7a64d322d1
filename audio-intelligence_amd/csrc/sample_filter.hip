// Full-vocabulary filter-and-draw on gfx950 (afhip_sample_filter, include/afhip.h): guidance mix + allowed intervals, repetition
// penalty, temperature, top-k (HF ties-kept or exact), top-p and an inverse-CDF draw in ascending id order, for rows of up to 2^23 ids.
//
// Every row is split into 8192-id chunks, one workgroup each, so B = 8 rows of a 152 064-id vocabulary already fill 152 workgroups.
// The k-th value and the top-p boundary are found by a radix select on order-preserving uint32 keys of the processed f32 values:
// four 8-bit digits for top-k (count histograms), four more for top-p (histograms of exp(x - rowmax) mass, restricted to the top-k
// survivors).  Each step is one launch over the chunks: a chunk's histogram goes to its own slab, and every workgroup of the NEXT
// launch sums the slabs of its row (a few KB) and finds the bucket itself -- no cross-workgroup protocol, the kernel boundary orders it.
// Masses are exp(x - rowmax) * 2^40 truncated to integers and summed as integers, so the sums (the top-p boundary, the CDF) do not
// depend on the order of summation: the results are bit-identical for any grid, placement or launch.
#include "sample_mix.h"
#include <limits.h>

namespace {

typedef unsigned long long u64;
constexpr int SF_THREADS = 256;
constexpr int SF_PER_THREAD = 32;
constexpr int SF_CHUNK = SF_THREADS * SF_PER_THREAD;
constexpr int SF_BINS = 256;
constexpr int SF_MAX_IV = 64;
constexpr int SF_MAX_PEN_V = 262144;               // penalty bitmap of a row in 32 KB of LDS
constexpr int SF_MAX_V = 1 << 23;                  // V * 2^40 < 2^64
constexpr int SF_STEPS = 8;                        // 4 top-k digits + 4 top-p digits
constexpr float SF_FX = 1099511627776.f;           // 2^40

struct RowState {
    uint32_t prefix;        // key digits fixed so far by the current search
    uint32_t cnt_above;     // top-k: ids whose key lies above the current bucket
    u64 mass_above;         // top-p: surviving mass above the current bucket
    u64 target;             // top-p: ceil(p * Z), Z = mass of the top-k survivors
    uint32_t tk;            // top-k threshold key (0 = top-k off)
    uint32_t tie_keep;      // ids with key == tk that survive top-k
    uint32_t tp;            // top-p threshold key
    uint32_t tp_off;        // top-p not applied (off, or a row with no mass)
};

struct FP {
    const float* logits;
    const float* cfg_logits;
    float cfg, omc;
    int rows, V, ld, nc, vp, bmw;
    const int32_t* allowed;
    int n_iv;
    const int32_t* pen_ids;
    const int32_t* n_ids;
    int max_ids;
    float pen, T;
    int kmode;              // 0 off, 1 HF (ties kept), 2 exact
    int k;
    float p;
    int nk, np;             // top-k / top-p radix steps (0 or 4 each)
    float* xs;              // [rows, vp] processed values
    float* cmax;            // [rows, nc] chunk maximum
    int* carg;              // [rows, nc] its first id
    uint32_t* cnt;          // [4][rows][nc][256]
    u64* mass;              // [4][rows][nc][256]
    RowState* st;           // [rows][SF_STEPS]
    u64* kmass;             // [rows][nc] surviving mass of each chunk
    uint32_t* bm;           // [rows][bmw] penalty bitmap or null
    const float* u;
    float* scores;
    int lds;
    int64_t* token;
};

__device__ __forceinline__ uint32_t fkey(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float kval(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// exp(x - m) in 2^-40 units; m is the row maximum, so the mass of one id is at most 2^40
__device__ __forceinline__ u64 fxm(float x, float m) {
    if (!(x > -INFINITY)) return 0ull;
    if (x >= m) return (u64)SF_FX;
    return (u64)(expf(x - m) * SF_FX);
}

// (v, i) beats (w, j) for the first-index maximum
__device__ __forceinline__ bool amax_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__device__ float row_max(const FP& p, int r) {
    float m = -INFINITY;
#pragma unroll 8
    for (int c = 0; c < p.nc; ++c) m = fmaxf(m, p.cmax[(long long)r * p.nc + c]);
    return m;
}

// inclusive prefix of v over the 256 threads in thread order; `total` = the block's sum
__device__ u64 block_incl_scan(u64 v, u64* wtot, u64& total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    u64 off = 0;
    for (int j = 0; j < w; ++j) off += wtot[j];
    total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    return v + off;
}

__device__ RowState init_state() {
    RowState s;
    s.prefix = 0; s.cnt_above = 0; s.mass_above = 0; s.target = 0; s.tk = 0; s.tie_keep = 0; s.tp = 0; s.tp_off = 1;
    return s;
}

// The state entering step s: the stored state entering step s-1 plus the histograms step s-1 wrote.  The block of chunk 0 stores it
// (slot s-1) for the launches after the last step.  Every workgroup of the row computes the same integers.
__device__ RowState advance(const FP& p, int r, int s, float m) {
    __shared__ u64 suf[SF_BINS];
    __shared__ RowState sres;
    if (s == 0) return init_state();
    const int tid = threadIdx.x, q = s - 1;
    RowState prev = q == 0 ? init_state() : p.st[(long long)r * SF_STEPS + q - 1];
    const bool kstep = q < p.nk;
    const int L = kstep ? q : q - p.nk;
    u64 v = 0;
    if (kstep) {
        const uint32_t* h = p.cnt + ((long long)L * p.rows + r) * p.nc * SF_BINS + tid;
#pragma unroll 8
        for (int c = 0; c < p.nc; ++c) v += h[(long long)c * SF_BINS];
    } else {
        const u64* h = p.mass + ((long long)L * p.rows + r) * p.nc * SF_BINS + tid;
#pragma unroll 8
        for (int c = 0; c < p.nc; ++c) v += h[(long long)c * SF_BINS];
        // the survivors AT the top-k threshold are not in the histograms (they are restricted to key > tk): add their mass here
        const int sh = 24 - 8 * L;
        if (prev.tie_keep > 0 && (L == 0 || (prev.tk >> (sh + 8)) == prev.prefix) && (int)((prev.tk >> sh) & 255u) == tid)
            v += (u64)prev.tie_keep * fxm(kval(prev.tk), m);
    }
    suf[tid] = v;
    __syncthreads();
    for (int o = 1; o < SF_BINS; o <<= 1) {
        const u64 add = tid + o < SF_BINS ? suf[tid + o] : 0ull;
        __syncthreads();
        suf[tid] += add;
        __syncthreads();
    }
    u64 above, target;
    if (kstep) {
        above = prev.cnt_above;
        target = (u64)p.k;
    } else {
        if (L == 0) {
            prev.mass_above = 0;
            const u64 Z = suf[0];
            prev.tp_off = Z == 0 ? 1u : 0u;
            double t = ceil((double)p.p * (double)Z);
            prev.target = t < 1.0 ? 1ull : (u64)t;
            if (prev.target > Z && Z > 0) prev.target = Z;
        }
        above = prev.mass_above;
        target = prev.target;
    }
    if (tid == 0) sres = prev;                       // default (unreachable when the histograms are consistent): digit 0
    __syncthreads();
    const u64 here = above + suf[tid];
    const u64 next = above + (tid + 1 < SF_BINS ? suf[tid + 1] : 0ull);
    const bool pick = here >= target && (tid == SF_BINS - 1 || next < target);
    if (pick) {
        RowState n = prev;
        n.prefix = (L == 0 ? 0u : prev.prefix << 8) | (uint32_t)tid;
        if (kstep) {
            n.cnt_above = (uint32_t)next;
            if (L == 3) {
                const uint32_t ties = (uint32_t)(suf[tid] - (tid + 1 < SF_BINS ? suf[tid + 1] : 0ull));
                n.tk = n.prefix;
                n.tie_keep = p.kmode == 2 ? (uint32_t)p.k - n.cnt_above : ties;
                n.prefix = 0;
            }
        } else {
            n.mass_above = next;
            if (L == 3) n.tp = n.prefix;
        }
        sres = n;
    }
    __syncthreads();
    RowState out = sres;
    if (!kstep && prev.tp_off) out = prev;           // no mass in the row: top-p keeps every top-k survivor
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) p.st[(long long)r * SF_STEPS + q] = out;
    return out;
}

// ---- 0: penalty bitmap of each row (one workgroup per row)
__global__ __launch_bounds__(SF_THREADS) void sf_bitmap(FP p) {
    __shared__ uint32_t bm[SF_MAX_PEN_V / 32];
    const int r = blockIdx.x, tid = threadIdx.x;
    for (int w = tid; w < p.bmw; w += SF_THREADS) bm[w] = 0u;
    __syncthreads();
    const int n = min(p.n_ids[r], p.max_ids);
    const int32_t* ids = p.pen_ids + (long long)r * p.max_ids;
    for (int j = tid; j < n; j += SF_THREADS) {
        const int id = ids[j];
        if (id >= 0 && id < p.V) atomicOr(&bm[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    for (int w = tid; w < p.bmw; w += SF_THREADS) p.bm[(long long)r * p.bmw + w] = bm[w];
}

// ---- 1: processed values (mix, intervals, penalty, temperature) and the chunk's first maximum
template <bool RB>
__global__ __launch_bounds__(SF_THREADS) void sf_prep(FP p) {
#pragma clang fp contract(off)
    __shared__ int siv[2 * SF_MAX_IV];
    __shared__ float wv[4];
    __shared__ int wi[4];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (p.allowed)
        for (int q = tid; q < 2 * p.n_iv; q += SF_THREADS) siv[q] = p.allowed[(long long)r * p.n_iv * 2 + q];
    __syncthreads();
    const float* row = p.logits + (long long)r * p.ld;
    const float* crow = p.cfg_logits ? p.cfg_logits + (long long)r * p.ld : nullptr;
    const uint32_t* bm = p.bm ? p.bm + (long long)r * p.bmw : nullptr;
    float* xr = p.xs + (long long)r * p.vp;
    // every load of the chunk in flight at once (32 per lane), then the arithmetic
    float rv[SF_PER_THREAD], cv[SF_PER_THREAD];
#pragma unroll
    for (int it = 0; it < SF_PER_THREAD; ++it) {
        const int i = c * SF_CHUNK + it * SF_THREADS + tid;
        rv[it] = i < p.V ? row[i] : 0.f;
        cv[it] = crow && i < p.V ? crow[i] : 0.f;
    }
    float best = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int it = 0; it < SF_PER_THREAD; ++it) {
        const int i = c * SF_CHUNK + it * SF_THREADS + tid;
        if (i >= p.V) continue;
        float x = cfg_mix<RB>(rv[it], crow ? &cv[it] : nullptr, p.cfg, p.omc);
        if (p.allowed) {
            bool ok = false;
            for (int q = 0; q < p.n_iv; ++q) ok |= i >= siv[2 * q] && i < siv[2 * q + 1];
            if (!ok) x = -INFINITY;
        }
        if (bm && ((bm[i >> 5] >> (i & 31)) & 1u)) x = x < 0.f ? x * p.pen : x / p.pen;
        x = x / p.T;
        x = x + 0.f;                                 // -0 -> +0: one key per value
        xr[i] = x;
        if (bi == INT_MAX || x > best) { best = x; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != INT_MAX && (bi == INT_MAX || amax_before(ov, oi, best, bi))) { best = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { wv[tid >> 6] = best; wi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (wi[w] != INT_MAX && (bi == INT_MAX || amax_before(wv[w], wi[w], best, bi))) { best = wv[w]; bi = wi[w]; }
        p.cmax[(long long)r * p.nc + c] = best;
        p.carg[(long long)r * p.nc + c] = bi;
    }
}

// ---- 2: one radix step: the chunk's histogram of digit L among the ids still in the searched bucket
__global__ __launch_bounds__(SF_THREADS) void sf_hist(FP p, int s) {
    __shared__ uint32_t hc[SF_BINS];
    __shared__ u64 hm[SF_BINS];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const float* xr = p.xs + (long long)r * p.vp;
    float xv[SF_PER_THREAD];                         // the chunk's loads overlap the bucket search below
#pragma unroll
    for (int it = 0; it < SF_PER_THREAD; ++it) {
        const int i = c * SF_CHUNK + it * SF_THREADS + tid;
        xv[it] = i < p.V ? xr[i] : -INFINITY;
    }
    const bool kstep = s < p.nk;
    const float m = kstep ? 0.f : row_max(p, r);
    const RowState st = advance(p, r, s, m);
    const int L = kstep ? s : s - p.nk;
    const int sh = 24 - 8 * L;
    hc[tid] = 0u;
    hm[tid] = 0ull;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SF_PER_THREAD; ++it) {
        const int i = c * SF_CHUNK + it * SF_THREADS + tid;
        if (i >= p.V) continue;
        const float x = xv[it];
        const uint32_t key = fkey(x);
        if (L > 0 && (key >> (sh + 8)) != st.prefix) continue;
        const int d = (key >> sh) & 255u;
        if (kstep) {
            atomicAdd(&hc[d], 1u);
        } else if (key > st.tk) {
            const u64 w = fxm(x, m);
            if (w) atomicAdd(&hm[d], w);
        }
    }
    __syncthreads();
    const long long o = (((long long)L * p.rows + r) * p.nc + c) * SF_BINS + tid;
    if (kstep) p.cnt[o] = hc[tid];
    else p.mass[o] = hm[tid];
}

struct Cut {
    uint32_t cut;           // ids with key > cut survive
    int partial;            // ids AT cut: exact top-k keeps the first tie_keep of them by id; otherwise all
    uint32_t tie_keep;
};

__device__ Cut final_cut(const FP& p, const RowState& st) {
    Cut k;
    k.cut = st.tk;
    if (p.np && !st.tp_off && st.tp > k.cut) k.cut = st.tp;
    k.partial = p.kmode == 2 && k.cut == st.tk;
    k.tie_keep = st.tie_keep;
    return k;
}

// ties at the cut in the chunks before c (exact top-k): the last top-k histogram counts them per chunk
__device__ uint32_t ties_before(const FP& p, int r, int c, const Cut& k) {
    if (!k.partial) return 0u;
    const uint32_t* h = p.cnt + ((3ll * p.rows + r) * p.nc) * SF_BINS + (k.cut & 255u);
    uint32_t n = 0;
#pragma unroll 8
    for (int j = 0; j < c; ++j) n += h[(long long)j * SF_BINS];
    return n;
}

// Survivors of chunk c of row r.  Thread t owns the 32 consecutive ids c * 8192 + 32 t + j, so a single block scan of the per-thread
// sums puts every id in ascending-id CDF order.  Fills x / w (surviving mass, 0 if removed) / kept per id and returns the exclusive
// prefix of this thread's mass; `total` = the chunk's surviving mass.  Exact top-k ties at the cut are ranked by id from `tie0`,
// the ties of the chunks before c.
__device__ u64 chunk_survivors(const FP& p, int r, int c, const Cut& k, float m, uint32_t tie0, float (&x)[SF_PER_THREAD],
                               u64 (&w)[SF_PER_THREAD], u64& total) {
    __shared__ u64 wtot[4];
    const int tid = threadIdx.x;
    const int i0 = c * SF_CHUNK + tid * SF_PER_THREAD;
    const float* xr = p.xs + (long long)r * p.vp;
#pragma unroll
    for (int j = 0; j < SF_PER_THREAD; ++j) x[j] = i0 + j < p.V ? xr[i0 + j] : -INFINITY;
    u64 nt = 0;
    if (k.partial) {
#pragma unroll
        for (int j = 0; j < SF_PER_THREAD; ++j) nt += i0 + j < p.V && fkey(x[j]) == k.cut;
    }
    u64 tie_rank = 0, sum = 0;
    if (k.partial) {                                 // uniform: every thread takes this branch or none
        u64 unused;
        tie_rank = block_incl_scan(nt, wtot, unused) - nt + tie0;   // ties before this thread's first id
    }
#pragma unroll
    for (int j = 0; j < SF_PER_THREAD; ++j) {
        const uint32_t key = fkey(x[j]);
        bool kept = i0 + j < p.V && key >= k.cut;
        if (k.partial && kept && key == k.cut) kept = ++tie_rank <= k.tie_keep;
        w[j] = kept ? fxm(x[j], m) : 0ull;
        if (!kept) x[j] = -INFINITY;
        sum += w[j];
    }
    return block_incl_scan(sum, wtot, total) - sum;
}

// ---- 3: survivors of each chunk: their mass, and the processed row with -inf where removed
__global__ __launch_bounds__(SF_THREADS) void sf_mark(FP p) {
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const float m = row_max(p, r);
    const RowState st = advance(p, r, p.nk + p.np, m);
    const Cut k = final_cut(p, st);
    float x[SF_PER_THREAD];
    u64 w[SF_PER_THREAD], total;
    chunk_survivors(p, r, c, k, m, ties_before(p, r, c, k), x, w, total);
    if (p.scores) {
        const int i0 = c * SF_CHUNK + tid * SF_PER_THREAD;
        float* out = p.scores + (long long)r * p.lds;
#pragma unroll
        for (int j = 0; j < SF_PER_THREAD; ++j)
            if (i0 + j < p.V) out[i0 + j] = x[j];
    }
    if (tid == 0) p.kmass[(long long)r * p.nc + c] = total;
}

// ---- 4: the draw (one workgroup per row): chunk of u * Z by the chunk sums, then the id inside it; u == NULL: first argmax
__global__ __launch_bounds__(SF_THREADS) void sf_draw(FP p) {
    __shared__ int s_tok;
    __shared__ int s_chunk;
    __shared__ u64 s_local;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        float best = -INFINITY;
        int bi = INT_MAX;
        for (int c = 0; c < p.nc; ++c) {
            const float v = p.cmax[(long long)r * p.nc + c];
            const int i = p.carg[(long long)r * p.nc + c];
            if (bi == INT_MAX || amax_before(v, i, best, bi)) { best = v; bi = i; }
        }
        s_tok = bi;
        s_chunk = -1;
        if (p.u) {
            u64 Z = 0;
#pragma unroll 8
            for (int c = 0; c < p.nc; ++c) Z += p.kmass[(long long)r * p.nc + c];
            if (Z > 0) {
                float uu = p.u[r];
                uu = uu > 0.f ? uu : 0.f;
                u64 t = (u64)((double)uu * (double)Z);
                if (t >= Z) t = Z - 1;
                u64 acc = 0;
                for (int c = 0; c < p.nc; ++c) {
                    const u64 w = p.kmass[(long long)r * p.nc + c];
                    if (t < acc + w) { s_chunk = c; s_local = t - acc; break; }
                    acc += w;
                }
            }
        }
    }
    __syncthreads();
    const int cc = s_chunk;
    if (cc >= 0) {
        const float m = row_max(p, r);
        const int ns = p.nk + p.np;
        const RowState st = ns == 0 ? init_state() : p.st[(long long)r * SF_STEPS + ns - 1];
        const Cut k = final_cut(p, st);
        float x[SF_PER_THREAD];
        u64 w[SF_PER_THREAD], total;
        u64 acc = chunk_survivors(p, r, cc, k, m, ties_before(p, r, cc, k), x, w, total);
        // the id whose CDF step covers s_local: acc + w_before <= s_local < acc + w_before + w (w > 0 there: exactly one id)
        const u64 tl = s_local;
#pragma unroll
        for (int j = 0; j < SF_PER_THREAD; ++j) {
            if (w[j] > 0 && acc <= tl && tl < acc + w[j]) s_tok = cc * SF_CHUNK + tid * SF_PER_THREAD + j;
            acc += w[j];
        }
    }
    __syncthreads();
    if (tid == 0) p.token[r] = s_tok;
}

struct SfLayout {
    size_t xs, cmax, carg, cnt, mass, st, kmass, bm, total;
    int nc, vp, bmw;
};

SfLayout sf_layout(int rows, int V) {
    SfLayout l;
    l.nc = cdiv(V, SF_CHUNK);
    l.vp = (V + 63) / 64 * 64;
    l.bmw = cdiv(V, 32);
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += (b + 255) / 256 * 256; return at; };
    const size_t R = (size_t)rows, NC = (size_t)l.nc;
    l.xs = take(R * l.vp * 4);
    l.cmax = take(R * NC * 4);
    l.carg = take(R * NC * 4);
    l.cnt = take(4 * R * NC * SF_BINS * 4);
    l.mass = take(4 * R * NC * SF_BINS * 8);
    l.st = take(R * SF_STEPS * sizeof(RowState));
    l.kmass = take(R * NC * 8);
    l.bm = take(R * l.bmw * 4);
    l.total = o;
    return l;
}

}  // namespace

extern "C" size_t afhip_sample_filter_workspace_bytes(int rows, int V) {
    if (rows <= 0 || V <= 0 || V >= SF_MAX_V) return 0;
    return sf_layout(rows, V).total;
}

extern "C" int afhip_sample_filter(const afhip_sample_filter_args* a, void* ws, size_t ws_bytes, void* stream) {
    AFHIP_CHECK(a != nullptr, "afhip_sample_filter: null args");
    AFHIP_CHECK(a->logits != nullptr, "afhip_sample_filter: null logits");
    AFHIP_CHECK(a->rows <= 65535, "afhip_sample_filter: rows=%d > 65535", a->rows);
    AFHIP_CHECK(a->rows > 0 && a->V > 0 && a->V < SF_MAX_V && a->ld >= a->V, "afhip_sample_filter: bad shape rows=%d V=%d ld=%d (0 < V < 2^23, ld >= V)",
                a->rows, a->V, a->ld);
    AFHIP_CHECK(a->model_dtype == AFHIP_F32 || a->model_dtype == AFHIP_BF16, "afhip_sample_filter: bad model_dtype");
    AFHIP_CHECK(a->allowed == nullptr || (a->n_iv >= 1 && a->n_iv <= SF_MAX_IV), "afhip_sample_filter: n_iv=%d must be in [1,%d]", a->n_iv, SF_MAX_IV);
    AFHIP_CHECK(a->penalty > 0.f, "afhip_sample_filter: repetition penalty must be > 0");
    AFHIP_CHECK(a->temperature > 0.f, "afhip_sample_filter: temperature must be > 0");
    AFHIP_CHECK(a->top_k >= 0 && a->top_k <= a->V, "afhip_sample_filter: top_k=%d must be in [0,%d] (0 = off)", a->top_k, a->V);
    AFHIP_CHECK(a->top_p > 0.f && a->top_p <= 1.f, "afhip_sample_filter: top_p must be in (0, 1]");
    const bool pen = a->penalty != 1.f && a->penalty_ids != nullptr;
    AFHIP_CHECK(!pen || (a->n_ids != nullptr && a->max_ids > 0), "afhip_sample_filter: penalty_ids needs n_ids and max_ids > 0");
    AFHIP_CHECK(!pen || a->V <= SF_MAX_PEN_V, "afhip_sample_filter: a repetition penalty needs V <= %d", SF_MAX_PEN_V);
    AFHIP_CHECK(a->scores == nullptr || a->ld_scores >= a->V, "afhip_sample_filter: ld_scores=%d < V", a->ld_scores);
    const SfLayout l = sf_layout(a->rows, a->V);
    AFHIP_CHECK(ws != nullptr && ((uintptr_t)ws & 255u) == 0, "afhip_sample_filter: workspace must be non-null and 256-byte aligned");
    AFHIP_CHECK(ws_bytes >= l.total, "afhip_sample_filter: workspace %zu bytes < %zu (afhip_sample_filter_workspace_bytes)", ws_bytes, l.total);
    if (a->token == nullptr && a->scores == nullptr) return 0;

    char* w = (char*)ws;
    FP p;
    p.logits = a->logits; p.cfg_logits = a->cfg_logits; p.cfg = a->cfg;
    p.omc = a->one_minus_cfg != 0.f ? a->one_minus_cfg : (float)(1.0 - (double)a->cfg);
    p.rows = a->rows; p.V = a->V; p.ld = a->ld; p.nc = l.nc; p.vp = l.vp; p.bmw = l.bmw;
    p.allowed = a->allowed; p.n_iv = a->n_iv;
    p.pen_ids = a->penalty_ids; p.n_ids = a->n_ids; p.max_ids = a->max_ids; p.pen = a->penalty; p.T = a->temperature;
    const bool kact = a->top_k > 0 && a->top_k < a->V;
    p.kmode = kact ? (a->exact_k ? 2 : 1) : 0;
    p.k = a->top_k; p.p = a->top_p;
    const bool need_filter = a->u != nullptr || a->scores != nullptr;
    p.nk = kact && need_filter ? 4 : 0;
    p.np = a->top_p < 1.f && need_filter ? 4 : 0;
    p.xs = (float*)(w + l.xs); p.cmax = (float*)(w + l.cmax); p.carg = (int*)(w + l.carg);
    p.cnt = (uint32_t*)(w + l.cnt); p.mass = (u64*)(w + l.mass); p.st = (RowState*)(w + l.st); p.kmass = (u64*)(w + l.kmass);
    p.bm = pen ? (uint32_t*)(w + l.bm) : nullptr;
    p.u = a->u; p.scores = a->scores; p.lds = a->ld_scores; p.token = a->token;

    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(l.nc, a->rows), blk(SF_THREADS);
    if (pen) hipLaunchKernelGGL(sf_bitmap, dim3(a->rows), blk, 0, s, p);
    if (a->model_dtype == AFHIP_BF16) hipLaunchKernelGGL(sf_prep<true>, grid, blk, 0, s, p);
    else hipLaunchKernelGGL(sf_prep<false>, grid, blk, 0, s, p);
    for (int st = 0; st < p.nk + p.np; ++st) hipLaunchKernelGGL(sf_hist, grid, blk, 0, s, p, st);
    if (need_filter) hipLaunchKernelGGL(sf_mark, grid, blk, 0, s, p);
    if (a->token) hipLaunchKernelGGL(sf_draw, dim3(a->rows), blk, 0, s, p);
    AFHIP_LAUNCH_CHECK();
    return 0;
}
