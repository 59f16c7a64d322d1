// Flash-style attention for gfx950 (encoder: non-causal + per-clip key length; LLM prefill/decode: causal, GQA).
// Scores never leave registers.  Orientation (cdna guide, "accumulator tile as the next MFMA's operand"):
//   S^T[key, query] = K_tile . Q^T      (A = K rows from LDS, B = Q rows held in registers for the whole kernel)
//   O^T[d,   query] = V^T    . P^T      (A = V^T rows from LDS, B = the S^T accumulator registers themselves)
// so the query lives on the MFMA lane: row max / row sum are per-lane loops + one lane^32 exchange, the O rescale
// is a per-lane scalar, and P feeds the second MFMA with no LDS round trip.  The key order inside an S^T tile is
// permuted on the K-load side (bits 2 and 3 of the tile row swapped) so that the V^T fragment of a k-step is 8
// consecutive keys (one 16-byte LDS read in bf16).
// One workgroup = 4 waves = 128 queries of one (batch, head); K/V tiles of 64 keys staged through LDS with
// register prefetch.  Same template for bf16 (32x32x16 MFMA) and exact f32 (32x32x2 MFMA) via common.h mma16.
#include "common.h"
#include <type_traits>
#include <stdlib.h>

namespace {

constexpr int QT = 128, KT = 64;

struct AttnP {
    const char* q;
    const char* k;
    const char* v;
    char* o;
    const int32_t* key_len;
    int B, Tq, Tk, n_q, n_kv, hd;
    long long ld_q, ld_kv, ld_o;
    long long q_bs, kv_bs, o_bs;
    long long q_hs, kv_hs, o_hs;
    int causal, q_pos0;
    float scale_log2;
    int n_xt;               // x-tiles per (batch, head): query tiles, or key ranges when key_split > 0
    int key_split;          // > 0: the x-tile index enumerates key ranges of this many keys (Tq <= 32), partials go to part_o / part_ml
    float* part_o;          // [split][B][n_q][32][HD] unnormalised O^T columns
    float* part_ml;         // [split][B][n_q][32][2]  running max (raw score units) and sum
    const char* new_k;      // decode: fused RoPE + KV append (afhip.h); NULL = off
    const char* new_v;
    long long new_kv_bs;
    const float* rope_cos;
    const float* rope_sin;
    int* ticket;            // split mode: in-launch merge by the last-arriving key-range workgroup (afhip.h); NULL = separate pass
    const int32_t* seq_pos; // split mode: per-sequence position of the token being generated, read on the DEVICE (Tk_b = seq_pos[b] + 1,
                            // RoPE row, append slot); p.Tk is then only the host's upper bound that sized the grid.  NULL = uniform p.Tk
    const int32_t* row_off; // packed (ragged) self-attention: sequence b's rows start at row row_off[b] of q / k / v / o and it has key_len[b]
                            // queries and keys; p.Tq / p.Tk are then only the upper bound that sized the grid.  NULL = [B, T] batches
    unsigned long long* dbg; // diagnostic: s_memtime stamps of workgroup 0 (AFHIP_ATTN_DBGPTR), normally NULL
    int o_img_rows;         // split mode: the merge writes out[b, col] into a fragment-order image of this many rows (afhip.h: out_img_rows); 0 = plain rows
};

__device__ __forceinline__ int swap23(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }
// chunk swizzles that make the 32-row ds_read_b128 operand pattern bank-conflict free (see gemm.hip swz): 128-B rows
// pair up in a 256-B bank row -> (row >> 1) & 7; 256-B rows own a bank row -> row & 15
template <int ROWBYTES> __device__ __forceinline__ int rswz(int row) {
    if constexpr (ROWBYTES == 128) return (row >> 1) & 7;
    else if constexpr (ROWBYTES == 256) return row & 15;
    else return row & 7;
}

// bf16 V tiles stay row-major [key][d] in LDS and are consumed transposed by ds_read_b64_tr_b16: a 16-lane group reads a
// 4-key x 16-d block (lane 4q+p supplies the address of key q, columns 4p..4p+3; lane i receives column i, key q in
// element q).  A 32-lane half therefore touches 4 keys x 64 B; moving that 64-B region by the key index keeps the 4 keys
// on different banks: 128-B rows (two rows per bank row) flip it on bit 1 of the key, 256-B rows rotate it by key & 3.
template <int ROWBYTES> __device__ __forceinline__ int vtrswz(int row) {
    if constexpr (ROWBYTES == 128) return ((row >> 1) & 1) << 2;
    else return (row & 3) << 2;
}
typedef short s16x4 __attribute__((ext_vector_type(4)));

// LAG (bf16, q prescaled to exp2 units, no key split): the softmax with a LAGGED row maximum.  S' = K.Q^T - m_lag leaves the MFMA chain
// ready for exp2 (the chain starts from a 16-register tuple holding -m_lag instead of zeros), so a key tile costs one v_exp_f32, one
// v_add_f32 (row sum) and half a v_cvt_pk per score and nothing else: no per-score max, no scale-and-shift fma, no O rescale.  m_lag
// is the true maximum of the first tile and is raised only when a tile's partial row sum shows a score more than 16 above it
// (P > 2^16): then that tile is redone with its true maximum, O and l rescaled once.  Mathematically the same softmax (every term
// carries the same 2^-m_lag factor, which cancels in O / l); P <= 2^16 keeps f32 sums far from overflow, and bf16 P has the same
// relative precision at any magnitude.
constexpr float LAG_SUM_LIMIT = 65536.f;
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const bf16x2_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

template <typename T, int HD, int NBUF, bool LAG = false>
__global__ __launch_bounds__(256) void attn_kernel(AttnP p) {
    static_assert(!LAG || sizeof(T) == 2, "the lagged-maximum softmax is the bf16 throughput form");
    constexpr int SZ = sizeof(T);
    constexpr int KROWB = HD * SZ;             // bytes per K row in LDS
    constexpr int VROWB = KT * SZ;             // bytes per V^T row in LDS
    constexpr int KCPR = KROWB / 16;           // 16-B chunks per K row (>= 8)
    constexpr int NLD = (KT * KROWB / 16) / 256;  // 16-B chunks per thread per operand tile
    constexpr int EPC = 16 / SZ;               // elements per 16-B chunk
    constexpr int DSTEPS = HD / 16, DT = HD / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int STAGE_BYTES = 2 * KT * KROWB;   // K tile + V tile; two stages, one barrier per key tile
    char* Ks = smem;
    char* Vt = smem + KT * KROWB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    // 1-D grid over (x-tile, head, batch).  Workgroups id and id+8 share an XCD (round-robin dispatch), so with
    // id = xcd + 8 * (xtile + n_xt * head_group), head = 8 * head_group + xcd, the x-tiles (query tiles or key ranges) of one
    // (batch, head) run back to back on ONE XCD and its K/V is fetched from HBM once, not once per query tile
    // (FETCH_SIZE was 2.1 GB per launch for 0.37 GB of q/k/v).  Falls back to head-major order when heads*batch % 8 != 0.
    const int nh = p.n_q * p.B;
    int xt, hb;
    if ((nh & 7) == 0) {
        const int xcd = blockIdx.x & 7, r = blockIdx.x >> 3;
        xt = r % p.n_xt;
        hb = (r / p.n_xt) * 8 + xcd;
    } else {
        xt = blockIdx.x % p.n_xt;
        hb = blockIdx.x / p.n_xt;
    }
    const int b = hb / p.n_q, hq = hb % p.n_q;
    const int hkv = hq / (p.n_q / p.n_kv);
    const int split = p.key_split > 0 ? xt : 0;
    const int q0 = p.key_split > 0 ? 0 : xt * QT;
    const int qrow = q0 + wave * 32 + fr;                 // this lane's query
    // [B, T] batches: sequence b at b * batch stride, p.Tq queries.  Packed batches: at row row_off[b], key_len[b] queries (= keys)
    long long q_off = (long long)b * p.q_bs, kv_off = (long long)b * p.kv_bs, o_off = (long long)b * p.o_bs;
    int Tq = p.Tq;
    if (p.row_off) {
        const long long r = p.row_off[b];
        q_off = r * p.ld_q; kv_off = r * p.ld_kv; o_off = r * p.ld_o;
        Tq = p.key_len[b];
        if (q0 >= Tq) return;                             // query tile past this sequence (workgroup-uniform, before any barrier)
    }
    const int qrow_c = qrow < Tq ? qrow : Tq - 1;
    const int qpos = p.q_pos0 + qrow;
    const int wave_qpos_min = p.q_pos0 + q0 + wave * 32;   // smallest query position held by this wave
    const bool wave_live = q0 + wave * 32 < Tq;            // wave-uniform

    const char* qb = p.q + (q_off + (long long)hq * p.q_hs) * SZ;
    const char* kb = p.k + (kv_off + (long long)hkv * p.kv_hs) * SZ;
    const char* vb = p.v + (kv_off + (long long)hkv * p.kv_hs) * SZ;

    int klen = p.Tk;
    if (p.seq_pos) { const int tk = p.seq_pos[b] + 1; klen = tk < klen ? tk : klen; }   // wave-uniform (b is per workgroup)
    const int tk_b = klen;                                  // keys of THIS sequence (== p.Tk without seq_pos)
    if (p.key_len) { const int kl = p.key_len[b]; klen = kl < klen ? kl : klen; }
    int kend = klen;                                       // keys this workgroup must visit
    if (p.causal) {
        const int last = p.q_pos0 + (q0 + QT - 1 < Tq - 1 ? q0 + QT - 1 : Tq - 1) + 1;
        kend = last < kend ? last : kend;
    }
    int kbeg = 0;
    if (p.key_split > 0) {
        kbeg = split * p.key_split;
        const int ke = kbeg + p.key_split;
        kend = ke < kend ? ke : kend;
        if (p.seq_pos && kbeg >= kend) return;             // key range beyond this sequence's context: nothing to do, the combine
                                                           // pass derives the number of live ranges from seq_pos as well
        if (kbeg > kend) kbeg = kend;
    }
    const float* rope_cos = p.rope_cos;
    const float* rope_sin = p.rope_sin;
    if (p.seq_pos && p.new_k) { rope_cos += (long long)(tk_b - 1) * (HD / 2); rope_sin += (long long)(tk_b - 1) * (HD / 2); }
    const int tbeg = kbeg / KT;
    const int ntiles = (kend + KT - 1) / KT;      // tiles [tbeg, ntiles)

    // decode (key ranges): the first K/V tile goes out BEFORE the q fragments are fetched and rotated -- a workgroup has only two tiles, and
    // q -> RoPE -> tile 0 was one dependent memory round trip more than needed
    u32x4 rk[NLD], rv[NLD];
    auto load_tile = [&](int t) {
        const int k0 = t * KT;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int c = tid + 256 * i;
            const int row = c / KCPR, cc = c % KCPR;
            int key = k0 + row;
            key = key < klen ? key : klen - 1;       // masked keys re-read the last live row: their P is 0, and 0 x (whatever sits behind the
                                                     // sequence -- padding, the next packed clip, stale workspace with NaNs) must stay 0
            const long long off = ((long long)key * p.ld_kv) * SZ + cc * 16;
            rk[i] = ld16(kb + off);
            rv[i] = ld16(vb + off);
            if (p.new_k && k0 + row == tk_b - 1) {
                // fused KV append (decode): this chunk of the token being generated comes from the projection output, not from
                // the cache; k is rotated here (partner elements d +- HD/2 sit KCPR/2 chunks away in the same row), and both are
                // written to the cache for the following steps.  Only the workgroup whose key range holds Tk-1 gets here.
                const char* nk = p.new_k + ((long long)b * p.new_kv_bs + (long long)hkv * HD) * SZ;
                const char* nv = p.new_v + ((long long)b * p.new_kv_bs + (long long)hkv * HD) * SZ;
                const bool lo = cc < KCPR / 2;
                const u32x4 own = ld16(nk + cc * 16), par = ld16(nk + (cc ^ (KCPR / 2)) * 16);
                const int i0 = (lo ? cc : cc - KCPR / 2) * EPC;
                T ov[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float c = rope_cos[i0 + e], sn = rope_sin[i0 + e];
                    const float xo = to_f32<T>(reinterpret_cast<const T*>(&own)[e]), xp = to_f32<T>(reinterpret_cast<const T*>(&par)[e]);
                    // first half: x1 = own, x2 = partner -> x1 c - x2 s;  second half: x2 = own, x1 = partner -> x2 c + x1 s
                    ov[e] = from_f32<T>(lo ? rope_mad(xo, c, -xp, sn) : rope_mad(xo, c, xp, sn));
                }
                rk[i] = *reinterpret_cast<const u32x4*>(ov);
                rv[i] = ld16(nv + cc * 16);
                st16(const_cast<char*>(kb) + off, rk[i]);
                st16(const_cast<char*>(vb) + off, rv[i]);
            }
        }
    };
    const bool early_tile = p.key_split > 0 && ntiles > tbeg;
    if (early_tile) load_tile(tbeg);

    // ---- Q fragments (B operand), resident for the whole kernel ----
    typename Frag8<T>::type qf[DSTEPS];
    {
        const T* qp = reinterpret_cast<const T*>(qb) + (long long)qrow_c * p.ld_q;
#pragma unroll
        for (int dc = 0; dc < DSTEPS; ++dc) qf[dc] = *reinterpret_cast<const typename Frag8<T>::type*>(qp + dc * 16 + fh * 8);
        if (p.new_k) {
            // fused RoPE (decode): element d = dc*16 + fh*8 + e pairs with d + HD/2, i.e. step dc + DSTEPS/2 of the SAME lane.
            // q cos + rotate_half(q) sin with separate roundings, then the storage dtype -- exactly rope_kv_kernel (norm.hip)
#pragma unroll
            for (int dc = 0; dc < DSTEPS / 2; ++dc)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int i = dc * 16 + fh * 8 + e;
                    const float c = rope_cos[i], sn = rope_sin[i];
                    const float x1 = to_f32<T>(qf[dc][e]), x2 = to_f32<T>(qf[dc + DSTEPS / 2][e]);
                    qf[dc][e] = from_f32<T>(rope_mad(x1, c, -x2, sn));
                    qf[dc + DSTEPS / 2][e] = from_f32<T>(rope_mad(x2, c, x1, sn));
                }
        }
    }

    f32x16 ot[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) ot[i][e] = 0.f;
    float m_i = -INFINITY, l_i = 0.f;
    f32x16 cinit;                                   // LAG: -m_lag in all 16 registers, the C input of every tile's first MFMA
    float m_lag = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) cinit[e] = 0.f;

    auto store_tile = [&](int buf) {
        char* Ks = smem + buf * STAGE_BYTES;
        char* Vt = Ks + KT * KROWB;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int c = tid + 256 * i;
            const int row = c / KCPR, cc = c % KCPR;
            st16(Ks + row * KROWB + ((cc ^ rswz<KROWB>(row)) << 4), rk[i]);
            if constexpr (SZ == 2) {
                // bf16: V stays row-major [key][d] (read back transposed by ds_read_b64_tr_b16)
                st16(Vt + row * KROWB + ((cc ^ vtrswz<KROWB>(row)) << 4), rv[i]);
            } else {
                // f32 (parity mode): transpose while storing, element e of this chunk is V[key=row][d = cc*EPC + e] -> Vt[d][key]
                const int kch = row / EPC, kin = row % EPC;
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const int d = cc * EPC + e;
                    char* dst = Vt + d * VROWB + ((kch ^ rswz<VROWB>(d)) << 4) + kin * SZ;
                    *reinterpret_cast<uint32_t*>(dst) = rv[i][e];
                }
            }
        }
    };

    if (ntiles > tbeg) {
        if (!early_tile) load_tile(tbeg);
        store_tile(0);
    }
    __syncthreads();

#ifdef AFHIP_ATTN_STAMPS   /* diagnostic build: -DAFHIP_ATTN_STAMPS, tools/attn_stamps.py */
#define AT_STAMP(k) do { if (p.dbg && blockIdx.x == 0 && (wave == 0 || wave == 3) && lane == 0 && t >= 8 && t < 12) p.dbg[((wave ? 1 : 0) * 4 + (t - 8)) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define AT_STAMP(k) do { } while (0)
#endif
    // one key tile; the LDS stage is a COMPILE-TIME constant (the loop below alternates two instantiations), so every fragment
    // address is a loop-invariant lane offset plus an immediate: ~20 v_add_u32 per tile fewer in a VALU-bound loop
    auto tile_body = [&](const int t, auto cur_v) __attribute__((always_inline)) {
        const int cur = NBUF == 2 ? (int)cur_v : 0;      // an integral_constant folds after inlining, an int stays a run-time value
        AT_STAMP(0);
        const int k0 = t * KT;
        Ks = smem + cur * STAGE_BYTES;
        Vt = Ks + KT * KROWB;
        if (t + 1 < ntiles) load_tile(t + 1);

        // a wave whose 32 query rows all lie past the sequence (decode: the GQA group's few rows live in wave 0 alone) only helps with the tile
        // loads and the barriers: its S / softmax / PV would be thrown away and its fragment reads compete for the LDS with the live wave's
        if (wave_live) {
        // ---- S^T = K . Q^T for the two 32-key sub-tiles ----
        f32x16 st[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if constexpr (!LAG) {
#pragma unroll
                for (int e = 0; e < 16; ++e) st[ks][e] = 0.f;
            }
            const int krow = ks * 32 + swap23(fr);
#pragma unroll
            for (int dc = 0; dc < DSTEPS; ++dc) {
                typename Frag8<T>::type kf;
                if constexpr (SZ == 2) {
                    const int ch = dc * 2 + fh;
                    kf = *reinterpret_cast<const bf16x8*>(Ks + krow * KROWB + ((ch ^ rswz<KROWB>(krow)) << 4));
                } else {
                    const int ch = dc * 4 + fh * 2;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(Ks + krow * KROWB + ((ch ^ rswz<KROWB>(krow)) << 4));
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(Ks + krow * KROWB + (((ch + 1) ^ rswz<KROWB>(krow)) << 4));
                    kf = f32x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                }
                if constexpr (LAG) st[ks] = mma16(kf, qf[dc], dc == 0 ? cinit : st[ks]);
                else st[ks] = mma16(kf, qf[dc], st[ks]);
            }
        }

        AT_STAMP(1);
        // ---- online softmax (query = this lane's column).  Masking is compiled into boundary tiles only (wave-uniform
        //      branch): interior tiles run max / fma / exp2 / add per score and nothing else. ----
        const bool edge = (k0 + KT > klen) || (p.causal && (k0 + KT - 1 > wave_qpos_min));
        if (edge) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = k0 + ks * 32 + swap23(mfma32_row(e, lane));
                    const bool ok = key < klen && (!p.causal || key <= qpos);
                    st[ks][e] = ok ? st[ks][e] : -INFINITY;
                }
        }
        uint32_t pk[2][8];                                   // LAG: P as packed bf16 pairs, the B operand of the O^T MFMAs
        if constexpr (LAG) {
            float psum = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    const float p0 = __builtin_amdgcn_exp2f(st[ks][e]), p1 = __builtin_amdgcn_exp2f(st[ks][e + 1]);
                    psum += p0;
                    psum += p1;
                    pk[ks][e >> 1] = cvt_pk_bf16(p0, p1);
                }
            const bool first = t == tbeg;
            if (first || __any(!(psum <= LAG_SUM_LIMIT))) {    // wave-uniform; NaN-safe (inf - inf cannot occur: m_lag is finite)
                float mx = -INFINITY;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, st[ks][e]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));         // the two lanes of a query agree
                // raise the lag to this tile's true maximum (first tile: SET it, O and l are still empty) -- only for the queries whose OWN
                // partial sum tripped the limit: a query's bits must not depend on which other queries share its wave
                const int own = !(psum <= LAG_SUM_LIMIT) ? 1 : 0;
                const bool trig = first || (own | __shfl_xor(own, 32, 64)) != 0;
                float d = (trig && (first || mx > 0.f)) ? mx : 0.f;
                d = (d == -INFINITY) ? 0.f : d;
                if (!first) {
                    const float alpha = __builtin_amdgcn_exp2f(-d);
                    l_i *= alpha;
#pragma unroll
                    for (int i = 0; i < DT; ++i)
#pragma unroll
                        for (int e = 0; e < 16; ++e) ot[i][e] *= alpha;
                }
                m_lag += d;
#pragma unroll
                for (int e = 0; e < 16; ++e) cinit[e] = -m_lag;
                psum = 0.f;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int e = 0; e < 16; e += 2) {
                        const float p0 = __builtin_amdgcn_exp2f(st[ks][e] - d), p1 = __builtin_amdgcn_exp2f(st[ks][e + 1] - d);
                        psum += p0;
                        psum += p1;
                        pk[ks][e >> 1] = cvt_pk_bf16(p0, p1);
                    }
            }
            l_i += psum;
        } else {
            float mx = -INFINITY;
    #pragma unroll
            for (int ks = 0; ks < 2; ++ks)
    #pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, st[ks][e]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_i, mx);                 // raw (unscaled) score units
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            if (__any(m_new != m_i)) {                           // the running max moved for some query of this wave
                const float alpha = __builtin_amdgcn_exp2f((m_i - m_use) * p.scale_log2);   // m_i = -inf -> 0
                l_i *= alpha;
    #pragma unroll
                for (int i = 0; i < DT; ++i)
    #pragma unroll
                    for (int e = 0; e < 16; ++e) ot[i][e] *= alpha;
                m_i = m_new;
            }
            const float moff = -m_use * p.scale_log2;
            float psum = 0.f;
    #pragma unroll
            for (int ks = 0; ks < 2; ++ks)
    #pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(st[ks][e], p.scale_log2, moff));
                    st[ks][e] = pv;
                    psum += pv;
                }
            l_i += psum;

        }

        AT_STAMP(2);
        // ---- O^T += V^T . P^T ; step s covers keys [16s, 16s+16) of the tile ----
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            typename Frag8<T>::type pf;
            if constexpr (LAG) {
                const u32x4 w = {pk[s >> 1][4 * (s & 1)], pk[s >> 1][4 * (s & 1) + 1], pk[s >> 1][4 * (s & 1) + 2], pk[s >> 1][4 * (s & 1) + 3]};
                pf = __builtin_bit_cast(bf16x8, w);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = from_f32<T>(st[s >> 1][8 * (s & 1) + j]);
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int vrow = dt * 32 + fr;
                typename Frag8<T>::type vf;
                if constexpr (SZ == 2) {
                    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, gsel = (lane >> 4) & 1;
                    const int col = dt * 32 + gsel * 16 + tp * 4;          // first of this lane's 4 address columns
                    const int key0 = s * 16 + fh * 8 + tq, key1 = key0 + 4;
                    const char* a0 = Vt + key0 * KROWB + (((col >> 3) ^ vtrswz<KROWB>(key0)) << 4) + (col & 7) * 2;
                    const char* a1 = Vt + key1 * KROWB + (((col >> 3) ^ vtrswz<KROWB>(key1)) << 4) + (col & 7) * 2;
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
                    typedef short s16x8 __attribute__((ext_vector_type(8)));
                    const s16x8 both = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    vf = __builtin_bit_cast(bf16x8, both);
                } else {
                    const int ch = s * 4 + fh * 2;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(Vt + vrow * VROWB + ((ch ^ rswz<VROWB>(vrow)) << 4));
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(Vt + vrow * VROWB + (((ch + 1) ^ rswz<VROWB>(vrow)) << 4));
                    vf = f32x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                }
                ot[dt] = mma16(vf, pf, ot[dt]);
            }
        }

        }   // wave_live
        AT_STAMP(3);
        if constexpr (NBUF == 2) {
            if (t + 1 < ntiles) store_tile(cur ^ 1);   // the other stage: its last readers passed the previous barrier
            AT_STAMP(4);
            __syncthreads();
            AT_STAMP(5);
        } else {
            __syncthreads();
            if (t + 1 < ntiles) store_tile(0);
            __syncthreads();
        }
    };
    if constexpr (HD == 64 && SZ == 2) {
        for (int t = tbeg; t < ntiles; t += 2) {
            tile_body(t, std::integral_constant<int, 0>{});
            if (t + 1 < ntiles) tile_body(t + 1, std::integral_constant<int, 1>{});
        }
    } else {
        // the head_dim-128 and f32 forms keep ONE body (two copies of it cost them registers they do not have)
        for (int t = tbeg; t < ntiles; ++t) tile_body(t, (t - tbeg) & 1);
    }

    // ---- normalise and write O[query, d] (or the unnormalised partial of this key range) ----
    const float l_tot = l_i + __shfl_xor(l_i, 32, 64);
    if (p.key_split > 0) {
        if (wave == 0 && qrow < p.Tq) {
            const long long slot = (((long long)split * p.B + b) * p.n_q + hq) * 32 + fr;
            float* po = p.part_o + slot * HD;
            if (p.ticket) {
                // in-launch merge: the partials are stored WRITE-THROUGH (sc1: relaxed agent-scope 8-byte stores), so the producer needs no
                // release fence (cdna guide, Guideline 16 R1) -- the L2 write-back of a release in each of the ~256 workgroups is what made
                // the fenced form slower than a separate combine launch
                typedef unsigned long long u64;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int d = dt * 32 + 8 * g + 4 * fh;
                        const f32x2 lo = {ot[dt][4 * g], ot[dt][4 * g + 1]}, hi = {ot[dt][4 * g + 2], ot[dt][4 * g + 3]};
                        __hip_atomic_store(reinterpret_cast<u64*>(po + d), __builtin_bit_cast(u64, lo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(reinterpret_cast<u64*>(po + d + 2), __builtin_bit_cast(u64, hi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                if (fh == 0) {
                    const f32x2 ml = {m_i, l_tot};
                    __hip_atomic_store(reinterpret_cast<u64*>(p.part_ml + slot * 2), __builtin_bit_cast(u64, ml), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int d = dt * 32 + 8 * g + 4 * fh;
                        *reinterpret_cast<f32x4*>(po + d) = f32x4{ot[dt][4 * g], ot[dt][4 * g + 1], ot[dt][4 * g + 2], ot[dt][4 * g + 3]};
                    }
                if (fh == 0) { p.part_ml[slot * 2] = m_i; p.part_ml[slot * 2 + 1] = l_tot; }
            }
        }
        if (p.ticket == nullptr) return;
        const int n_live = p.seq_pos ? (tk_b + p.key_split - 1) / p.key_split : p.n_xt;
        // ---- in-launch merge (cdna guide, Guideline 16 counter form): publish, take a ticket, the last arriver merges ----
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's partial stores have left
        __syncthreads();                                                   // ... and every wave's
        int* flag = reinterpret_cast<int*>(smem);                          // the K/V tiles are dead: their LDS carries the verdict
        if (tid == 0) {
            // the ticket is an agent-scope RELEASE: it orders this workgroup's partial stores (already write-through and drained) before the
            // count another XCD's merging workgroup acquires on -- the relaxed form worked on gfx950 but was a data race under the HSA memory
            // model.  This path is not the default (option DECODE_MERGE): the separate merge launch is faster.
            const int tk = __hip_atomic_fetch_add(p.ticket + hb, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            flag[0] = (tk == n_live - 1) ? 1 : 0;
        }
        __syncthreads();
        if (flag[0] == 0) return;                                          // wave-uniform
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        // same arithmetic, same order over the key ranges as attn_combine_kernel
        for (int idx = tid; idx < p.Tq * HD; idx += 256) {
            const int qr = idx / HD, d = idx - qr * HD;
            float m = -INFINITY;
            for (int sp = 0; sp < n_live; ++sp) m = fmaxf(m, p.part_ml[((((long long)sp * p.B + b) * p.n_q + hq) * 32 + qr) * 2]);
            float l = 0.f, o = 0.f;
            for (int sp = 0; sp < n_live; ++sp) {
                const long long slot = (((long long)sp * p.B + b) * p.n_q + hq) * 32 + qr;
                const float ms = p.part_ml[slot * 2];
                const float w = (ms == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((ms - m) * p.scale_log2);
                l += p.part_ml[slot * 2 + 1] * w;
                o += p.part_o[slot * HD + d] * w;
            }
            T* op = reinterpret_cast<T*>(p.o) + (long long)b * p.o_bs + (long long)qr * p.ld_o + (long long)hq * p.o_hs;
            op[d] = from_f32<T>(l > 0.f ? o / l : 0.f);
        }
        if (tid == 0) p.ticket[hb] = 0;                                    // ready for the next launch (ordered by the kernel boundary)
        return;
    }
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    if (qrow < Tq) {
        T* op = reinterpret_cast<T*>(p.o) + o_off + (long long)qrow * p.ld_o + (long long)hq * p.o_hs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = dt * 32 + 8 * g + 4 * fh;
                if constexpr (SZ == 2) {
                    bf16x4 w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = (bf16)(ot[dt][4 * g + e] * inv);
                    *reinterpret_cast<bf16x4*>(op + d) = w;
                } else {
                    f32x4 w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = ot[dt][4 * g + e] * inv;
                    *reinterpret_cast<f32x4*>(op + d) = w;
                }
            }
    }
}

// merge the key-range partials of the split kernel: out = sum_s O_s * 2^((m_s - m) c) / sum_s l_s * 2^((m_s - m) c).
// One workgroup per (sequence, head, query row), one thread per output column.  The (max, sum) pairs of the key ranges are staged
// and turned into weights in LDS once per workgroup, and the O_s loads of eight ranges are issued together before they are
// accumulated IN RANGE ORDER (same fma chain as a plain loop, so the bits do not depend on the staging): with one dependent
// load per range the merge of the 118 ranges of a 15 000-key context took 50 us per layer, longer than the attention itself.
constexpr int CMB_CHUNK = 512;
template <typename T>
__global__ void attn_combine_kernel(AttnP p_in, int n_split, int HD) {
    // the arguments this launch reads, fetched in one batch (left alone the compiler spreads them over four dependent scalar round trips in a
    // 5-us kernel); the opaque copy hides the address space of the pointers, the CMB_AS1 casts below put it back
    AttnP p = p_in;
    asm volatile("" : "+s"(p.o), "+s"(p.B), "+s"(p.Tq), "+s"(p.n_q), "+s"(p.ld_o), "+s"(p.o_bs), "+s"(p.o_hs), "+s"(p.scale_log2), "+s"(p.key_split),
                 "+s"(p.part_o), "+s"(p.part_ml), "+s"(p.seq_pos), "+s"(p.o_img_rows), "+s"(n_split), "+s"(HD));
#define CMB_AS1 __attribute__((address_space(1)))
    const CMB_AS1 float* const part_ml = (const CMB_AS1 float*)p.part_ml;
    const CMB_AS1 float* const part_o = (const CMB_AS1 float*)p.part_o;
    __shared__ float s_w[CMB_CHUNK], s_l[CMB_CHUNK], s_red[4];
    const int row = blockIdx.x;                      // (b, hq, qrow) flattened
    const int qrow = row % p.Tq, hq = (row / p.Tq) % p.n_q, b = row / (p.Tq * p.n_q);
    const int d = threadIdx.x;
    if (p.seq_pos) { const int live = (((const CMB_AS1 int32_t*)p.seq_pos)[b] + 1 + p.key_split - 1) / p.key_split; n_split = live < n_split ? live : n_split; }
    auto slot_of = [&](int sp) { return (((long long)sp * p.B + b) * p.n_q + hq) * 32 + qrow; };
    if (n_split <= 16) {
        // short contexts (the 7B decode step: 7 key ranges of 128 keys, 14 of 64): every load of the merge -- the (max, sum) pairs and this thread's O column of
        // all ranges -- is issued before the first is used: one memory round trip instead of three dependent ones (5.7 us per layer for
        // 0.8 MB).  Same maximum, same weights, same fma chains in range order as the general path below: same bits.
        float ms[16], ls[16], vs[16];
#pragma unroll
        for (int sp = 0; sp < 16; ++sp) {
            const long long slot = slot_of(sp < n_split ? sp : 0);
            ms[sp] = part_ml[slot * 2];
            ls[sp] = part_ml[slot * 2 + 1];
            vs[sp] = part_o[slot * HD + d];
        }
        float m = -INFINITY;
#pragma unroll
        for (int sp = 0; sp < 16; ++sp) m = sp < n_split ? fmaxf(m, ms[sp]) : m;
        float l = 0.f, o = 0.f;
#pragma unroll
        for (int sp = 0; sp < 16; ++sp) {
            if (sp < n_split) {
                const float w = (ms[sp] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((ms[sp] - m) * p.scale_log2);
                l = fmaf(ls[sp], w, l);
                o = fmaf(vs[sp], w, o);
            }
        }
        const float y = l > 0.f ? o / l : 0.f;
        if (p.o_img_rows > 0) {
            const int RM = p.o_img_rows, k = (int)((long long)qrow * p.ld_o + (long long)hq * p.o_hs) + d;
            const long long off = (long long)(k >> 6) * (RM * 128) + ((((k >> 3) & 1) * (4 * RM) + ((k >> 4) & 3) * RM + b) << 4) + ((k & 7) << 1);
            *(CMB_AS1 T*)(p.o + off) = from_f32<T>(y);
        } else {
            CMB_AS1 T* op = (CMB_AS1 T*)p.o + (long long)b * p.o_bs + (long long)qrow * p.ld_o + (long long)hq * p.o_hs;
            op[d] = from_f32<T>(y);
        }
        return;
    }
    float m = -INFINITY;
    for (int sp = d; sp < n_split; sp += HD) m = fmaxf(m, part_ml[slot_of(sp) * 2]);
    m = wave_max(m);
    if ((d & 63) == 0) s_red[d >> 6] = m;
    __syncthreads();
    m = s_red[0];
    for (int w = 1; w < (HD >> 6); ++w) m = fmaxf(m, s_red[w]);
    float l = 0.f, o = 0.f;
    for (int base = 0; base < n_split; base += CMB_CHUNK) {
        const int n = (n_split - base) < CMB_CHUNK ? (n_split - base) : CMB_CHUNK;
        __syncthreads();                             // the previous chunk's weights have been consumed
        for (int i = d; i < n; i += HD) {
            const long long slot = slot_of(base + i);
            const float ms = part_ml[slot * 2];
            s_w[i] = (ms == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((ms - m) * p.scale_log2);
            s_l[i] = part_ml[slot * 2 + 1];
        }
        __syncthreads();
        int i = 0;
        for (; i + 8 <= n; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part_o[slot_of(base + i + u) * HD + d];
#pragma unroll
            for (int u = 0; u < 8; ++u) { l = fmaf(s_l[i + u], s_w[i + u], l); o = fmaf(v[u], s_w[i + u], o); }
        }
        for (; i < n; ++i) { l = fmaf(s_l[i], s_w[i], l); o = fmaf(part_o[slot_of(base + i) * HD + d], s_w[i], o); }
    }
    const float y = l > 0.f ? o / l : 0.f;
    if (p.o_img_rows > 0) {
        // element (row b, column k) of the image the decode step's o projection streams (img_phase.h)
        const int RM = p.o_img_rows, k = (int)((long long)qrow * p.ld_o + (long long)hq * p.o_hs) + d;
        const long long off = (long long)(k >> 6) * (RM * 128) + ((((k >> 3) & 1) * (4 * RM) + ((k >> 4) & 3) * RM + b) << 4) + ((k & 7) << 1);
        *(CMB_AS1 T*)(p.o + off) = from_f32<T>(y);
        return;
    }
    CMB_AS1 T* op = (CMB_AS1 T*)p.o + (long long)b * p.o_bs + (long long)qrow * p.ld_o + (long long)hq * p.o_hs;
    op[d] = from_f32<T>(y);
}


// ---- decode attention at head_dim 128, bf16: one new token per sequence against its KV cache (round 4) ----------------------------------
// The generic kernel above keeps the GQA group's few query rows in one wave and walks its key range as two LDS-staged tiles, the second
// requested only after the first has landed: a 10-us launch for 0.4 MB.  Here a workgroup takes the same (sequence, kv head, 128-key range)
// and the same partial format (the merge pass is unchanged), but
//   * every byte it needs -- K and V rows of its 128 keys, q, the cos / sin row -- is requested before anything is waited for;
//   * K goes straight from global memory into the A operand of v_mfma_f32_16x16x32_bf16 (lane (key, 16-byte chunk) = one 16-byte load, no
//     LDS staging, no barrier); each wave owns 32 keys: S[32 keys, 16 query slots] = 8 MFMAs;
//   * P.V runs on the vector ALU (<= 8 query rows x 8 keys x 8 columns per lane: 512 fma) on V rows loaded in their natural layout -- the
//     matrix pipe would want V transposed, which is what the LDS round trip of the generic kernel is for;
//   * the four waves' partial softmaxes (and the four key quarters inside a wave) meet once, through LDS, in fixed order.
// Fused RoPE + KV append as in attn_kernel (same rope_mad, same bits in the cache).  Masked key slots re-read the last live row and their V is
// forced to zero, so nothing behind the context -- uninitialised cache, the row being appended -- can reach the output.
// the kernel arguments go through an opaque scalar copy (below); these put the global address space back on what is loaded through them
#define DL_AS1 __attribute__((address_space(1)))
__device__ __forceinline__ u32x4 ldg16(const void* q) { return *(const DL_AS1 u32x4*)q; }
__device__ __forceinline__ void stg16(void* q, u32x4 v) { *(DL_AS1 u32x4*)q = v; }
constexpr int DL_REP = 8;                                   // query rows (GQA group size) this form holds
constexpr int DL_LDS_P = 4 * 64 * 8 * 4;                    // P of each wave: [key quarter][query slot][8 keys] f32
constexpr int DL_LDS_O = 16 * DL_REP * 128 * 4;             // partial O: [wave][key quarter][query][128] f32
constexpr int DL_LDS = DL_LDS_P + DL_LDS_O + 4 * DL_REP * 2 * 4;
#ifdef AFHIP_ATTN_STAMPS   /* diagnostic build (tools/decode_attn_stamps.py): 100-MHz wall clock of wave 0 of every workgroup */
#define DL_STAMP(k) do { if (p.dbg && tid == 0) ((DL_AS1 unsigned long long*)p.dbg)[(long long)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define DL_STAMP(k) do { } while (0)
#endif
__global__ __launch_bounds__(256) void attn_decode128_kernel(AttnP p_in) {
    // every kernel argument this launch reads, fetched in ONE batch: left to itself the compiler loads the fields where they are first needed,
    // five dependent scalar round trips (0.3-0.5 us each) before the first K row is requested
    AttnP p = p_in;
    asm volatile("" : "+s"(p.q), "+s"(p.k), "+s"(p.v), "+s"(p.B), "+s"(p.Tq), "+s"(p.Tk), "+s"(p.n_q), "+s"(p.ld_q), "+s"(p.ld_kv),
                 "+s"(p.q_bs), "+s"(p.kv_bs), "+s"(p.q_hs), "+s"(p.kv_hs), "+s"(p.scale_log2), "+s"(p.n_xt), "+s"(p.key_split));
    asm volatile("" : "+s"(p.part_o), "+s"(p.part_ml), "+s"(p.new_k), "+s"(p.new_v), "+s"(p.new_kv_bs), "+s"(p.rope_cos), "+s"(p.rope_sin),
                 "+s"(p.seq_pos), "+s"(p.dbg));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    DL_STAMP(0);
    const int nh = p.n_q * p.B;
    int xt, hb;
    if ((nh & 7) == 0) {                                    // same XCD-aware order as attn_kernel: the ranges of one (sequence, head) share an L2
        const int xcd = blockIdx.x & 7, r = blockIdx.x >> 3;
        xt = r % p.n_xt;
        hb = (r / p.n_xt) * 8 + xcd;
    } else {
        xt = blockIdx.x % p.n_xt;
        hb = blockIdx.x / p.n_xt;
    }
    const int b = hb / p.n_q, hkv = hb % p.n_q;
    const int rep = p.Tq;
    int klen = p.Tk;
    if (p.seq_pos) { const int tk = ((const DL_AS1 int32_t*)p.seq_pos)[b] + 1; klen = tk < klen ? tk : klen; }
    const int tk_b = klen;
    const int kbeg = xt * p.key_split;
    const int kend = (kbeg + p.key_split) < klen ? (kbeg + p.key_split) : klen;
    if (kbeg >= kend) return;                               // range beyond this sequence's context (the merge derives the live ranges the same way)
    DL_STAMP(1);
    const char* qb = p.q + ((long long)b * p.q_bs + (long long)hkv * p.q_hs) * 2;
    const char* kb = p.k + ((long long)b * p.kv_bs + (long long)hkv * p.kv_hs) * 2;
    const char* vb = p.v + ((long long)b * p.kv_bs + (long long)hkv * p.kv_hs) * 2;
    const unsigned rowb = (unsigned)(p.ld_kv * 2);          // one (sequence, head)'s cache is far below 4 GiB (host check): 32-bit offsets inside it
    const float* rope_cos = p.rope_cos;
    const float* rope_sin = p.rope_sin;
    if (p.seq_pos && p.new_k) { rope_cos += (long long)(tk_b - 1) * 64; rope_sin += (long long)(tk_b - 1) * 64; }
    const int wk0 = kbeg + 32 * wave;                       // this wave's 32 keys
    const bool fused = p.new_k != nullptr;
    const char* nk = fused ? p.new_k + ((long long)b * p.new_kv_bs + (long long)hkv * 128) * 2 : nullptr;
    const char* nv = fused ? p.new_v + ((long long)b * p.new_kv_bs + (long long)hkv * 128) * 2 : nullptr;

    // ---- every load of the launch ----
    u32x4 kf[2][4], vf[8], qf[4];
    f32x4 cs[2][2], sn[2][2];                               // cos / sin of rotation pairs 32 s + 8 g .. + 8 (s = 0, 1)
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int key = wk0 + 16 * blk + c;
        const int kc = key < klen ? key : klen - 1;
        const char* row = (fused && key == tk_b - 1) ? nk : kb + (unsigned)kc * rowb;
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[blk][s] = ldg16(row + (4 * s + g) * 16);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int key = wk0 + 16 * (k >> 2) + 4 * g + (k & 3);
        const int kc = key < klen ? key : klen - 1;
        const char* row = (fused && key == tk_b - 1) ? nv : vb + (unsigned)kc * rowb;
        vf[k] = ldg16(row + c * 16);
    }
    {
        const int j = c < rep ? c : rep - 1;
        const char* qrow = qb + (long long)j * p.ld_q * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = ldg16(qrow + (4 * s + g) * 16);
    }
    if (fused) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                cs[s][h] = *(const DL_AS1 f32x4*)(rope_cos + 32 * s + 8 * g + 4 * h);
                sn[s][h] = *(const DL_AS1 f32x4*)(rope_sin + 32 * s + 8 * g + 4 * h);
            }
        // rotate-half RoPE: element d = 32 s + 8 g + e (s = 0, 1) pairs with d + 64 = k-step s + 2 of the SAME lane.  q cos + rotate_half(q) sin
        // with separate roundings, then bf16 -- exactly rope_kv_kernel (norm.hip) and attn_kernel
        auto rotate = [&](u32x4 (&x)[4]) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16 lo[8], hi[8];
                *reinterpret_cast<u32x4*>(lo) = x[s];
                *reinterpret_cast<u32x4*>(hi) = x[s + 2];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float cc = cs[s][e >> 2][e & 3], ss = sn[s][e >> 2][e & 3];
                    const float x1 = (float)lo[e], x2 = (float)hi[e];
                    lo[e] = (bf16)rope_mad(x1, cc, -x2, ss);
                    hi[e] = (bf16)rope_mad(x2, cc, x1, ss);
                }
                x[s] = *reinterpret_cast<const u32x4*>(lo);
                x[s + 2] = *reinterpret_cast<const u32x4*>(hi);
            }
        };
        rotate(qf);
        // the token being generated: its k is rotated here, and k, v are written to the cache for the following steps (only the lanes of the
        // one workgroup whose range holds position tk_b - 1 get here)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int key = wk0 + 16 * blk + c;
            if (key == tk_b - 1) {
                rotate(kf[blk]);
#pragma unroll
                for (int s = 0; s < 4; ++s) stg16(const_cast<char*>(kb) + (unsigned)key * rowb + (4 * s + g) * 16, kf[blk][s]);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int key = wk0 + 16 * (k >> 2) + 4 * g + (k & 3);
            if (key == tk_b - 1) stg16(const_cast<char*>(vb) + (unsigned)key * rowb + c * 16, vf[k]);
        }
    }

    DL_STAMP(2);
    // ---- S[key, query slot] for this wave's 32 keys ----
    f32x4 sacc[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        sacc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[blk][s]), __builtin_bit_cast(bf16x8, qf[s]), sacc[blk], 0, 0, 0);
    }
    // lane (g, c) holds, for query slot c, the scores of keys wk0 + 16 blk + 4 g + r: the same 8 keys whose V rows lane group g loaded
    float sv[8], pv[8];
#ifdef AFHIP_ATTN_STAMPS
    { float t_ = sacc[0][0] + sacc[1][0]; asm volatile("" :: "v"(t_)); }
    DL_STAMP(3);
#endif
    bool ok[8];
    float mloc = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int key = wk0 + 16 * (k >> 2) + 4 * g + (k & 3);
        ok[k] = key < kend;
        sv[k] = sacc[k >> 2][k & 3];
        mloc = ok[k] ? fmaxf(mloc, sv[k]) : mloc;
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float m_use = (mloc == -INFINITY) ? 0.f : mloc;
    const float moff = -m_use * p.scale_log2;
    float lsum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        pv[k] = ok[k] ? __builtin_amdgcn_exp2f(fmaf(sv[k], p.scale_log2, moff)) : 0.f;
        lsum += pv[k];
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    float* Pw = reinterpret_cast<float*>(smem) + wave * 512;
    *reinterpret_cast<f32x4*>(Pw + (g * 16 + c) * 8) = f32x4{pv[0], pv[1], pv[2], pv[3]};
    *reinterpret_cast<f32x4*>(Pw + (g * 16 + c) * 8 + 4) = f32x4{pv[4], pv[5], pv[6], pv[7]};

    // ---- O[query, 8 c .. 8 c + 8] over this lane's 8 keys ----
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    f32x2_t vv[8][4];                                       // column pairs: the fma below is v_pk_fma_f32
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t w = ok[k] ? vf[k][e] : 0u;       // two bf16: widening is a shift / a mask
            vv[k][e] = f32x2_t{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
        }
    DL_STAMP(4);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's P tile is in LDS (one wave: no barrier)
    __builtin_amdgcn_wave_barrier();
    float* Op = reinterpret_cast<float*>(smem + DL_LDS_P);
    float* ML = reinterpret_cast<float*>(smem + DL_LDS_P + DL_LDS_O);
#pragma unroll
    for (int q = 0; q < DL_REP; ++q) {
        if (q < rep) {
            const f32x4 p0 = *reinterpret_cast<const f32x4*>(Pw + (g * 16 + q) * 8), p1 = *reinterpret_cast<const f32x4*>(Pw + (g * 16 + q) * 8 + 4);
            const float pq[8] = {p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
            f32x2_t o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f32x2_t{0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = __builtin_elementwise_fma(f32x2_t{pq[k], pq[k]}, vv[k][e], o[e]);
            float* dst = Op + (((wave * 4 + g) * DL_REP + q) * 128 + 8 * c);
            *reinterpret_cast<f32x4*>(dst) = f32x4{o[0][0], o[0][1], o[1][0], o[1][1]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[2][0], o[2][1], o[3][0], o[3][1]};
        }
    }
    if (g == 0 && c < DL_REP) { ML[(wave * DL_REP + c) * 2] = mloc; ML[(wave * DL_REP + c) * 2 + 1] = lsum; }
    DL_STAMP(5);
    __syncthreads();
    DL_STAMP(6);

    // ---- the four waves meet: same weights, same order for every output column ----
    for (int idx = tid; idx < rep * 128; idx += 256) {
        const int q = idx >> 7, d = idx & 127;
        float mw[4], mt = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) { mw[w] = ML[(w * DL_REP + q) * 2]; mt = fmaxf(mt, mw[w]); }
        float acc = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float al = (mw[w] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mw[w] - mt) * p.scale_log2);
            const float* src = Op + ((w * 4) * DL_REP + q) * 128 + d;
            const float sw = ((src[0] + src[DL_REP * 128]) + src[2 * DL_REP * 128]) + src[3 * DL_REP * 128];
            acc = fmaf(sw, al, acc);
            l = fmaf(ML[(w * DL_REP + q) * 2 + 1], al, l);
        }
        const long long slot = (((long long)xt * p.B + b) * p.n_q + hkv) * 32 + q;
        ((DL_AS1 float*)p.part_o)[slot * 128 + d] = acc;
        if (d == 0) { ((DL_AS1 float*)p.part_ml)[slot * 2] = mt; ((DL_AS1 float*)p.part_ml)[slot * 2 + 1] = l; }
    }
    DL_STAMP(7);
}

}  // namespace

bool afhip_attention_enc64(const afhip_attn_args* a, hipStream_t s);   // attention_enc.hip: the one-wave-per-SIMD encoder form
bool afhip_attention_enc64_applies(const afhip_attn_args* a);

namespace {
// the lagged-maximum softmax form of attn_kernel (encoder, LayerNorm-folded mode)
bool attn_lag_form(const afhip_attn_args* a) {
    return a->dtype == AFHIP_BF16 && a->hd == 64 && a->q_prescaled && a->key_split == 0 && afhip_opt(AFHIP_OPT_ATTN_NBUF) != 1 &&
           afhip_opt(AFHIP_OPT_ATTN_LAG) != 0;
}
}  // namespace

// which kernel afhip_attention(a) runs for a non-decode shape: the predicates it dispatches on (common.h)
int afhip_attention_form(const afhip_attn_args* a) {
    if (afhip_attention_enc64_applies(a)) return AFHIP_ENC_ATTN_ENC64;
    return attn_lag_form(a) ? AFHIP_ENC_ATTN_LAG : 0;
}

extern "C" int afhip_attention(const afhip_attn_args* a, void* stream) {
    AFHIP_CHECK(a != nullptr, "afhip_attention: null args");
    AFHIP_CHECK(a->dtype == AFHIP_F32 || a->dtype == AFHIP_BF16, "afhip_attention: bad dtype %d", a->dtype);
    AFHIP_CHECK(a->q && a->k && a->v && a->out, "afhip_attention: null tensor");
    AFHIP_CHECK(a->B > 0 && a->Tq > 0 && a->Tk > 0 && a->n_q > 0 && a->n_kv > 0 && a->n_q % a->n_kv == 0,
                "afhip_attention: bad shape B=%d Tq=%d Tk=%d n_q=%d n_kv=%d", a->B, a->Tq, a->Tk, a->n_q, a->n_kv);
    AFHIP_CHECK(a->hd == 64 || a->hd == 128, "afhip_attention: head_dim %d unsupported (64 or 128)", a->hd);
    const size_t sz = dtype_size(a->dtype);
    AFHIP_CHECK(((uintptr_t)a->q % 16) == 0 && ((uintptr_t)a->k % 16) == 0 && ((uintptr_t)a->v % 16) == 0 && ((uintptr_t)a->out % 16) == 0,
                "afhip_attention: tensors must be 16-byte aligned");
    AFHIP_CHECK((a->ld_q * sz) % 16 == 0 && (a->ld_kv * sz) % 16 == 0 && (a->ld_o * sz) % 16 == 0 &&
                    (a->q_head_stride * sz) % 16 == 0 && (a->kv_head_stride * sz) % 16 == 0 &&
                    (a->q_batch_stride * sz) % 16 == 0 && (a->kv_batch_stride * sz) % 16 == 0 && (a->o_batch_stride * sz) % 16 == 0,
                "afhip_attention: strides must keep 16-byte alignment");
    AFHIP_CHECK(a->ld_o >= a->hd, "afhip_attention: ld_o too small");
    if (a->causal) AFHIP_CHECK(a->q_pos0 >= 0 && a->q_pos0 + a->Tq <= a->Tk, "afhip_attention: causal needs q_pos0+Tq <= Tk (%d+%d vs %d)", a->q_pos0, a->Tq, a->Tk);

    if (a->row_off) AFHIP_CHECK(a->key_split == 0 && !a->causal && a->key_len && a->Tq == a->Tk, "afhip_attention: row_off (packed batches) needs key_len, Tq == Tk, no causal mask, no key_split");
    {
        const int slot = afhip_prof_begin((hipStream_t)stream);
        if (afhip_attention_enc64(a, (hipStream_t)stream)) {
            // the roofline leg of bench.py quotes this kernel as it is paid inside the timed step (4 Tq Tk hd flops per head and clip)
            afhip_prof_end(slot, (hipStream_t)stream, 4.0 * a->Tq * (double)a->Tk * a->hd * a->n_q * a->B, AFHIP_PROF_ATTN);
            AFHIP_LAUNCH_CHECK();
            return 0;
        }
    }
    AFHIP_CHECK(!a->out_fp8, "afhip_attention: out_fp8 is a feature of the encoder form (bf16, head_dim 64, q_prescaled, non-causal, no key split)");

    AttnP p;
    p.q = (const char*)a->q; p.k = (const char*)a->k; p.v = (const char*)a->v; p.o = (char*)a->out;
    p.key_len = a->key_len;
    p.B = a->B; p.Tq = a->Tq; p.Tk = a->Tk; p.n_q = a->n_q; p.n_kv = a->n_kv; p.hd = a->hd;
    p.ld_q = a->ld_q; p.ld_kv = a->ld_kv; p.ld_o = a->ld_o;
    p.q_bs = a->q_batch_stride; p.kv_bs = a->kv_batch_stride; p.o_bs = a->o_batch_stride;
    p.q_hs = a->q_head_stride; p.kv_hs = a->kv_head_stride; p.o_hs = a->o_head_stride > 0 ? a->o_head_stride : a->hd;
    p.causal = a->causal; p.q_pos0 = a->q_pos0;
    p.scale_log2 = a->q_prescaled ? 1.0f : a->scale * 1.4426950408889634f;
    hipStream_t s = (hipStream_t)stream;
    // key-range splitting for tiny query counts (decode): partials + a combine pass
    int n_split = 1;
    p.key_split = 0; p.part_o = nullptr; p.part_ml = nullptr;
    p.new_k = (const char*)a->new_k; p.new_v = (const char*)a->new_v; p.new_kv_bs = a->new_kv_batch_stride;
    p.rope_cos = a->rope_cos; p.rope_sin = a->rope_sin;
    p.ticket = a->key_split > 0 ? a->split_ticket : nullptr;
    p.seq_pos = a->seq_pos;
    p.row_off = a->row_off;
    p.o_img_rows = a->out_img_rows;
    if (a->out_img_rows) AFHIP_CHECK(a->key_split > 0 && a->split_ticket == nullptr && a->dtype == AFHIP_BF16 && (a->out_img_rows == 8 || a->out_img_rows == 16) && a->B <= a->out_img_rows,
                                     "afhip_attention: out_img_rows (8 or 16, >= B) is a feature of the bf16 split-context (decode) form");
    if (a->row_off) AFHIP_CHECK(a->key_split == 0 && !a->causal && a->key_len && a->Tq == a->Tk, "afhip_attention: row_off (packed batches) needs key_len, Tq == Tk, no causal mask, no key_split");
    if (a->seq_pos) AFHIP_CHECK(a->key_split > 0, "afhip_attention: seq_pos needs the split-context (decode) form, key_split > 0");
    if (a->new_k) {
        AFHIP_CHECK(a->key_split > 0 && a->new_v && a->rope_cos && a->rope_sin, "afhip_attention: fused RoPE/append needs key_split > 0, new_v and the cos/sin rows");
        AFHIP_CHECK(((uintptr_t)a->new_k % 16) == 0 && ((uintptr_t)a->new_v % 16) == 0 && (a->new_kv_batch_stride * sz) % 16 == 0, "afhip_attention: new_k / new_v must keep 16-byte alignment");
    }
#ifdef AFHIP_ATTN_STAMPS   /* diagnostic build only (tools/attn_stamps.py) */
    { const char* dp = getenv("AFHIP_ATTN_DBGPTR"); p.dbg = dp ? (unsigned long long*)strtoull(dp, nullptr, 0) : nullptr; }
#else
    p.dbg = nullptr;
#endif
    if (a->key_split > 0) {
        AFHIP_CHECK(a->key_split % KT == 0, "afhip_attention: key_split must be a multiple of %d", KT);
        AFHIP_CHECK(a->Tq <= 32 && !a->causal, "afhip_attention: key_split needs Tq <= 32 and causal == 0");
        n_split = cdiv(a->Tk, a->key_split);
        const size_t need = (size_t)n_split * a->B * a->n_q * 32 * (a->hd + 2) * sizeof(float);
        AFHIP_CHECK(a->partial_ws != nullptr && a->partial_ws_bytes >= need, "afhip_attention: partial workspace %zu < %zu bytes", (size_t)a->partial_ws_bytes, need);
        AFHIP_CHECK(((uintptr_t)a->partial_ws % 16) == 0, "afhip_attention: partial workspace must be 16-byte aligned");
        p.key_split = a->key_split;
        p.part_o = (float*)a->partial_ws;
        p.part_ml = p.part_o + (size_t)n_split * a->B * a->n_q * 32 * a->hd;
    }
    p.n_xt = a->key_split > 0 ? n_split : cdiv(a->Tq, QT);
    AFHIP_CHECK((long long)p.n_xt * a->n_q * a->B < (1ll << 31), "afhip_attention: grid too large");
    const dim3 grid((unsigned)(p.n_xt * a->n_q * a->B)), block(256);
    const int nbuf = afhip_opt(AFHIP_OPT_ATTN_NBUF) == 1 ? 1 : 2;   // A/B switch
    size_t lds = (size_t)nbuf * 2 * KT * a->hd * sz;     // stages of (K tile + V tile)
    lds += (size_t)(afhip_opt(AFHIP_OPT_ATTN_LDS_PAD) > 0 ? afhip_opt(AFHIP_OPT_ATTN_LDS_PAD) : 0);   // occupancy experiment
    {
        static unsigned long long attr_done = 0;
        if (afhip_first_use_on_device(&attr_done)) {
            (void)hipFuncSetAttribute((const void*)attn_kernel<bf16, 128, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * KT * 128 * 2);
            (void)hipFuncSetAttribute((const void*)attn_kernel<bf16, 64, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            (void)hipFuncSetAttribute((const void*)attn_kernel<bf16, 64, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            (void)hipFuncSetAttribute((const void*)attn_kernel<float, 64, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * KT * 64 * 4);
            (void)hipFuncSetAttribute((const void*)attn_kernel<float, 128, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * KT * 128 * 4);
        }
    }
    // decode at head_dim 128, bf16, a GQA group of at most 8 query rows, ranges of at most 128 keys: the lean form (same partials, same merge)
    const bool lean = a->dtype == AFHIP_BF16 && a->hd == 128 && a->key_split > 0 && a->key_split <= 128 && a->Tq <= DL_REP && !a->causal &&
                      a->key_len == nullptr && a->row_off == nullptr && a->split_ticket == nullptr && a->n_q == a->n_kv &&
                      afhip_opt(AFHIP_OPT_DECODE_LEAN) != 0;
    if (lean) {
        static unsigned long long lean_attr = 0;
        if (afhip_first_use_on_device(&lean_attr))
            (void)hipFuncSetAttribute((const void*)attn_decode128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DL_LDS);
        hipLaunchKernelGGL(attn_decode128_kernel, grid, block, DL_LDS, s, p);
    } else {
#define AFHIP_ATTN_LAUNCH(TT, HH)                                                                          \
    do {                                                                                                   \
        if (nbuf == 2) hipLaunchKernelGGL((attn_kernel<TT, HH, 2>), grid, block, lds, s, p);             \
        else hipLaunchKernelGGL((attn_kernel<TT, HH, 1>), grid, block, lds, s, p);                        \
    } while (0)
    if (attn_lag_form(a)) {                                                                 // A/B switch ATTN_LAG
        hipLaunchKernelGGL((attn_kernel<bf16, 64, 2, true>), grid, block, lds, s, p);      // lagged-maximum softmax (encoder, LayerNorm-folded mode)
    } else if (a->dtype == AFHIP_BF16) {
        if (a->hd == 64) AFHIP_ATTN_LAUNCH(bf16, 64); else AFHIP_ATTN_LAUNCH(bf16, 128);
    } else {
        if (a->hd == 64) AFHIP_ATTN_LAUNCH(float, 64); else AFHIP_ATTN_LAUNCH(float, 128);
    }
    }
#undef AFHIP_ATTN_LAUNCH
    AFHIP_LAUNCH_CHECK();
    if (a->key_split > 0 && a->split_ticket == nullptr) {
        const dim3 g2(a->B * a->n_q * a->Tq), b2(a->hd);
        if (a->dtype == AFHIP_BF16) hipLaunchKernelGGL(attn_combine_kernel<bf16>, g2, b2, 0, s, p, n_split, a->hd);
        else hipLaunchKernelGGL(attn_combine_kernel<float>, g2, b2, 0, s, p, n_split, a->hd);
        AFHIP_LAUNCH_CHECK();
    }
    return 0;
}
