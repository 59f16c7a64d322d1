// Band-limited rational-ratio resampler (fp32) in front of the log-mel: the GPU form of the librosa.resample call in
// ContinuousAudioIO.preprocess (multimodal_io/audio.py:1031-1034).  Filter, sample convention and table layout: include/afhip.h.
//
// The polyphase sum y[m] = sum_t x[q(m) - K + t] H[p(m)][t] is a banded GEMM.  With P = 16 / gcd(L, 16) periods of the ratio per
// "super-period" (L' = P L outputs, M' = P M inputs, L' a multiple of 16), output m = J L' + c reads the inputs from J M' + D_c - K on,
// D_c = floor(c M / L), p = (c M) mod L.  For the 16 outputs c0..c0+15 of one column tile and a row J:
//     y[J L' + c] = sum_n A[J][n] B[n][c],   A[J][n] = x[J M' + D_c0 - K + n],   B[n][c] = H[p_c][n - (D_c - D_c0)] (0 outside the row)
// -- rows J are super-periods, columns the 16 phases of the tile, n runs over the tile's band (T_pad + D_c0+15 - D_c0 values; ~10 %
// of it multiplies the zeros outside each column's own taps).  One wave owns one column tile and 64 rows: four 16x16 accumulators of
// v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain) share each B fragment, so per 16 band values a lane loads 4 A + 1 B runs
// of 16 bytes for 16 MFMAs (1024 FMA each) -- the operand supply a VALU form (one coefficient per FMA: consecutive outputs change phase)
// could not get from LDS.  Both operands come straight from global memory through buffer loads: x with the clip's valid length as the
// range (outside -> 0, the zero extension of the convention), the table with an explicit out-of-row test -> 0.  Nothing is staged in
// LDS, so the table may be any size (400 KB at 11.025 kHz).
//
// The order of every output's sum depends only on c = m mod L' (the tile's band start is fixed per column tile), never on m0, the
// row group or the batch: windows cut from one clip with an input shift of a multiple of M' and m0 shifted by the same multiple of
// L' are bit-identical to the whole clip's outputs (long_audio.py relies on it).
#include "common.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

namespace {

constexpr int RS_MAX_RATE = 384000;
constexpr int RS_MAX_L = 1024;
constexpr int RS_MAX_TPAD = 16384;      // 2K+1 <= 16381: rates as low as ~2 kHz on the low side of a pair (8 kHz: 159 taps at 8 kHz)
constexpr int RS_MAX_ROW = 1 << 28;     // samples per input row: byte offsets stay inside int32 with the band added
constexpr int RS_ROWS = 64;             // rows (super-periods) per wave: 4 MFMA row tiles

struct RsPlan {
    int L, M, K, T, T_pad, P, Lp;
    long long Mp;
};

long long gcd_ll(long long a, long long b) {
    while (b) { long long t = a % b; a = b; b = t; }
    return a;
}

struct RsFilter {
    double fc, beta, Th, fs_in, i0b;
};

double bessel_i0(double x) {
    // power series sum (x/2)^(2k) / (k!)^2: terms fall below 1e-17 of the sum for beta <= 11 well before k = 60
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// the formula of the header: Kaiser-windowed sinc, cutoff 0.955 f_min/2, transition 0.09 f_min/2, 110 dB
int rs_plan(int fs_in, int fs_out, RsPlan* pl, RsFilter* f) {
    AFHIP_CHECK(fs_in > 0 && fs_out > 0 && fs_in <= RS_MAX_RATE && fs_out <= RS_MAX_RATE,
                "afhip_resample: rates %d -> %d must be integers in [1, %d]", fs_in, fs_out, RS_MAX_RATE);
    const long long g = gcd_ll(fs_in, fs_out);
    const int L = (int)(fs_out / g), M = (int)(fs_in / g);
    AFHIP_CHECK(L <= RS_MAX_L, "afhip_resample: %d -> %d reduces to L = %d up-sampling phases (> %d)", fs_in, fs_out, L, RS_MAX_L);
    const double A = 110.0, fmin = (double)(fs_in < fs_out ? fs_in : fs_out);
    const double fc = 0.955 * fmin / 2.0, delta = 0.09 * fmin / 2.0;
    const double Th = (A - 7.95) / (4.57 * 2.0 * M_PI * delta);
    const double Kd = ceil(Th * (double)fs_in);
    AFHIP_CHECK(2.0 * Kd + 1.0 <= RS_MAX_TPAD - 3, "afhip_resample: %d -> %d needs %.0f taps per output (> %d)", fs_in, fs_out, 2.0 * Kd + 1.0,
                RS_MAX_TPAD - 3);
    pl->L = L; pl->M = M; pl->K = (int)Kd;
    pl->T = 2 * pl->K + 1;
    pl->T_pad = (pl->T + 3) & ~3;
    pl->P = 16 / (int)gcd_ll(L, 16);
    pl->Lp = pl->P * L;
    pl->Mp = (long long)pl->P * M;
    if (f) {
        f->fc = fc; f->beta = 0.1102 * (A - 8.7); f->Th = Th; f->fs_in = (double)fs_in;
        f->i0b = bessel_i0(f->beta);
    }
    return 0;
}

struct RsArgs {
    const float* x; long long x_stride; const int* n_in;
    float* y; long long y_stride;
    const float* H; int T_pad;
    int L, M, K, Lp; long long Mp;
    long long m0; int n_out_max;
    long long J_lo; int n_rg, n_ct, B;
};

// the builtin returns the dword as an integer: reinterpret it (an assignment to float would convert its value)
__device__ __forceinline__ float rs_ld(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

__global__ __launch_bounds__(256) void resample_kernel(RsArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ct = (int)(w % a.n_ct);
    const long long rest = w / a.n_ct;
    const int rg = (int)(rest % a.n_rg);
    const int b = __builtin_amdgcn_readfirstlane((int)(rest / a.n_rg));
    if (b >= a.B) return;

    // the clip's valid length, held to its row (a longer length would read the next row)
    int n_in = a.n_in[b];
    n_in = n_in < 0 ? 0 : (n_in > a.x_stride ? (int)a.x_stride : n_in);
    n_in = __builtin_amdgcn_readfirstlane(n_in);
    const long long n_out_b = ((long long)n_in * a.L + a.M - 1) / a.M;

    const int col = lane & 15, kk = lane >> 4;
    const int c0 = ct * 16, c = c0 + col;
    const long long D_c0 = (long long)c0 * a.M / a.L;
    const int e_c = (int)((long long)c * a.M / a.L - D_c0);                  // this column's tap offset inside the band
    const int p_c = (int)(((long long)c * a.M) % a.L);
    const int e_last = (int)((long long)(c0 + 15) * a.M / a.L - D_c0);
    const int n_chunks = (e_last + a.T_pad + 15) >> 4;
    const long long J0 = a.J_lo + (long long)rg * RS_ROWS;

    float* yb = a.y + (long long)b * a.y_stride;
    const long long m_first = J0 * a.Lp + c0;
    f32x4 acc[4] = {};
    if (m_first < n_out_b) {
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (long long)b * a.x_stride), 0, n_in * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t hr = __builtin_amdgcn_make_buffer_rsrc((void*)a.H, 0, a.L * a.T_pad * 4, 0x00020000);
        // A rows of this lane (row = lane & 15 of each row tile), as input indices; starts clamped to +-2^28 keep every index of the band an
        // int32 that is still outside [0, n_in), so a row wholly outside the clip reads zeros
        int xo[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            long long s = (J0 + rt * 16 + col) * a.Mp + D_c0 - a.K + 4 * kk;
            s = s < -(1ll << 28) ? -(1ll << 28) : (s > (1ll << 28) ? (1ll << 28) : s);
            xo[rt] = (int)s;
        }
        const int hrow = p_c * a.T_pad, tap0 = 4 * kk - e_c;
        // chunk of 16 band values: lane k-group kk holds n = 16 ch + 4 kk + s for MFMA s = 0..3 (k order of the chain: kk within one MFMA)
        float av[2][4][4], bv[2][4];
        // four consecutive dwords from index i of a range [0, lim): one 16-byte load when all four are inside (the common case: 16
        // lanes of a row tile then read 256 contiguous bytes), else one dword load per element with its own range test -- the result never
        // hangs on how the hardware range-checks a multi-dword access that straddles the range's end
        auto ld4 = [](__amdgpu_buffer_rsrc_t r, int base, int i, int lim, float (&v)[4]) {
            if (i >= 0 && i <= lim - 4) {
                const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (base + i) * 4, 0, 0));
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) v[s] = rs_ld(r, (unsigned)(i + s) < (unsigned)lim ? (base + i + s) * 4 : -4);
            }
        };
        auto load = [&](int ch, float (&A)[4][4], float (&Bv)[4]) {
            ld4(hr, hrow, ch * 16 + tap0, a.T_pad, Bv);
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) ld4(xr, 0, xo[rt] + ch * 16, n_in, A[rt]);
        };
        load(0, av[0], bv[0]);
        for (int ch = 0; ch < n_chunks; ch += 2) {
            if (ch + 1 < n_chunks) load(ch + 1, av[1], bv[1]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0][rt][s], bv[0][s], acc[rt], 0, 0, 0);
            if (ch + 1 >= n_chunks) break;
            if (ch + 2 < n_chunks) load(ch + 2, av[0], bv[0]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1][rt][s], bv[1][s], acc[rt], 0, 0, 0);
        }
    }
    // D[row = 4 kk + v][col] of row tile rt is output m = (J0 + 16 rt + 4 kk + v) L' + c; positions past the clip's n_out are exact zeros
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long long m = (J0 + rt * 16 + 4 * kk + v) * a.Lp + c;
            const long long o = m - a.m0;
            if (o >= 0 && o < a.n_out_max) yb[o] = m < n_out_b ? acc[rt][v] : 0.f;
        }
}

}  // namespace

extern "C" int afhip_resample_plan(int fs_in, int fs_out, int* L, int* M, int* K, int* T_pad) {
    AFHIP_CHECK(L && M && K && T_pad, "afhip_resample_plan: null pointer");
    RsPlan pl;
    const int rc = rs_plan(fs_in, fs_out, &pl, nullptr);
    if (rc) return rc;
    *L = pl.L; *M = pl.M; *K = pl.K; *T_pad = pl.T_pad;
    return 0;
}

// [L][T_pad] f32, row p = phase p/L: H[p][k + K] = h((p/L - k) / fs_in), k = -K..K, zeros after 2K+1; built in double, rounded once
extern "C" int afhip_resample_tables_host(int fs_in, int fs_out, void* host_buf) {
    AFHIP_CHECK(host_buf, "afhip_resample_tables_host: null pointer");
    RsPlan pl;
    RsFilter f;
    const int rc = rs_plan(fs_in, fs_out, &pl, &f);
    if (rc) return rc;
    float* H = reinterpret_cast<float*>(host_buf);
    memset(H, 0, sizeof(float) * (size_t)pl.L * pl.T_pad);
    for (int p = 0; p < pl.L; ++p)
        for (int j = 0; j < pl.T; ++j) {
            const double tau = ((double)p / pl.L - (double)(j - pl.K)) / f.fs_in;
            const double r = tau / f.Th;
            if (fabs(r) > 1.0) continue;
            const double arg = 2.0 * f.fc * tau;
            const double sinc = arg == 0.0 ? 1.0 : sin(M_PI * arg) / (M_PI * arg);
            const double win = bessel_i0(f.beta * sqrt(1.0 - r * r)) / f.i0b;
            H[(size_t)p * pl.T_pad + j] = (float)((2.0 * f.fc / f.fs_in) * sinc * win);
        }
    return 0;
}

extern "C" int afhip_resample(const float* x, int B, const int32_t* n_in, long long x_stride, float* y, long long m0, int n_out_max,
                              long long y_stride, int fs_in, int fs_out, const float* tables, void* stream) {
    AFHIP_CHECK(x && n_in && y && tables, "afhip_resample: null pointer");
    AFHIP_CHECK(B > 0 && B <= 65535, "afhip_resample: bad batch %d", B);
    AFHIP_CHECK(x_stride > 0 && x_stride <= RS_MAX_ROW, "afhip_resample: x_stride %lld must be in [1, %d]", x_stride, RS_MAX_ROW);
    AFHIP_CHECK(n_out_max > 0, "afhip_resample: n_out_max %d must be positive", n_out_max);
    AFHIP_CHECK(B == 1 || y_stride >= n_out_max, "afhip_resample: y_stride %lld < n_out_max %d", y_stride, n_out_max);
    AFHIP_CHECK(m0 >= 0 && m0 <= (1ll << 40), "afhip_resample: m0 %lld out of range", m0);
    RsPlan pl;
    const int rc = rs_plan(fs_in, fs_out, &pl, nullptr);
    if (rc) return rc;
    RsArgs a;
    a.x = x; a.x_stride = x_stride; a.n_in = n_in; a.y = y; a.y_stride = y_stride; a.H = tables; a.T_pad = pl.T_pad;
    a.L = pl.L; a.M = pl.M; a.K = pl.K; a.Lp = pl.Lp; a.Mp = pl.Mp; a.m0 = m0; a.n_out_max = n_out_max; a.B = B;
    a.J_lo = m0 / pl.Lp;
    const long long n_J = (m0 + n_out_max - 1) / pl.Lp - a.J_lo + 1;
    a.n_rg = (int)((n_J + RS_ROWS - 1) / RS_ROWS);
    a.n_ct = pl.Lp / 16;
    const long long waves = (long long)B * a.n_rg * a.n_ct;
    AFHIP_CHECK(waves <= (1ll << 33), "afhip_resample: grid too large");
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    AFHIP_LAUNCH_CHECK();
    return 0;
}
