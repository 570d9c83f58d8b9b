// Front and back end of the Whisper units encoder (reference encoder/whisper/audio.py:62-82, model.py:35-40,121-131):
//   logmel_power_kernel   audio -> log10 of the mel power spectrum, plus one partial maximum per workgroup
//   logmel_finish_kernel  the per-clip dynamic-range floor and the affine map, stored as conv1's K4P input or as a plain tensor
//   whisper_pos_kernel    x += sinusoid table (after conv2) and the LayerNorm partials block 0's attn_ln reads
//   whisper_ln_post_kernel  ln_post over K4P rows, stored frame-major [B][T][C] with zero rows beyond a clip's length
//
// The framed DFT is a product of the frames with a windowed cos / sin basis.  It is launch- and memory-bound (1.1 GFLOP per 30 s
// clip), so the structure is chosen for accuracy: the basis is kept in double ([400][201] (cos, sin) pairs, window folded in) and the
// 400-term sums run as double FMAs, which makes a product of two fp32-representable values and its accumulation exact to 1e-16.
// What is left of the error against a float64 evaluation of the reference's lines is the fp32 mel product and log10.
// Reflect padding (torch.stft center = True) and a clip's end are index arithmetic on the clip's own length: nothing at or beyond
// lengths[b] is ever loaded.
#include "gn_chan.h"
#include "k4p.h"
#include "kernels.h"

#include <math.h>

namespace lds {

constexpr int LM_NFFT = 400, LM_HOP = 160, LM_BINS = 201;
constexpr int LM_FB = 16;                                      // frames per workgroup
constexpr int LM_SPAN = LM_HOP * (LM_FB - 1) + LM_NFFT;        // samples a workgroup's frames cover

static __device__ __forceinline__ float block_max_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();      // (red may still be read from an earlier use)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// grid (ceil(Fmax / LM_FB), B).  slen: device int32 [B] sample counts (null = L).  logspec plain [B][n_mels][Fmax] receives
// log10(max(mel, 1e-10)) of the clip's own frames only; pmax [B][gridDim.x] the workgroup's maximum (-inf for a workgroup beyond the clip).
__global__ void __launch_bounds__(256) logmel_power_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L, int Fmax,
                                                           const double2* __restrict__ basis, const float* __restrict__ filtT, int n_mels,
                                                           float* __restrict__ logspec, float* __restrict__ pmax) {
    __shared__ double xs[LM_SPAN];
    __shared__ float pw[LM_BINS][LM_FB];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * LM_FB;
    const long long n = slen ? (long long)slen[b] : L;
    const int F = (int)(n / LM_HOP);
    if (f0 >= F) {
        if (tid == 0) pmax[(long long)b * gridDim.x + blockIdx.x] = -INFINITY;
        return;
    }
    const int nf = (F - f0 < LM_FB) ? F - f0 : LM_FB;
    const int used = LM_HOP * (nf - 1) + LM_NFFT;
    for (int i = tid; i < LM_SPAN; i += 256) {
        long long s = (long long)f0 * LM_HOP - LM_NFFT / 2 + i;
        if (s < 0) s = -s;                       // reflect, edge sample not repeated
        if (s >= n) s = 2 * (n - 1) - s;
        xs[i] = (i < used && s >= 0 && s < n) ? (double)audio[(long long)b * L + s] : 0.0;
    }
    __syncthreads();
    if (tid < LM_BINS) {
        double re[LM_FB], im[LM_FB];
#pragma unroll
        for (int f = 0; f < LM_FB; ++f) { re[f] = 0.0; im[f] = 0.0; }
        for (int i = 0; i < LM_NFFT; ++i) {
            const double2 cs = basis[i * LM_BINS + tid];
#pragma unroll
            for (int f = 0; f < LM_FB; ++f) {
                const double x = xs[f * LM_HOP + i];
                re[f] = fma(cs.x, x, re[f]);
                im[f] = fma(cs.y, x, im[f]);
            }
        }
#pragma unroll
        for (int f = 0; f < LM_FB; ++f) pw[tid][f] = (float)(re[f] * re[f] + im[f] * im[f]);
    }
    __syncthreads();
    float lmax = -INFINITY;
    for (int o = tid; o < 2 * n_mels; o += 256) {
        const int g = o / n_mels, m = o - g * n_mels;      // 8 frames g * 8 .. g * 8 + 7 of mel channel m
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int k = 0; k < LM_BINS; ++k) {
            const float w = filtT[k * n_mels + m];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, pw[k][g * 8 + e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = g * 8 + e;
            if (f < nf) {
                const float v = log10f(fmaxf(acc[e], 1e-10f));
                logspec[((long long)b * n_mels + m) * Fmax + f0 + f] = v;
                lmax = fmaxf(lmax, v);
            }
        }
    }
    lmax = block_max_256(lmax, red);
    if (tid == 0) pmax[(long long)b * gridDim.x + blockIdx.x] = lmax;
}

// max(., clipmax - 8) then (. + 4) / 4 with clipmax over this clip's whole array (the maximum of the workgroups' partial maxima: exact
// and independent of any order).  grid (ceil((Fmax + 2) / 256), rows, B).  k4p: rows = n_mels / 4 K4P rows, one 16-byte entry per thread,
// pad frames and frames beyond the clip written as zeros; else rows = n_mels plain rows [B][n_mels][Fmax], zeros beyond the clip.
__global__ void __launch_bounds__(256) logmel_finish_kernel(const float* __restrict__ logspec, const float* __restrict__ pmax, int nblk,
                                                            const int* __restrict__ slen, long long L, int Fmax, int n_mels, int k4p,
                                                            float* __restrict__ out) {
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.z, row = blockIdx.y;
    float mx = -INFINITY;
    for (int i = tid; i < nblk; i += 256) mx = fmaxf(mx, pmax[(long long)b * nblk + i]);
    mx = block_max_256(mx, red);
    const float floor_v = mx - 8.0f;
    const int F = (int)((slen ? (long long)slen[b] : L) / LM_HOP);
    const int tt = blockIdx.x * 256 + tid;
    if (k4p) {
        if (tt >= Fmax + 2) return;
        const int t = tt - 1, q = row >> 1, h = row & 1;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < F) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 8 * q + 2 * j + h;
                v[j] = (fmaxf(logspec[((long long)b * n_mels + c) * Fmax + t], floor_v) + 4.0f) / 4.0f;
            }
        }
        *reinterpret_cast<float4*>(out + (((long long)b * (n_mels >> 2) + row) * (Fmax + 2) + tt) * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        if (tt >= Fmax) return;
        const long long o = ((long long)b * n_mels + row) * Fmax + tt;
        out[o] = (tt < F) ? (fmaxf(logspec[o], floor_v) + 4.0f) / 4.0f : 0.f;
    }
}

hipError_t launch_logmel(const float* audio, const int* slen, long long L, int Fmax, const double* basis, const float* filtT, int n_mels,
                         float* logspec, float* pmax, float* out, int out_k4p, int B, hipStream_t s) {
    if (B <= 0 || B > 65535 || Fmax <= 0 || n_mels <= 0 || n_mels % 8 || n_mels > 128) return hipErrorInvalidValue;
    const int nblk = (Fmax + LM_FB - 1) / LM_FB;
    {
        ProfScope ps(s, "logmel_power", 2.0 * B * (double)Fmax * LM_BINS * (2.0 * LM_NFFT + n_mels), 4.0 * B * ((double)Fmax * LM_HOP + (double)Fmax * n_mels));
        hipLaunchKernelGGL(logmel_power_kernel, dim3(nblk, B), dim3(256), 0, s, audio, slen, L, Fmax, reinterpret_cast<const double2*>(basis), filtT, n_mels,
                           logspec, pmax);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    ProfScope ps(s, "logmel_finish", 3.0 * B * (double)Fmax * n_mels, 8.0 * B * (double)Fmax * n_mels);
    const int cols = out_k4p ? Fmax + 2 : Fmax;
    hipLaunchKernelGGL(logmel_finish_kernel, dim3((cols + 255) / 256, out_k4p ? n_mels / 4 : n_mels, B), dim3(256), 0, s, logspec, pmax, nblk, slen, L, Fmax,
                       n_mels, out_k4p, out);
    return hipGetLastError();
}

// x (K4P [B][C][T], conv2's output: zeros beyond a clip's length and in the pad frames) += posk (the table in K4P order, one "batch
// element" of n_ctx frames) on the clip's own frames, and the (mean, M2) partials over every 32 channels of the sum, in the format of
// DmaConvArgs::lnpart_out ([B][C/32][T]; zeros beyond the clip: what conv_dma's epilogue writes for its zeroed columns).
// One thread per (frame, 32-channel group, clip): eight 16-byte entries, consecutive frames in consecutive lanes.
__global__ void __launch_bounds__(256) whisper_pos_kernel(float* __restrict__ x, const float* __restrict__ posk, int n_ctx, float2* __restrict__ lnpart,
                                                          const int* __restrict__ lens, int C, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const int Tb = ragged_len(lens, b, 1, T);
    float2* lp = lnpart + ((long long)b * (C >> 5) + g) * T + t;
    if (t >= Tb) { *lp = make_float2(0.f, 0.f); return; }
    float v[32];
#pragma unroll
    for (int r = 0; r < 8; ++r) {      // K4P row (4 g + r / 2, r % 2)
        const long long row = (long long)(g * 4 + (r >> 1)) * 2 + (r & 1);
        float4* xp = reinterpret_cast<float4*>(x + (((long long)b * (C >> 2) + row) * (T + 2) + t + 1) * 4);
        const float4 pv = *reinterpret_cast<const float4*>(posk + (row * (n_ctx + 2) + t + 1) * 4);
        float4 xv = *xp;
        xv.x += pv.x; xv.y += pv.y; xv.z += pv.z; xv.w += pv.w;
        *xp = xv;
        v[4 * r] = xv.x; v[4 * r + 1] = xv.y; v[4 * r + 2] = xv.z; v[4 * r + 3] = xv.w;
    }
    float s1 = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) s1 += v[r];
    const float mean = s1 * (1.0f / 32.0f);
    float m2 = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) { const float d = v[r] - mean; m2 = fmaf(d, d, m2); }
    *lp = make_float2(mean, m2);
}

hipError_t launch_whisper_pos(float* x, const float* posk, int n_ctx, float2* lnpart, const int* lens, int B, int C, int T, hipStream_t s) {
    if (B <= 0 || B > 65535 || C % 32 || T <= 0 || T > n_ctx) return hipErrorInvalidValue;
    ProfScope ps(s, "whisper_pos", 4.0 * B * (double)C * T, 8.0 * B * (double)C * T);
    hipLaunchKernelGGL(whisper_pos_kernel, dim3((T + 255) / 256, C / 32, B), dim3(256), 0, s, x, posk, n_ctx, lnpart, lens, C, T);
    return hipGetLastError();
}

// ln_post: out[b][t][c] = (x[b][c][t] - mean_t) * rstd_t * gamma[c] + beta[c] from the last block's LayerNorm partials (the statistics
// every folded LayerNorm of the stack uses, gn_chan.h ln_column_stats); rows t >= T_b are zeros.  LVL: the level of `lens` (1: Whisper's
// mel frames; 0: the wav2vec 2.0 encoder's own frame counts).  grid (ceil(T / 32), C / 64, B): a
// 64-channel x 32-frame tile goes through LDS so that both the K4P reads and the frame-major stores are whole lines.
template <int LVL>
__global__ void __launch_bounds__(256) whisper_ln_post_kernel(const float* __restrict__ x, const float2* __restrict__ lnpart, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                              const int* __restrict__ lens, int C, int T) {
    __shared__ float tile[32][65];
    __shared__ float smu[32], srs[32];
    const int tid = threadIdx.x, t0 = blockIdx.x * 32, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int Tb = ragged_len(lens, b, LVL, T);
    if (tid < 32) {
        const int t = t0 + tid;
        const bool ok = t < Tb;
        float mu, rs;
        ln_column_stats(lnpart + (long long)b * (C >> 5) * T + (ok ? t : 0), T, C >> 5, eps, ok, mu, rs);
        smu[tid] = mu; srs[tid] = rs;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = tid + 256 * e, row = idx >> 5, tl = idx & 31;      // 16 K4P rows of this channel block x 32 frames
        const int t = t0 + tl;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < Tb) v = *reinterpret_cast<const float4*>(x + (((long long)b * (C >> 2) + (c0 >> 2) + row) * (T + 2) + t + 1) * 4);
        const int cl = 8 * (row >> 1) + (row & 1);                          // channel 8 q + 2 j + h
        tile[tl][cl] = v.x; tile[tl][cl + 2] = v.y; tile[tl][cl + 4] = v.z; tile[tl][cl + 6] = v.w;
    }
    __syncthreads();
    const int c = tid & 63;
    const float ga = gamma[c0 + c], be = beta[c0 + c];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int tl = (tid >> 6) + 4 * e, t = t0 + tl;
        if (t < T) out[((long long)b * T + t) * C + c0 + c] = (t < Tb) ? fmaf((tile[tl][c] - smu[tl]) * srs[tl], ga, be) : 0.f;
    }
}

hipError_t launch_whisper_ln_post(const float* x, const float2* lnpart, const float* gamma, const float* beta, float eps, float* out, const int* lens,
                                  int B, int C, int T, hipStream_t s, int lvl) {
    if (B <= 0 || B > 65535 || C % 64 || T <= 0 || lvl < 0 || lvl > 1) return hipErrorInvalidValue;
    ProfScope ps(s, "whisper_ln_post", 4.0 * B * (double)C * T, 8.0 * B * (double)C * T);
    const dim3 grid((T + 31) / 32, C / 64, B);
    if (lvl) hipLaunchKernelGGL(whisper_ln_post_kernel<1>, grid, dim3(256), 0, s, x, lnpart, gamma, beta, eps, out, lens, C, T);
    else hipLaunchKernelGGL(whisper_ln_post_kernel<0>, grid, dim3(256), 0, s, x, lnpart, gamma, beta, eps, out, lens, C, T);
    return hipGetLastError();
}

}  // namespace lds
