// The HuBERT units encoder's own kernels (reference encoder/hubert/model.py:96-148); everything else of that encoder is conv_dma and
// attention_k4p launches (model.hip hubert_run).  All tensors between the kernels are K4P (k4p.h) and keep its invariants: the two pad
// frames of every row and the frames at and beyond a clip's own count are zeros.  Exact fp32, every reduction in a fixed order, no atomics.
//   hubert_conv0_stats / _finalize / _apply   conv0 (1 -> C, k 10, stride 5, no bias) + GroupNorm(C, C) + GELU
//   hubert_posconv                             x + GELU(grouped conv, k <= 128, "same" padding, last frame dropped) on the fp32 MFMA
//   hubert_ln                                  LayerNorm over the channels of a K4P tensor, materialised (post-LN blocks: it is the residual)
//   hubert_store_frames                        K4P -> frame-major [B][T][C] with zero rows beyond a clip
#include "k4p.h"
#include "kernels.h"

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHubK0 = 10, kHubS0 = 5;      // conv0's kernel and stride (model.py:99)
constexpr int kHubChunk = 256;              // frames per partial of norm0's statistics

static __device__ __forceinline__ float hub_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
// butterfly sum: both lanes of a pair add the same two numbers, so every lane ends with the same bits
static __device__ __forceinline__ float hub_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// one output of conv0: the taps in order, one fmaf chain
static __device__ __forceinline__ float hub_conv0(const float* __restrict__ w, const float (&x)[kHubK0]) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < kHubK0; ++k) a = fmaf(w[k], x[k], a);
    return a;
}

// ---- conv0 + norm0 + GELU --------------------------------------------------------------------------------------------------------
// The raw convolution is never stored: it is ten multiply-adds per output from an audio window that stays in cache, against a round trip
// of C x N0 floats (196 MB per 30 s clip at C = 512).  Pass 1 recomputes it for the statistics, pass 2 for the value.
//
// Pass 1: (mean, M2) of every channel over one chunk of 256 frames, two-pass inside the chunk (exact mean first, then the squares of the
// deviations).  grid (chunks, C / 64, B); a wave takes 16 channels, its lanes the frames.  Chunks beyond the clip's n0 write nothing.
__global__ void __launch_bounds__(256) hubert_conv0_stats_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L, int pad,
                                                                 const float* __restrict__ w0, const int* __restrict__ nlen, int N0, int C, int nchunk,
                                                                 float2* __restrict__ part) {
    __shared__ float xs[kHubChunk * kHubS0 + kHubK0];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = blockIdx.x, b = blockIdx.z;
    const int Lb = slen ? slen[b] : (int)L;
    const int Nb = nlen ? (nlen[b] < N0 ? nlen[b] : N0) : N0;
    const int t0 = chunk * kHubChunk;
    const int nv = (Nb - t0 < kHubChunk) ? Nb - t0 : kHubChunk;
    if (nv <= 0) return;
    const float* ab = audio + (long long)b * L;
    for (int i = tid; i < kHubChunk * kHubS0 + kHubK0 - kHubS0; i += 256) {
        const long long s = (long long)t0 * kHubS0 + i - pad;
        xs[i] = (s >= 0 && s < Lb) ? ab[s] : 0.f;
    }
    __syncthreads();
    float xv[4][kHubK0];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < kHubK0; ++k) xv[i][k] = xs[(lane + 64 * i) * kHubS0 + k];
    const float rn = 1.0f / (float)nv;
    for (int cc = 0; cc < 16; ++cc) {
        const int c = blockIdx.y * 64 + wave * 16 + cc;
        const float* w = w0 + (long long)c * kHubK0;
        float v[4], s1 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = hub_conv0(w, xv[i]);
            s1 += (lane + 64 * i < nv) ? v[i] : 0.f;
        }
        const float mean = hub_wave_sum(s1) * rn;
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = v[i] - mean;
            s2 += (lane + 64 * i < nv) ? d * d : 0.f;
        }
        s2 = hub_wave_sum(s2);
        if (lane == 0) part[((long long)b * nchunk + chunk) * C + c] = make_float2(mean, s2);
    }
}
// the chunks of one (clip, channel) combined in chunk order with Chan's update (the formula of gn_chan.h's partials):
//   N = n + n_i, d = mean_i - mean, mean += d n_i / N, M2 += M2_i + d^2 n n_i / N;   stat = (mean, 1 / sqrt(M2 / N + eps)), biased variance
__global__ void __launch_bounds__(256) hubert_conv0_finalize_kernel(const float2* __restrict__ part, const int* __restrict__ nlen, int N0, int C, int nchunk,
                                                                    float eps, float2* __restrict__ stat) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    const int Nb = nlen ? (nlen[b] < N0 ? nlen[b] : N0) : N0;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int nv = (Nb - ch * kHubChunk < kHubChunk) ? Nb - ch * kHubChunk : kHubChunk;
        if (nv <= 0) break;
        const float2 p = part[((long long)b * nchunk + ch) * C + c];
        const float ni = (float)nv, N = n + ni, d = p.x - mean;
        mean += d * (ni / N);
        m2 += p.y + d * d * (n * ni / N);
        n = N;
    }
    stat[(long long)b * C + c] = make_float2(mean, 1.0f / sqrtf(m2 / n + eps));
}
// Pass 2: out (K4P [B][C][N0]) = GELU((conv0 - mean) rstd gamma + beta) on the clip's own frames, zeros beyond and in the pad frames.
// grid (ceil((N0 + 2) / 256), C / 64, B): a thread takes one entry column (frame -1 .. N0) of 64 channels = 16 entries of 16 bytes,
// consecutive lanes consecutive frames.
__global__ void __launch_bounds__(256) hubert_conv0_apply_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L, int pad,
                                                                 const float* __restrict__ w0, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float2* __restrict__ stat, const int* __restrict__ nlen, int N0, int C,
                                                                 float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    if (e >= N0 + 2) return;
    const int t = e - 1;
    const int Lb = slen ? slen[b] : (int)L;
    const int Nb = nlen ? (nlen[b] < N0 ? nlen[b] : N0) : N0;
    const bool live = t >= 0 && t < Nb;
    float x[kHubK0];
    const float* ab = audio + (long long)b * L;
#pragma unroll
    for (int k = 0; k < kHubK0; ++k) {
        const long long s = (long long)t * kHubS0 + k - pad;
        x[k] = (live && s >= 0 && s < Lb) ? ab[s] : 0.f;
    }
    const int c0 = blockIdx.y * 64;
    for (int r = 0; r < 16; ++r) {                  // K4P row (q, h) = (c0 / 8 + r / 2, r % 2): channels 8 q + h + 2 j
        const int cb = c0 + 8 * (r >> 1) + (r & 1);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = cb + 2 * j;
                const float2 st = stat[(long long)b * C + c];
                v[j] = hub_gelu(fmaf((hub_conv0(w0 + (long long)c * kHubK0, x) - st.x) * st.y, gamma[c], beta[c]));
            }
        }
        *reinterpret_cast<f32x4*>(out + (((long long)b * (C >> 2) + (c0 >> 2) + r) * (N0 + 2) + e) * 4) = v;
    }
}

hipError_t launch_hubert_conv0(const float* audio, const int* slen, long long L, int pad, const float* w0, const float* gamma, const float* beta, float eps,
                               const int* nlen, int N0, int C, float2* part, float2* stat, float* out, int B, hipStream_t s) {
    if (B <= 0 || B > 65535 || C % 64 || N0 <= 0 || pad < 0 || L <= 0) return hipErrorInvalidValue;
    const int nchunk = (N0 + kHubChunk - 1) / kHubChunk;
    {
        ProfScope ps(s, "hubert_conv0_stats", 2.0 * kHubK0 * B * (double)C * N0, 4.0 * B * (double)L);
        hipLaunchKernelGGL(hubert_conv0_stats_kernel, dim3(nchunk, C / 64, B), dim3(256), 0, s, audio, slen, L, pad, w0, nlen, N0, C, nchunk, part);
        hipLaunchKernelGGL(hubert_conv0_finalize_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, part, nlen, N0, C, nchunk, eps, stat);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    ProfScope ps(s, "hubert_conv0_apply", 2.0 * kHubK0 * B * (double)C * N0, 4.0 * B * (double)C * N0);
    hipLaunchKernelGGL(hubert_conv0_apply_kernel, dim3((N0 + 2 + 255) / 256, C / 64, B), dim3(256), 0, s, audio, slen, L, pad, w0, gamma, beta, stat, nlen, N0,
                       C, out);
    return hipGetLastError();
}

// ---- positional convolution --------------------------------------------------------------------------------------------------------
// out = x + GELU(bias + sum_{ci in group, k < K} w[c][ci][k] x[ci][t - K / 2 + k]) with zeros outside the clip's [0, T_b): the reference's
// Conv1d(padding K / 2) with its last output frame dropped (model.py:136-148).  Per group a GEMM of GW = C / groups rows, GW K deep, on
// v_mfma_f32_16x16x4_f32.  A workgroup takes (64 frames, one group, one clip): the group's input window (GW rows x 64 + K - 1 frames) is
// staged once into LDS; wave w reduces the taps k = w, w + 4, ... (each over all the group's channels, four at a time) for the whole
// GW x 64 tile, and the four partial tiles meet in LDS, added in wave order.  So an output's summation order is fixed by (K, GW) alone.
// Weights packed by the host (model.hip pack_posconv): [group][k][ci / 4][row tile][64 lanes], lane l = row (l & 15), ci offset (l >> 4):
// one 256-byte line per A operand.
constexpr int kPosNT = 64, kPosWP = 208;      // row stride = 16 (mod 32): the four k-rows of one ds_read_b32 fall on disjoint bank groups
constexpr int kPosRS = 65;

template <int MT>
__global__ void __launch_bounds__(256) hubert_posconv_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                                                             float* __restrict__ out, const int* __restrict__ nlen, int C, int T, int K) {
    constexpr int GW = 16 * MT;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // the window [GW][kPosWP], then the partial tiles [4][GW][kPosRS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int t0 = blockIdx.x * kPosNT, g = blockIdx.y, b = blockIdx.z;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
    const bool dead = t0 >= Tb;      // (block-uniform)
    const long long xb = ((long long)b * (C >> 2) + g * (GW / 4)) * (T + 2);      // entry index of this group's first row
    if (!dead) {
        const int W = kPosNT + K - 1, half = K >> 1;
        for (int idx = tid; idx < (GW / 4) * W; idx += 256) {
            const int r = idx / W, f = idx - r * W;
            const int t = t0 - half + f;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t >= 0 && t < Tb) v = *reinterpret_cast<const f32x4*>(x + (xb + (long long)r * (T + 2) + t + 1) * 4);
            float* d = smem + (8 * (r >> 1) + (r & 1)) * kPosWP + f;
            d[0] = v[0]; d[2 * kPosWP] = v[1]; d[4 * kPosWP] = v[2]; d[6 * kPosWP] = v[3];
        }
        __syncthreads();
        f32x4 acc[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* xl = smem + l4 * kPosWP + l15;
        const float* wl = wp + (long long)g * K * (GW / 4) * MT * 64 + lane;
        for (int k = wave; k < K; k += 4) {
            const float* wk = wl + (long long)k * (GW / 4) * MT * 64;
#pragma unroll
            for (int c4 = 0; c4 < GW / 4; ++c4) {
                float a[MT], bv[4];
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = wk[(c4 * MT + m) * 64];
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = xl[4 * c4 * kPosWP + k + 16 * j];
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], bv[j], acc[m][j], 0, 0, 0);
            }
        }
        __syncthreads();      // every wave is done with the window
        float* red = smem + wave * GW * kPosRS;      // D[row = 4 (l >> 4) + r][col = l & 15]
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(m * 16 + 4 * l4 + r) * kPosRS + 16 * j + l15] = acc[m][j][r];
        __syncthreads();
    }
    for (int idx = tid; idx < (GW / 4) * kPosNT; idx += 256) {
        const int r = idx >> 6, tl = idx & 63, t = t0 + tl;
        if (t >= T) continue;
        const long long o = (xb + (long long)r * (T + 2) + t + 1) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!dead && t < Tb) {
            const f32x4 xin = *reinterpret_cast<const f32x4*>(x + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cl = 8 * (r >> 1) + (r & 1) + 2 * j;
                const float* p = smem + cl * kPosRS + tl;
                const float y = ((p[0] + p[GW * kPosRS]) + p[2 * GW * kPosRS]) + p[3 * GW * kPosRS] + bias[g * GW + cl];
                v[j] = xin[j] + hub_gelu(y);
            }
        }
        *reinterpret_cast<f32x4*>(out + o) = v;
        if (t == 0) *reinterpret_cast<f32x4*>(out + o - 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t == T - 1) *reinterpret_cast<f32x4*>(out + o + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int MT>
static hipError_t launch_posconv_cfg(const float* x, const float* wp, const float* bias, float* out, const int* nlen, int B, int C, int T, int K, int groups,
                                     hipStream_t s) {
    constexpr int GW = 16 * MT;
    constexpr size_t win = (size_t)GW * kPosWP, red = (size_t)4 * GW * kPosRS;
    constexpr size_t lds_bytes = (win > red ? win : red) * sizeof(float);
    auto kern = hubert_posconv_kernel<MT>;
    if (lds_bytes > 48 * 1024) {
        static std::atomic<unsigned long long> attr_done{0};
        hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((T + kPosNT - 1) / kPosNT, groups, B), dim3(256), lds_bytes, s, x, wp, bias, out, nlen, C, T, K);
    return hipGetLastError();
}

hipError_t launch_hubert_posconv(const float* x, const float* wp, const float* bias, float* out, const int* nlen, int B, int C, int T, int K, int groups,
                                 hipStream_t s) {
    if (B <= 0 || B > 65535 || groups <= 0 || groups > 65535 || C % groups || T <= 0 || K < 2 || K > 128 || (K & 1)) return hipErrorInvalidValue;
    const int gw = C / groups;
    ProfScope ps(s, "hubert_posconv", 2.0 * B * (double)C * gw * K * T, 4.0 * (2.0 * B * (double)C * T + (double)C * gw * K));
    switch (gw) {
        case 16: return launch_posconv_cfg<1>(x, wp, bias, out, nlen, B, C, T, K, groups, s);
        case 32: return launch_posconv_cfg<2>(x, wp, bias, out, nlen, B, C, T, K, groups, s);
        case 48: return launch_posconv_cfg<3>(x, wp, bias, out, nlen, B, C, T, K, groups, s);
        case 64: return launch_posconv_cfg<4>(x, wp, bias, out, nlen, B, C, T, K, groups, s);
        default: return hipErrorInvalidValue;
    }
}

// ---- LayerNorm over the channels, materialised ----------------------------------------------------------------------------------------
// out (K4P) = (x - mean_t) rstd_t gamma + beta per frame, statistics two-pass over the frame's C channels (the values stay in registers).
// grid (ceil(T / 16), B); thread (frame tl, slice s) holds the K4P rows s, s + 16, ... of its frame; the 16 slices' sums meet in LDS and
// every thread adds them in slice order.  C a multiple of 64, at most 1024.
__global__ void __launch_bounds__(256) hubert_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        float* __restrict__ out, const int* __restrict__ nlen, int C, int T) {
    __shared__ float red[16][17];
    const int tid = threadIdx.x, tl = tid & 15, sl = tid >> 4;
    const int t = blockIdx.x * 16 + tl, b = blockIdx.y;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
    const bool live = t < Tb;
    const int rps = C >> 6;      // rows per slice
    const long long base = (long long)b * (C >> 2) * (T + 2);
    f32x4 v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        v[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < rps && live) v[e] = *reinterpret_cast<const f32x4*>(x + (base + (long long)(sl + 16 * e) * (T + 2) + t + 1) * 4);
    }
    float s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (e < rps) s1 += (v[e][0] + v[e][1]) + (v[e][2] + v[e][3]);
    red[sl][tl] = s1;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += red[i][tl];
    const float mean = tot / (float)C;
    __syncthreads();
    float s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (e < rps) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[e][j] - mean; s2 = fmaf(d, d, s2); }
        }
    red[sl][tl] = s2;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += red[i][tl];
    const float rs = 1.0f / sqrtf(tot / (float)C + eps);
    if (t >= T) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (e < rps) {
            const int row = sl + 16 * e, cb = 8 * (row >> 1) + (row & 1);
            f32x4 y = {0.f, 0.f, 0.f, 0.f};
            if (live) {
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = fmaf((v[e][j] - mean) * rs, gamma[cb + 2 * j], beta[cb + 2 * j]);
            }
            float* o = out + (base + (long long)row * (T + 2) + t + 1) * 4;
            *reinterpret_cast<f32x4*>(o) = y;
            if (t == 0) *reinterpret_cast<f32x4*>(o - 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t == T - 1) *reinterpret_cast<f32x4*>(o + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

hipError_t launch_hubert_ln(const float* x, const float* gamma, const float* beta, float eps, float* out, const int* nlen, int B, int C, int T, hipStream_t s) {
    if (B <= 0 || B > 65535 || C % 64 || C > 1024 || T <= 0) return hipErrorInvalidValue;
    ProfScope ps(s, "hubert_ln", 8.0 * B * (double)C * T, 8.0 * B * (double)C * T);
    hipLaunchKernelGGL(hubert_ln_kernel, dim3((T + 15) / 16, B), dim3(256), 0, s, x, gamma, beta, eps, out, nlen, C, T);
    return hipGetLastError();
}

// ---- K4P -> frame-major -----------------------------------------------------------------------------------------------------------------
// out[b][t][c] = x[b][c][t] for t < T_b, zeros beyond.  grid (ceil(T / 32), C / 64, B): a 64-channel x 32-frame tile goes through LDS so
// that both the K4P reads and the frame-major stores are whole lines (the tile of whisper_ln_post, logmel.hip).
__global__ void __launch_bounds__(256) hubert_store_frames_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ nlen, int C,
                                                                  int T) {
    __shared__ float tile[32][65];
    const int tid = threadIdx.x, t0 = blockIdx.x * 32, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = tid + 256 * e, row = idx >> 5, tl = idx & 31;      // 16 K4P rows of this channel block x 32 frames
        const int t = t0 + tl;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < Tb) v = *reinterpret_cast<const float4*>(x + (((long long)b * (C >> 2) + (c0 >> 2) + row) * (T + 2) + t + 1) * 4);
        const int cl = 8 * (row >> 1) + (row & 1);
        tile[tl][cl] = v.x; tile[tl][cl + 2] = v.y; tile[tl][cl + 4] = v.z; tile[tl][cl + 6] = v.w;
    }
    __syncthreads();
    const int c = tid & 63;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int tl = (tid >> 6) + 4 * e, t = t0 + tl;
        if (t < T) out[((long long)b * T + t) * C + c0 + c] = tile[tl][c];
    }
}

hipError_t launch_hubert_store_frames(const float* x, float* out, const int* nlen, int B, int C, int T, hipStream_t s) {
    if (B <= 0 || B > 65535 || C % 64 || T <= 0) return hipErrorInvalidValue;
    ProfScope ps(s, "hubert_store_frames", 0.0, 8.0 * B * (double)C * T);
    hipLaunchKernelGGL(hubert_store_frames_kernel, dim3((T + 31) / 32, C / 64, B), dim3(256), 0, s, x, out, nlen, C, T);
    return hipGetLastError();
}

// ---- K4P -> frame-major, accumulated: the weighted layer sum of the *ForXVector / *ForSequenceClassification heads ------------------------
// out[b][t][c] = (first ? 0 : out[b][t][c]) + w x[b][c][t] for t < T_b (one fmaf), zeros beyond: hubert_store_frames_kernel's tile with the
// running sum read back where the plain store overwrites.  The caller runs the hidden states in ascending order, so the order of a sum's
// terms is fixed.
__global__ void __launch_bounds__(256) hubert_store_frames_acc_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ nlen, int C,
                                                                      int T, float w, int first) {
    __shared__ float tile[32][65];
    const int tid = threadIdx.x, t0 = blockIdx.x * 32, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = tid + 256 * e, row = idx >> 5, tl = idx & 31;
        const int t = t0 + tl;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < Tb) v = *reinterpret_cast<const float4*>(x + (((long long)b * (C >> 2) + (c0 >> 2) + row) * (T + 2) + t + 1) * 4);
        const int cl = 8 * (row >> 1) + (row & 1);
        tile[tl][cl] = v.x; tile[tl][cl + 2] = v.y; tile[tl][cl + 4] = v.z; tile[tl][cl + 6] = v.w;
    }
    __syncthreads();
    const int c = tid & 63;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int tl = (tid >> 6) + 4 * e, t = t0 + tl;
        if (t < T) {
            float* o = out + ((long long)b * T + t) * C + c0 + c;
            *o = t < Tb ? fmaf(w, tile[tl][c], first ? 0.f : *o) : 0.f;
        }
    }
}

hipError_t launch_hubert_store_frames_acc(const float* x, float* out, const int* nlen, float w, int first, int B, int C, int T, hipStream_t s) {
    if (B <= 0 || B > 65535 || C % 64 || T <= 0) return hipErrorInvalidValue;
    ProfScope ps(s, "hubert_store_frames_acc", 2.0 * B * (double)C * T, 12.0 * B * (double)C * T);
    hipLaunchKernelGGL(hubert_store_frames_acc_kernel, dim3((T + 31) / 32, C / 64, B), dim3(256), 0, s, x, out, nlen, C, T, w, first);
    return hipGetLastError();
}

}  // namespace lds
