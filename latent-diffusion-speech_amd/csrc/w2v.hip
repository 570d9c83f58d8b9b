// The wav2vec 2.0 units encoder's own kernels (XLSR-53: the "layer norm" flavour of the network, every convolution of the feature extractor
// followed by a LayerNorm over the channels of each frame); everything else of that encoder is conv_dma, attention_k4p, hubert_posconv
// and whisper_ln_post launches (model.hip w2v_run).  All tensors between the kernels are K4P (k4p.h) and keep its invariants: the two
// pad frames of every row and the frames at and beyond a clip's own count are zeros.  Exact fp32, every reduction in a fixed order, no
// atomics.
//   w2v_conv0     conv0 (1 -> C, k 10, stride 5, bias) + LayerNorm over the C channels of each frame + GELU, one pass
//   w2v_ln_act    GELU(LayerNorm over the channels) of a K4P tensor, materialised; optionally the (mean, M2) partials of its output
//   w2v_lnpart    the (mean, M2) partials over every 32 channels of a K4P tensor (DmaConvArgs::lnpart_out's format)
#include "k4p.h"
#include "kernels.h"

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kW2vK0 = 10, kW2vS0 = 5;      // conv0's kernel and stride

static __device__ __forceinline__ float w2v_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// ---- conv0 + LayerNorm + GELU ------------------------------------------------------------------------------------------------------
// out (K4P [B][C][N0]) = GELU(LN_c(bias + conv0(audio))) on the clip's own frames, zeros beyond and in the pad frames.  The statistics
// belong to a frame, so a frame's C channels stay in registers between the convolution and the store and nothing raw is written.
// grid (ceil((N0 + 2) / 64), B), 512 threads: lane = entry column (frame -1 .. N0), wave w holds the K4P rows w, w + 8, ... of its 64
// frames, so every weight, bias, gamma and beta address is wave-uniform (scalar loads) and every store instruction writes 1 KB of one
// row.  The eight waves' sums meet in LDS and every thread adds them in wave order; two passes (mean, then squared deviations).
// NR = the most rows per wave (C / 32 <= NR).
template <int NR>
__global__ void __launch_bounds__(512) w2v_conv0_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L,
                                                        const float* __restrict__ w0, const float* __restrict__ bias, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, const int* __restrict__ nlen, int N0, int C,
                                                        float* __restrict__ out) {
    __shared__ float red[8][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int t = e - 1;
    const int Lb = slen ? slen[b] : (int)L;
    const int Nb = nlen ? (nlen[b] < N0 ? nlen[b] : N0) : N0;
    const int rps = C >> 5;      // rows per wave
    const long long ob = (long long)b * (C >> 2) * (N0 + 2);
    if ((int)blockIdx.x * 64 - 1 >= Nb) {      // (block-uniform) all 64 columns lie beyond the clip
        if (e < N0 + 2) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (r < rps) *reinterpret_cast<f32x4*>(out + (ob + (long long)(wave + 8 * r) * (N0 + 2) + e) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    const bool live = t >= 0 && t < Nb;
    float x[kW2vK0];
    const float* ab = audio + (long long)b * L;
#pragma unroll
    for (int k = 0; k < kW2vK0; ++k) {
        const long long s = (long long)t * kW2vS0 + k;
        x[k] = (live && s < Lb) ? ab[s] : 0.f;
    }
    f32x4 v[NR];
    float s1 = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < rps) {
            const int row = wave + 8 * r, cb = 8 * (row >> 1) + (row & 1);      // K4P row (q, h): channels 8 q + h + 2 j
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = cb + 2 * j;
                const float* w = w0 + (long long)c * kW2vK0;
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < kW2vK0; ++k) a = fmaf(w[k], x[k], a);
                v[r][j] = a + bias[c];
            }
            s1 += (v[r][0] + v[r][1]) + (v[r][2] + v[r][3]);
        }
    }
    red[wave][lane] = s1;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += red[i][lane];
    const float mean = tot / (float)C;
    __syncthreads();
    float s2 = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r < rps) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[r][j] - mean; s2 = fmaf(d, d, s2); }
        }
    red[wave][lane] = s2;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += red[i][lane];
    const float rs = 1.0f / sqrtf(tot / (float)C + eps);
    if (e >= N0 + 2) return;
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r < rps) {
            const int row = wave + 8 * r, cb = 8 * (row >> 1) + (row & 1);
            f32x4 y = {0.f, 0.f, 0.f, 0.f};
            if (live) {
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = w2v_gelu(fmaf((v[r][j] - mean) * rs, gamma[cb + 2 * j], beta[cb + 2 * j]));
            }
            *reinterpret_cast<f32x4*>(out + (ob + (long long)row * (N0 + 2) + e) * 4) = y;
        }
}

hipError_t launch_w2v_conv0(const float* audio, const int* slen, long long L, const float* w0, const float* bias, const float* gamma, const float* beta,
                            float eps, const int* nlen, int N0, int C, float* out, int B, hipStream_t s) {
    if (B <= 0 || B > 65535 || C < 64 || C % 64 || C > 1024 || N0 <= 0 || L < (long long)(N0 - 1) * kW2vS0 + kW2vK0) return hipErrorInvalidValue;
    ProfScope ps(s, "w2v_conv0", 2.0 * kW2vK0 * B * (double)C * N0, 4.0 * B * ((double)C * (N0 + 2) + (double)L));
    const dim3 grid((N0 + 2 + 63) / 64, B);
    if (C <= 512)
        hipLaunchKernelGGL(w2v_conv0_kernel<16>, grid, dim3(512), 0, s, audio, slen, L, w0, bias, gamma, beta, eps, nlen, N0, C, out);
    else
        hipLaunchKernelGGL(w2v_conv0_kernel<32>, grid, dim3(512), 0, s, audio, slen, L, w0, bias, gamma, beta, eps, nlen, N0, C, out);
    return hipGetLastError();
}

// ---- LayerNorm over the channels + GELU, materialised ----------------------------------------------------------------------------------
// out (K4P) = GELU((x - mean_t) rstd_t gamma + beta) per frame; hubert_ln's scheme: grid (ceil(T / 16), B), thread (frame tl, slice s)
// holds the K4P rows s, s + 16, ... of its frame, the 16 slices' sums meet in LDS and every thread adds them in slice order.  C a multiple
// of 64, at most 1024.  x and out are different tensors.
// PART: also part [B][C / 32][T] = (mean, M2) of every 32 channels of the OUTPUT (rows 8 g .. 8 g + 7 = slices 8 (g & 1) .. + 7 of register
// e = g / 2), two-pass and added in slice order; (0, 0) beyond a clip -- what conv_dma's epilogue writes as DmaConvArgs::lnpart_out.
template <bool PART>
__global__ void __launch_bounds__(256) w2v_ln_act_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         float* __restrict__ out, float2* __restrict__ part, const int* __restrict__ nlen, int C, int T) {
    __shared__ float red[16][17];
    __shared__ float ps[PART ? 16 : 1][16][17];
    __shared__ float gm[PART ? 32 : 1][17];
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
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (e < rps) {
            const int row = sl + 16 * e, cb = 8 * (row >> 1) + (row & 1);
            f32x4 y = {0.f, 0.f, 0.f, 0.f};
            if (live) {
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = w2v_gelu(fmaf((v[e][j] - mean) * rs, gamma[cb + 2 * j], beta[cb + 2 * j]));
            }
            v[e] = y;
            if (t < T) {
                float* o = out + (base + (long long)row * (T + 2) + t + 1) * 4;
                *reinterpret_cast<f32x4*>(o) = y;
                if (t == 0) *reinterpret_cast<f32x4*>(o - 4) = f32x4{0.f, 0.f, 0.f, 0.f};
                if (t == T - 1) *reinterpret_cast<f32x4*>(o + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    if constexpr (PART) {
        const int ng = C >> 5;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e < rps) ps[e][sl][tl] = (v[e][0] + v[e][1]) + (v[e][2] + v[e][3]);
        __syncthreads();
        for (int g = sl; g < ng; g += 16) {
            const int e = g >> 1, s0 = 8 * (g & 1);
            float m = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) m += ps[e][s0 + i][tl];
            gm[g][tl] = m * (1.0f / 32.0f);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e < rps) {
                const float mu = gm[2 * e + (sl >> 3)][tl];
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float d = v[e][j] - mu; q = fmaf(d, d, q); }
                ps[e][sl][tl] = q;
            }
        __syncthreads();
        for (int g = sl; g < ng; g += 16) {
            const int e = g >> 1, s0 = 8 * (g & 1);
            float m2 = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) m2 += ps[e][s0 + i][tl];
            if (t < T) part[((long long)b * ng + g) * T + t] = live ? make_float2(gm[g][tl], m2) : make_float2(0.f, 0.f);
        }
    }
}

hipError_t launch_w2v_ln_act(const float* x, const float* gamma, const float* beta, float eps, float* out, float2* part, const int* nlen, int B, int C, int T,
                             hipStream_t s) {
    if (B <= 0 || B > 65535 || C < 64 || C % 64 || C > 1024 || T <= 0 || x == out) return hipErrorInvalidValue;
    ProfScope ps(s, "w2v_ln_act", 8.0 * B * (double)C * T, 8.0 * B * (double)C * T);
    const dim3 grid((T + 15) / 16, B);
    if (part) hipLaunchKernelGGL(w2v_ln_act_kernel<true>, grid, dim3(256), 0, s, x, gamma, beta, eps, out, part, nlen, C, T);
    else hipLaunchKernelGGL(w2v_ln_act_kernel<false>, grid, dim3(256), 0, s, x, gamma, beta, eps, out, part, nlen, C, T);
    return hipGetLastError();
}

// ---- LayerNorm partials of a K4P tensor ------------------------------------------------------------------------------------------------
// part [B][C / 32][T] = (mean, M2) over every 32 channels of x at every frame of the clip, (0, 0) beyond it: the residual stream behind the
// positional convolution, whose first consumer is a convolution with its LayerNorm folded.  One thread per (frame, group, clip): eight
// 16-byte entries, consecutive frames in consecutive lanes (whisper_pos's pass without the table).
__global__ void __launch_bounds__(256) w2v_lnpart_kernel(const float* __restrict__ x, float2* __restrict__ part, const int* __restrict__ nlen, int C, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
    float2* lp = part + ((long long)b * (C >> 5) + g) * T + t;
    if (t >= Tb) { *lp = make_float2(0.f, 0.f); return; }
    float v[32];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (((long long)b * (C >> 2) + g * 8 + r) * (T + 2) + t + 1) * 4);
        v[4 * r] = xv[0]; v[4 * r + 1] = xv[1]; v[4 * r + 2] = xv[2]; v[4 * r + 3] = xv[3];
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

hipError_t launch_w2v_lnpart(const float* x, float2* part, const int* nlen, int B, int C, int T, hipStream_t s) {
    if (B <= 0 || B > 65535 || C < 32 || C % 32 || C / 32 > 65535 || T <= 0) return hipErrorInvalidValue;
    ProfScope ps(s, "w2v_lnpart", 3.0 * B * (double)C * T, 4.0 * B * (double)C * T);
    hipLaunchKernelGGL(w2v_lnpart_kernel, dim3((T + 255) / 256, C / 32, B), dim3(256), 0, s, x, part, nlen, C, T);
    return hipGetLastError();
}

}  // namespace lds
