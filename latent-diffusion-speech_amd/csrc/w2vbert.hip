// The w2v-BERT 2.0 units encoder's own kernels (a Conformer behind a Kaldi-style filter-bank front end; transformers' Wav2Vec2BertModel
// on SeamlessM4TFeatureExtractor's input_features).  Everything else of that encoder is conv_dma, attention_k4p_rel, hubert_ln,
// w2v_lnpart and hubert_store_frames launches (model.hip w2vbert_run).  Tensors between the kernels are K4P (k4p.h) and keep its
// invariants: the two pad frames of every row and the frames at and beyond a clip's own count are zeros.  Every reduction runs in a fixed
// order, there are no atomics, and nothing at or beyond a clip's own sample / frame count is read.
//   w2vbert_fbank_power   audio -> natural log of the 80 Kaldi mel powers of every 400-sample frame (hop 160, not centred)
//   w2vbert_fbank_stats   per (clip, mel bin): mean and 1 / sqrt(var(ddof = 1) + 1e-7) over the clip's own frames, two passes
//   w2vbert_fbank_finish  normalise, stack `stride` frames per row: input_features [B][Rmax][n_mels * stride], zeros beyond a clip's rows
//   w2vbert_feats_k4p     input_features -> K4P + the (mean, M2) partials the feature projection's folded LayerNorm reads
//   w2vbert_relpos        p[b][head][t][r] = q_t . E[r]: the relative-key table the attention kernel adds to its scores
//   w2vbert_dwconv        causal depthwise convolution + LayerNorm over the channels of each frame + swish, one pass
#include "k4p.h"
#include "kernels.h"

#include <math.h>

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- filter bank ---------------------------------------------------------------------------------------------------------------------
// logmel.hip's scheme: the framed DFT is a product of the frames with a basis kept in double, here [400][257] (cos, sin) pairs with the
// 2^15 scale, the frame's mean removal, the pre-emphasis and the Povey window folded in on the host (all of them linear in the frame's
// samples; model.hip w2vbert_basis), summed as double FMAs.  The reference rounds the spectrum to complex64; this keeps more.
constexpr int FB_NFFT = 400, FB_HOP = 160, FB_BINS = 257;
constexpr int FB_FB = 16;                                      // frames per workgroup
constexpr int FB_SPAN = FB_HOP * (FB_FB - 1) + FB_NFFT;        // samples a workgroup's frames cover

static __device__ __forceinline__ int fb_frames(long long n) { return n < FB_NFFT ? 0 : (int)((n - FB_NFFT) / FB_HOP) + 1; }

// grid (ceil(Nmax / FB_FB), B), 320 threads (one per bin).  logspec plain [B][n_mels][Nmax] receives log(max(mel, floor)) of the clip's
// own frames only.
__global__ void __launch_bounds__(320) w2vbert_fbank_power_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L, int Nmax,
                                                                  const double2* __restrict__ basis, const float* __restrict__ filtT, int n_mels,
                                                                  float mel_floor, float* __restrict__ logspec) {
    __shared__ double xs[FB_SPAN];
    __shared__ float pw[FB_BINS][FB_FB];
    const int tid = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * FB_FB;
    const long long n = slen ? (long long)slen[b] : L;
    const int N = fb_frames(n);
    if (f0 >= N) return;
    const int nf = (N - f0 < FB_FB) ? N - f0 : FB_FB;
    const int used = FB_HOP * (nf - 1) + FB_NFFT;      // (the last used sample is the clip's sample f0 * 160 + used - 1 < n)
    for (int i = tid; i < FB_SPAN; i += 320) xs[i] = (i < used) ? (double)audio[(long long)b * L + (long long)f0 * FB_HOP + i] : 0.0;
    __syncthreads();
    if (tid < FB_BINS) {
        double re[FB_FB], im[FB_FB];
#pragma unroll
        for (int f = 0; f < FB_FB; ++f) { re[f] = 0.0; im[f] = 0.0; }
        for (int i = 0; i < FB_NFFT; ++i) {
            const double2 cs = basis[i * FB_BINS + tid];
#pragma unroll
            for (int f = 0; f < FB_FB; ++f) {
                const double x = xs[f * FB_HOP + i];
                re[f] = fma(cs.x, x, re[f]);
                im[f] = fma(cs.y, x, im[f]);
            }
        }
#pragma unroll
        for (int f = 0; f < FB_FB; ++f) pw[tid][f] = (float)(re[f] * re[f] + im[f] * im[f]);
    }
    __syncthreads();
    for (int o = tid; o < 2 * n_mels; o += 320) {
        const int g = o / n_mels, m = o - g * n_mels;      // 8 frames g * 8 .. g * 8 + 7 of mel channel m
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int k = 0; k < FB_BINS; ++k) {
            const float w = filtT[k * n_mels + m];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, pw[k][g * 8 + e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = g * 8 + e;
            if (f < nf) logspec[((long long)b * n_mels + m) * Nmax + f0 + f] = logf(fmaxf(acc[e], mel_floor));
        }
    }
}

// fixed-order sum of one double per thread over the 256 threads of a workgroup (a halving tree: the order does not depend on timing)
static __device__ __forceinline__ double fb_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();      // (red may still be read from an earlier use)
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// grid (n_mels, B): stat[b][m] = (mean, 1 / sqrt(var(ddof = 1) + 1e-7)) of logspec[b][m][0 .. N_b), two passes in double, kept in double
__global__ void __launch_bounds__(256) w2vbert_fbank_stats_kernel(const float* __restrict__ logspec, const int* __restrict__ slen, long long L, int Nmax,
                                                                  int n_mels, double2* __restrict__ stat) {
    __shared__ double red[256];
    const int tid = threadIdx.x, m = blockIdx.x, b = blockIdx.y;
    const int N = fb_frames(slen ? (long long)slen[b] : L);
    const float* x = logspec + ((long long)b * n_mels + m) * Nmax;
    double s = 0.0;
    for (int i = tid; i < N; i += 256) s += (double)x[i];
    const double mean = fb_block_sum(s, red) / (double)N;
    double q = 0.0;
    for (int i = tid; i < N; i += 256) { const double d = (double)x[i] - mean; q = fma(d, d, q); }
    const double var = fb_block_sum(q, red) / (double)(N - 1);      // (N >= 2: the callers reject shorter clips)
    if (tid == 0) stat[(long long)b * n_mels + m] = make_double2(mean, 1.0 / sqrt(var + 1e-7));      // (double: the mean is ~20, the deviations ~1)
}

// out [B][Rmax][n_mels * stride]: row r holds the normalised frames stride r .. stride r + stride - 1 side by side; a frame at or beyond
// the clip's N_b (the tail of an odd clip's last row) is the extractor's padding, 0; rows at and beyond ceil(N_b / stride) are zeros
__global__ void __launch_bounds__(256) w2vbert_fbank_finish_kernel(const float* __restrict__ logspec, const double2* __restrict__ stat,
                                                                   const int* __restrict__ slen, long long L, int Nmax, int Rmax, int n_mels, int stride,
                                                                   float* __restrict__ out) {
    const int W = n_mels * stride, b = blockIdx.y;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)Rmax * W) return;
    const int r = (int)(e / W), c = (int)(e - (long long)r * W);
    const int f = r * stride + c / n_mels, m = c % n_mels;
    const int N = fb_frames(slen ? (long long)slen[b] : L);
    float v = 0.f;
    if (f < N) {
        const double2 st = stat[(long long)b * n_mels + m];
        v = (float)(((double)logspec[((long long)b * n_mels + m) * Nmax + f] - st.x) * st.y);
    }
    out[(long long)b * Rmax * W + e] = v;
}

hipError_t launch_w2vbert_fbank(const float* audio, const int* slen, long long L, int Nmax, int Rmax, const double* basis, const float* filtT, int n_mels,
                                int stride, float mel_floor, float* logspec, double2* stat, float* out, int B, hipStream_t s) {
    if (B <= 0 || B > 65535 || Nmax < 2 || Rmax <= 0 || n_mels <= 0 || n_mels > 128 || stride < 1 || L < (long long)(Nmax - 1) * FB_HOP + FB_NFFT)
        return hipErrorInvalidValue;
    {
        ProfScope ps(s, "w2vbert_fbank_power", 2.0 * B * (double)Nmax * FB_BINS * (2.0 * FB_NFFT + n_mels), 4.0 * B * ((double)Nmax * FB_HOP + (double)Nmax * n_mels));
        hipLaunchKernelGGL(w2vbert_fbank_power_kernel, dim3((Nmax + FB_FB - 1) / FB_FB, B), dim3(320), 0, s, audio, slen, L, Nmax,
                           reinterpret_cast<const double2*>(basis), filtT, n_mels, mel_floor, logspec);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    {
        ProfScope ps(s, "w2vbert_fbank_stats", 4.0 * B * (double)Nmax * n_mels, 8.0 * B * (double)Nmax * n_mels);
        hipLaunchKernelGGL(w2vbert_fbank_stats_kernel, dim3(n_mels, B), dim3(256), 0, s, logspec, slen, L, Nmax, n_mels, stat);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    ProfScope ps(s, "w2vbert_fbank_finish", 2.0 * B * (double)Nmax * n_mels, 4.0 * B * ((double)Nmax * n_mels + (double)Rmax * n_mels * stride));
    const long long tot = (long long)Rmax * n_mels * stride;
    hipLaunchKernelGGL(w2vbert_fbank_finish_kernel, dim3((unsigned)((tot + 255) / 256), B), dim3(256), 0, s, logspec, stat, slen, L, Nmax, Rmax, n_mels, stride, out);
    return hipGetLastError();
}

// ---- input_features -> K4P -----------------------------------------------------------------------------------------------------------
// feats [B][T][C] frame-major -> out K4P [B][C][T] and part [B][C / 32][T] = (mean, M2) of every 32 channels (DmaConvArgs::ln_part's
// format).  Rows at and beyond vlen[b] (the clip's unmasked rows) are not read: zeros and (0, 0).  One thread per (entry column, 32-channel
// group, clip): 128 contiguous bytes in, eight 16-byte K4P entries out.  grid (ceil((T + 2) / 256), C / 32, B).
__global__ void __launch_bounds__(256) w2vbert_feats_k4p_kernel(const float* __restrict__ feats, float* __restrict__ out, float2* __restrict__ part,
                                                                const int* __restrict__ vlen, int C, int T) {
    const int e = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z;
    if (e >= T + 2) return;
    const int t = e - 1;
    const int Tv = vlen ? (vlen[b] < T ? vlen[b] : T) : T;
    const bool live = t >= 0 && t < Tv;
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = 0.f;
    if (live) {
        const f32x4* src = reinterpret_cast<const f32x4*>(feats + ((long long)b * T + t) * C + g * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 q = src[i];
            v[4 * i] = q[0]; v[4 * i + 1] = q[1]; v[4 * i + 2] = q[2]; v[4 * i + 3] = q[3];
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {      // K4P row g * 8 + r = (block g * 4 + r / 2, half r & 1): channels 8 (r / 2) + 2 j + (r & 1) of the group
        const int c0 = 8 * (r >> 1) + (r & 1);
        *reinterpret_cast<f32x4*>(out + (((long long)b * (C >> 2) + g * 8 + r) * (T + 2) + e) * 4) = f32x4{v[c0], v[c0 + 2], v[c0 + 4], v[c0 + 6]};
    }
    if (t < 0 || t >= T) return;
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s1 += v[i];
    const float mean = s1 * (1.0f / 32.0f);
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) { const float d = v[i] - mean; m2 = fmaf(d, d, m2); }
    part[((long long)b * (C >> 5) + g) * T + t] = live ? make_float2(mean, m2) : make_float2(0.f, 0.f);
}

hipError_t launch_w2vbert_feats_k4p(const float* feats, float* out, float2* part, const int* vlen, int B, int C, int T, hipStream_t s) {
    if (B <= 0 || B > 65535 || C < 32 || C % 32 || C / 32 > 65535 || T <= 0) return hipErrorInvalidValue;
    ProfScope ps(s, "w2vbert_feats_k4p", 3.0 * B * (double)C * T, 8.0 * B * (double)C * T);
    hipLaunchKernelGGL(w2vbert_feats_k4p_kernel, dim3((T + 2 + 255) / 256, C / 32, B), dim3(256), 0, s, feats, out, part, vlen, C, T);
    return hipGetLastError();
}

// ---- relative-key table --------------------------------------------------------------------------------------------------------------
// relp [B][heads][T][kRelStride]: entry r < NR of query t = scale2 * q_t . E[r] (E = the layer's distance_embedding [NR][64], shared by the
// heads; scale2 = log2(e) / 8, the unit of attention_k4p's scores), zeros for queries at and beyond qlen[b].  The attention kernel adds
// relp[t][clamp(j - t, -left, right) + left] to the score of key j.  grid (ceil(T / 64), heads, B), 256 threads: lane = query, wave w takes
// r = w, w + 4, ...; a query's 64 values stay in registers, E lies in LDS in the K4P order of those registers (one ds_read_b128 per four
// products, the same address in every lane), each sum runs over the head dimension in that fixed order.  The 64 x NR tile leaves through
// LDS so that the stores are whole lines.
constexpr int kRelPad = kW2vbertRelStride + 1;
__global__ void __launch_bounds__(256) w2vbert_relpos_kernel(const float* __restrict__ qk, const float* __restrict__ E, float* __restrict__ relp,
                                                             const int* __restrict__ qlen, int C, int T, int NR, float scale2) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Es = smem;                    // [NR][16][4]: entry e = kq * 2 + hh holds dims 8 kq + 2 j + hh
    float* Os = smem + NR * 64;          // [64][kRelPad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blockIdx.x * 64, hd = blockIdx.y, b = blockIdx.z, H = gridDim.y;
    const int Tq = qlen ? (qlen[b] < T ? qlen[b] : T) : T;
    for (int i = tid; i < NR * 64; i += 256) {
        const int r = i >> 6, k = i & 63, e = k >> 2, j = k & 3;
        Es[i] = E[r * 64 + 8 * (e >> 1) + 2 * j + (e & 1)];
    }
    const int t = t0 + lane;
    const bool live = t < Tq;
    f32x4 q[16];
    const float* qb = qk + ((long long)b * 2 * C + (long long)hd * 64) / 4 * (T + 2) * 4;      // K4P rows hd * 16 .. hd * 16 + 15 of the q half
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        q[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (live) q[e] = *reinterpret_cast<const f32x4*>(qb + ((long long)e * (T + 2) + t + 1) * 4);
        q[e] *= scale2;
    }
    __syncthreads();
    for (int r = wave; r < NR; r += 4) {
        const f32x4* er = reinterpret_cast<const f32x4*>(Es + r * 64);
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const f32x4 w = er[e];
            a = fmaf(q[e][0], w[0], a); a = fmaf(q[e][1], w[1], a); a = fmaf(q[e][2], w[2], a); a = fmaf(q[e][3], w[3], a);
        }
        Os[lane * kRelPad + r] = a;
    }
    for (int r = NR + wave; r < kW2vbertRelStride; r += 4) Os[lane * kRelPad + r] = 0.f;
    __syncthreads();
    const int nrow = (T - t0 < 64) ? T - t0 : 64;
    float* ob = relp + (((long long)b * H + hd) * T + t0) * kW2vbertRelStride;
    for (int i = tid; i < nrow * kW2vbertRelStride; i += 256) ob[i] = Os[(i / kW2vbertRelStride) * kRelPad + (i % kW2vbertRelStride)];
}

hipError_t launch_w2vbert_relpos(const float* qk, const float* E, float* relp, const int* qlen, int B, int C, int T, int heads, int NR, hipStream_t s) {
    if (B <= 0 || B > 65535 || heads < 1 || C != heads * 64 || T <= 0 || NR < 1 || NR > kW2vbertRelStride) return hipErrorInvalidValue;
    ProfScope ps(s, "w2vbert_relpos", 2.0 * B * (double)C * T * NR, 4.0 * B * ((double)C * T + (double)heads * T * kW2vbertRelStride));
    const size_t lds_bytes = ((size_t)NR * 64 + 64 * kRelPad) * sizeof(float);
    hipLaunchKernelGGL(w2vbert_relpos_kernel, dim3((T + 63) / 64, heads, B), dim3(256), lds_bytes, s, qk, E, relp, qlen, C, T, NR,
                       1.4426950408889634f / 8.0f);
    return hipGetLastError();
}

// ---- depthwise causal convolution + LayerNorm + swish ----------------------------------------------------------------------------------
// out (K4P, not x) = swish(LN_c(y)), y[c][t] = sum_k w[c][k] x[c][t - (K - 1) + k]: frames before the clip's start and input frames at and
// beyond vlen[b] read as zeros (whatever x holds there), output frames at and beyond nlen[b] are zeros.  The statistics belong to a frame, so
// a frame's C channels stay in registers between the convolution and the store: hubert_ln's thread map (grid (ceil(T / 16), B), thread
// (frame tl, slice sl) holds the K4P rows sl, sl + 16, ...).  Sixteen K4P rows x the block's 16 + K - 1 input frames pass through LDS at a
// time, so the tensor is read from memory once (plus the K - 1 frame halo per block); wp = the taps packed [K4P row][k][4] (one 16-byte
// load per tap, the same address in the 16 lanes of a slice).  K <= 32, C a multiple of 64 up to 1024.
constexpr int kDwMaxK = 32;
__global__ void __launch_bounds__(256) w2vbert_dwconv_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                             const int* __restrict__ vlen, const int* __restrict__ nlen, int C, int T, int K) {
    __shared__ f32x4 tile[16][16 + kDwMaxK];
    __shared__ float red[16][17];
    const int tid = threadIdx.x, tl = tid & 15, sl = tid >> 4;
    const int t0 = blockIdx.x * 16, t = t0 + tl, b = blockIdx.y;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
    const int Tv = vlen ? (vlen[b] < Tb ? vlen[b] : Tb) : Tb;
    const bool live = t < Tb;
    const int rps = C >> 6;      // rows per slice
    const long long base = (long long)b * (C >> 2) * (T + 2);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (t0 >= Tb) {      // (block-uniform) all 16 frames lie beyond the clip
        if (t < T) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e < rps) {
                    float* o = out + (base + (long long)(sl + 16 * e) * (T + 2) + t + 1) * 4;
                    *reinterpret_cast<f32x4*>(o) = zero;
                    if (t == T - 1) *reinterpret_cast<f32x4*>(o + 4) = zero;
                }
        }
        return;
    }
    const int span = 15 + K;      // input frames t0 - (K - 1) .. t0 + 15
    f32x4 v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        v[e] = zero;
        if (e < rps) {      // (block-uniform)
            __syncthreads();      // every thread is done with the previous rows' tile
            for (int idx = tid; idx < 16 * span; idx += 256) {
                const int r = idx / span, f = idx - r * span, fr = t0 - (K - 1) + f;
                f32x4 q = zero;
                if (fr >= 0 && fr < Tv) q = *reinterpret_cast<const f32x4*>(x + (base + (long long)(r + 16 * e) * (T + 2) + fr + 1) * 4);
                tile[r][f] = q;
            }
            __syncthreads();
            const f32x4* w = reinterpret_cast<const f32x4*>(wp) + (long long)(sl + 16 * e) * K;
            f32x4 a = zero;
            for (int k = 0; k < K; ++k) {
                const f32x4 wk = w[k], xv = tile[sl][tl + k];
                a[0] = fmaf(wk[0], xv[0], a[0]); a[1] = fmaf(wk[1], xv[1], a[1]); a[2] = fmaf(wk[2], xv[2], a[2]); a[3] = fmaf(wk[3], xv[3], a[3]);
            }
            v[e] = a;
        }
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
            f32x4 y = zero;
            if (live) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = fmaf((v[e][j] - mean) * rs, gamma[cb + 2 * j], beta[cb + 2 * j]);
                    y[j] = u / (1.0f + expf(-u));
                }
            }
            float* o = out + (base + (long long)row * (T + 2) + t + 1) * 4;
            *reinterpret_cast<f32x4*>(o) = y;
            if (t == 0) *reinterpret_cast<f32x4*>(o - 4) = zero;
            if (t == T - 1) *reinterpret_cast<f32x4*>(o + 4) = zero;
        }
    }
}

hipError_t launch_w2vbert_dwconv(const float* x, const float* wp, const float* gamma, const float* beta, float eps, float* out, const int* vlen,
                                 const int* nlen, int B, int C, int T, int K, hipStream_t s) {
    if (B <= 0 || B > 65535 || C < 64 || C % 64 || C > 1024 || T <= 0 || K < 1 || K > kDwMaxK || x == out) return hipErrorInvalidValue;
    ProfScope ps(s, "w2vbert_dwconv", (2.0 * K + 10.0) * B * (double)C * T, 8.0 * B * (double)C * T);
    hipLaunchKernelGGL(w2vbert_dwconv_kernel, dim3((T + 15) / 16, B), dim3(256), 0, s, x, wp, gamma, beta, eps, out, vlen, nlen, C, T, K);
    return hipGetLastError();
}

}  // namespace lds
