// The HiFi-VAEGAN encoder's own convolutions (reference encoder/hifi_vaegan/modules/models.py:14-54):
//   conv_down   out[b,co,t] = bias[co] + sum_{ci,k} W[co][ci][k] * lrelu(x[b,ci, t*stride - pad + k]) over plain [B][Ci][L] input,
//               as an implicit GEMM (M = co, N = t, K = (ci, k) in the weight's own [Co][Ci*K] order) on v_mfma_f32_32x32x2_f32.
//               It runs conv_pre (1 -> 16, k 7, stride 1; slope 1 = no activation), the five strided downsamplers (k = 2u, stride u)
//               and conv_post (slope 0.01).  Taps outside [0, L) read exact zeros; in a ragged batch, so do taps at or beyond the element's
//               vlen_in, and frames at or beyond its vlen are stored as zeros (a workgroup wholly beyond vlen skips its reduction).
//   vae_head    conv_post's [B][2C][T] -> out [B][T][2C] (m, then logs or zeros) and z = m + n * exp(logs) as [B][T][C]; in a ragged
//               batch, rows beyond the element's frame count are zeros.
// Every output element is one k-ordered fmaf chain from zero (K-steps of 32 rows, two rows per MFMA) plus the bias, whatever the tile
// shape, so an utterance encodes to the same bits alone and inside a batch.
#include "kernels.h"

#include <math.h>
#include <stdio.h>

#include <algorithm>

namespace lds {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDownKC = 32;      // rows of the reduction per K-step

// 256 threads = 2 x 2 waves; a wave owns WM x WN tiles of 32 x 32, the workgroup (64 WM) channels x (64 WN) frames.
// Staging: thread (kk = tid & 31, r0 = tid >> 5) loads reduction row kk of channels / frames r0, r0 + 8, ...; lanes of a wave read
// consecutive weights of one channel (coalesced) and consecutive taps of one frame.  The next K-step's loads are issued before the
// current step's MFMAs (register prefetch), so global latency overlaps the matrix work.
template <int WM, int WN>
__global__ void __launch_bounds__(256) conv_down_kernel(const ConvDownArgs p) {
    constexpr int BM = 64 * WM, BN = 64 * WN, NW = BM / 8, NX = BN / 8;
    constexpr int SW = BM + 1, SX = BN + 1;      // odd row pitch: the transposing LDS stores do not collide
    __shared__ float Ws[kDownKC * SW];
    __shared__ float Xs[kDownKC * SX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, h = lane >> 5, c = lane & 31;
    const int t0 = blockIdx.x * BN, co0 = blockIdx.y * BM, b = blockIdx.z;
    const int Kd = p.Ci * p.K;
    const int kk = tid & 31, r0 = tid >> 5;
    const float* xb = p.x + (long long)b * p.Ci * p.L;
    const int Lin = p.vlen_in ? min(p.L, p.vlen_in[b]) : p.L;      // ragged batch: the input reads as zeros from Lin on ...
    const int Lout = p.vlen ? min(p.To, p.vlen[b]) : p.To;         // ... and the output is zeros from Lout on
    float wv[NW], xv[NX];
    auto load = [&](int k0) {
        const int kg = k0 + kk;
        const bool kin = kg < Kd;
        const int ci = kin ? kg / p.K : 0;
        const int tap = kg - ci * p.K;
        const float* xr = xb + (long long)ci * p.L;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int co = co0 + r0 + 8 * i;
            wv[i] = (kin && co < p.Co) ? p.w[(long long)co * Kd + kg] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int t = t0 + r0 + 8 * i;
            const long long s = (long long)t * p.stride - p.pad + tap;
            float v = (kin && t < p.To && s >= 0 && s < Lin) ? xr[s] : 0.f;
            xv[i] = v >= 0.f ? v : v * p.slope;
        }
    };
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (t0 < Lout) load(0);
    for (int k0 = 0; t0 < Lout && k0 < Kd; k0 += kDownKC) {      // (t0 >= Lout: every column of the tile is padding; only zeros are stored)
#pragma unroll
        for (int i = 0; i < NW; ++i) Ws[kk * SW + r0 + 8 * i] = wv[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) Xs[kk * SX + r0 + 8 * i] = xv[i];
        __syncthreads();
        if (k0 + kDownKC < Kd) load(k0 + kDownKC);
#pragma unroll 4
        for (int kp = 0; kp < kDownKC / 2; ++kp) {
            const int row = 2 * kp + h;
            float a[WM], bb[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) a[i] = Ws[row * SW + (wm * WM + i) * 32 + c];
#pragma unroll
            for (int j = 0; j < WN; ++j) bb[j] = Xs[row * SX + (wn * WN + j) * 32 + c];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int t = t0 + (wn * WN + j) * 32 + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * WM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < p.Co && t < p.To) p.out[((long long)b * p.Co + co) * p.To + t] = t < Lout ? acc[i][j][r] + (p.bias ? p.bias[co] : 0.f) : 0.f;
            }
        }
}

static thread_local char g_down_cfg[64] = "";
const char* conv_down_last_config() { return g_down_cfg; }

static int device_cus() {
    static std::atomic<int> cus{0};
    int n = cus.load(std::memory_order_relaxed);
    if (n == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus.store(n, std::memory_order_relaxed);
    }
    return n;
}

template <int WM, int WN>
static hipError_t launch_down_cfg(const ConvDownArgs& a, hipStream_t s) {
    const dim3 grid((a.To + 64 * WN - 1) / (64 * WN), (a.Co + 64 * WM - 1) / (64 * WM), a.B);
    snprintf(g_down_cfg, sizeof(g_down_cfg), "BM%d BN%d grid %u", 64 * WM, 64 * WN, grid.x * grid.y * grid.z);
    hipLaunchKernelGGL((conv_down_kernel<WM, WN>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conv_down(const ConvDownArgs& a, hipStream_t s) {
    if (!a.x || !a.w || !a.out || a.Ci < 1 || a.Co < 1 || a.K < 1 || a.stride < 1 || a.pad < 0 || a.L < 1 || a.To < 1 || a.B < 1 || a.B > 65535)
        return hipErrorInvalidValue;
    if ((long long)a.To > ((long long)a.L + 2 * a.pad - a.K) / a.stride + 1) return hipErrorInvalidValue;
    if ((long long)a.Co > 65535 * 64) return hipErrorInvalidValue;
    switch (a.tile) {
        case 0: break;
        case 128128: return launch_down_cfg<2, 2>(a, s);
        case 64128: return launch_down_cfg<1, 2>(a, s);
        case 64064: return launch_down_cfg<1, 1>(a, s);
        default: return hipErrorInvalidValue;
    }
    // the largest tile that still gives every CU two workgroups (one when even that is not reached: the 64 x 64 tile)
    const long long cus = device_cus();
    auto blocks = [&](int bm, int bn) { return (long long)((a.Co + bm - 1) / bm) * ((a.To + bn - 1) / bn) * a.B; };
    if (a.Co > 64 && blocks(128, 128) >= 2 * cus) return launch_down_cfg<2, 2>(a, s);
    if (blocks(64, 128) >= cus) return launch_down_cfg<1, 2>(a, s);
    return launch_down_cfg<1, 1>(a, s);
}

// one thread per (b, t, c), c fastest: the [B][T][2C] / [B][T][C] stores are coalesced; z's product and sum are rounded separately,
// like the reference's three eager ops (randn_like(m) * exp(logs), then + m); ragged batch: rows t >= tlen[b] are written as zeros
__global__ void __launch_bounds__(256) vae_head_kernel(const float* __restrict__ y, const float* __restrict__ noise, float* __restrict__ out,
                                                       float* __restrict__ z, int C, int T, int only_mean, long long n, const int* __restrict__ tlen) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % C);
        const long long bt = i / C;
        const int t = (int)(bt % T);
        const long long b = bt / T;
        if (tlen && t >= tlen[b]) {
            out[bt * 2 * C + ch] = 0.f;
            out[bt * 2 * C + C + ch] = 0.f;
            if (z) z[bt * C + ch] = 0.f;
            continue;
        }
        const float m = y[(b * 2 * C + ch) * T + t];
        const float lg = y[(b * 2 * C + C + ch) * T + t];
        out[bt * 2 * C + ch] = m;
        out[bt * 2 * C + C + ch] = only_mean ? 0.f : lg;
        if (z) z[bt * C + ch] = __fadd_rn(m, __fmul_rn(noise[(b * C + ch) * T + t], expf(lg)));
    }
}

hipError_t launch_vae_head(const float* y, const float* noise, float* out, float* z, int B, int C, int T, int only_mean, hipStream_t s, const int* tlen) {
    if (!y || !out || (z && !noise) || B < 1 || C < 1 || T < 1) return hipErrorInvalidValue;
    const long long n = (long long)B * T * C;
    const long long nb = std::min<long long>((n + 255) / 256, 65536);
    ProfScope ps(s, "vae_head", 2.0 * n, 4.0 * n * (z ? 5 : 4));
    hipLaunchKernelGGL(vae_head_kernel, dim3((unsigned)nb), dim3(256), 0, s, y, noise, out, z, C, T, only_mean, n, tlen);
    return hipGetLastError();
}

}  // namespace lds
