// The WavLM units encoder's own kernels (transformers' WavLMModel); its gated-bias attention is attention_k4p.hip's attention_k4p_bias,
// everything else of that encoder is the launches that HuBERT and wav2vec 2.0 run (model.hip wavlm_run).  Exact fp32 (the waveform
// statistics in double), every reduction in a fixed order, no atomics.
//   wavlm_gate         gate[b][head][t] of one block's attention input (K4P): gru_rel_pos_linear + the two sigmoids of WavLMAttention.forward
//   wavlm_wave_stats   (mean, 1 / sqrt(var + 1e-7)) of every clip's own samples (Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm)
//   wavlm_wave_norm    the clip's samples normalised with them
#include "k4p.h"
#include "kernels.h"

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the gate of the relative position bias ----------------------------------------------------------------------------------------------
// p = W x_h + bias over the 64 channels of head h at frame t (W [8][64], shared by the heads); a = sigmoid(p0 + p1 + p2 + p3),
// b = sigmoid(p4 + .. + p7); gate = a (b const[h] - 1) + 2.  grid (ceil(T / 256), heads, B): a thread takes one frame of one head, i.e.
// the 16 K4P rows of that head at its frame (consecutive lanes consecutive frames: whole lines), and adds the channels in the rows'
// order.  Every weight address is uniform (scalar loads).  A frame at or beyond the clip's count reads nothing and gets gate 0.
__global__ void __launch_bounds__(256) wavlm_gate_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ cst, float* __restrict__ gate, const int* __restrict__ nlen, int C,
                                                         int T) {
    const int t = blockIdx.x * 256 + threadIdx.x, hd = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const int Tb = nlen ? (nlen[b] < T ? nlen[b] : T) : T;
    float g = 0.f;
    if (t < Tb) {
        float p[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) p[o] = bias[o];
        const float* xb = x + (((long long)b * (C >> 2) + hd * 16) * (T + 2) + t + 1) * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r) {      // K4P row r of the head: channels 8 (r / 2) + (r % 2) + 2 j
            const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (long long)r * (T + 2) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cl = 8 * (r >> 1) + (r & 1) + 2 * j;
#pragma unroll
                for (int o = 0; o < 8; ++o) p[o] = fmaf(w[o * 64 + cl], v[j], p[o]);
            }
        }
        const float a = 1.0f / (1.0f + expf(-((p[0] + p[1]) + (p[2] + p[3]))));
        const float bb = 1.0f / (1.0f + expf(-((p[4] + p[5]) + (p[6] + p[7]))));
        g = fmaf(a, fmaf(bb, cst[hd], -1.0f), 2.0f);
    }
    gate[((long long)b * gridDim.y + hd) * T + t] = g;
}

hipError_t launch_wavlm_gate(const float* x, const float* w, const float* bias, const float* cst, float* gate, const int* nlen, int B, int C, int T, int heads,
                             hipStream_t s) {
    if (B <= 0 || B > 65535 || heads < 1 || heads > 65535 || C != heads * 64 || T <= 0) return hipErrorInvalidValue;
    ProfScope ps(s, "wavlm_gate", 16.0 * B * (double)C * T, 4.0 * B * ((double)C * T + (double)heads * T));
    hipLaunchKernelGGL(wavlm_gate_kernel, dim3((T + 255) / 256, heads, B), dim3(256), 0, s, x, w, bias, cst, gate, nlen, C, T);
    return hipGetLastError();
}

// ---- waveform normalisation -------------------------------------------------------------------------------------------------------------
// One workgroup per clip, two passes in double (the exact mean first, then the squared deviations); a thread adds its samples in index
// order, the 1024 partial sums meet in LDS in a fixed tree.  stat[b] = (mean, 1 / sqrt(var + 1e-7)), var the biased variance.
static __device__ __forceinline__ double wavlm_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__global__ void __launch_bounds__(1024) wavlm_wave_stats_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L,
                                                                double2* __restrict__ stat) {
    __shared__ double red[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lb = slen ? slen[b] : (int)L;
    const float* ab = audio + (long long)b * L;
    double s1 = 0.0;
    for (int i = tid; i < Lb; i += 1024) s1 += (double)ab[i];
    const double mean = wavlm_block_sum(s1, red) / (double)Lb;
    double s2 = 0.0;
    for (int i = tid; i < Lb; i += 1024) { const double d = (double)ab[i] - mean; s2 += d * d; }
    const double var = wavlm_block_sum(s2, red) / (double)Lb;
    if (tid == 0) stat[b] = make_double2(mean, 1.0 / sqrt(var + 1e-7));
}
__global__ void __launch_bounds__(256) wavlm_wave_norm_kernel(const float* __restrict__ audio, const int* __restrict__ slen, long long L,
                                                              const double2* __restrict__ stat, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int Lb = slen ? slen[b] : (int)L;
    if (i >= Lb) return;
    const double2 st = stat[b];
    out[(long long)b * L + i] = (float)(((double)audio[(long long)b * L + i] - st.x) * st.y);
}

hipError_t launch_wavlm_wave_norm(const float* audio, const int* slen, long long L, double2* stat, float* out, int B, hipStream_t s) {
    if (B <= 0 || B > 65535 || L <= 0 || L > ((long long)1 << 30)) return hipErrorInvalidValue;
    ProfScope ps(s, "wavlm_wave_norm", 6.0 * B * (double)L, 16.0 * B * (double)L);
    hipLaunchKernelGGL(wavlm_wave_stats_kernel, dim3(B), dim3(1024), 0, s, audio, slen, L, stat);
    hipLaunchKernelGGL(wavlm_wave_norm_kernel, dim3((unsigned)((L + 255) / 256), B), dim3(256), 0, s, audio, slen, L, stat, out);
    return hipGetLastError();
}

}  // namespace lds
