// Memory-bound companions of conv_dma over K4P activations (k4p.h): layout conversion at the UNet boundary,
// GroupNorm(+scale/shift)(+SiLU) and LayerNorm materialised ONCE per tensor (reference nn.GroupNorm / SiLU in
// resnet.py:591-641, transformer_1d.py:134,262; nn.LayerNorm in attention.py:83,102,118), nearest resampling.
// An 8-channel block of a K4P tensor is one contiguous run of 2*(T+2)*4 floats, so all of these stream 16-byte
// entries with unit stride; the GroupNorm statistics are per-block partials written by the producing convolution's
// epilogue and combined with Chan's formula in a fixed order, never atomics, so results do not depend on scheduling.
#include "k4p.h"
#include "gn_chan.h"
#include "kernels.h"

#include <hip/hip_ext.h>

#include <math.h>
#include <stdlib.h>

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// one workgroup per (b, 8-channel block)
__global__ void __launch_bounds__(256) to_k4p_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int T, int Ctot, int c_off, const int* __restrict__ lens) {
    const int q = blockIdx.x, b = blockIdx.y;
    const int Tp = T + 2, Tv = ragged_len(lens, b, 0, T);      // (ragged batch: zeros from the utterance's length on)
    float* ob = out + (((long long)b * (Ctot >> 3) + (c_off >> 3) + q) * 2) * Tp * 4;
    const float* ib = in + ((long long)b * C + q * 8) * T;
    for (int idx = threadIdx.x; idx < 2 * Tp; idx += 256) {
        const int hh = idx / Tp, e = idx - hh * Tp, t = e - 1;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < Tv) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ib[(long long)(2 * j + hh) * T + t];
        }
        *reinterpret_cast<f32x4*>(ob + (long long)idx * 4) = v;
    }
}
hipError_t launch_to_k4p(const float* in, float* out, int B, int C, int T, int Ctot, int c_off, hipStream_t s, const int* lens) {
    if ((C & 7) || (Ctot & 7) || (c_off & 7)) return hipErrorInvalidValue;
    ProfScope ps(s, "to_k4p", 0.0, 8.0 * B * (double)C * T);
    hipLaunchKernelGGL(to_k4p_kernel, dim3(C / 8, B), dim3(256), 0, s, in, out, C, T, Ctot, c_off, lens);
    return hipGetLastError();
}

// Vocoder entry into K4P: plain [B][C][T] -> K4P rows with `pad` zero frames per side (the dilated k 7 / 11 convolutions pad up to 25
// frames), the raw tensor (residual operand) and its LeakyReLU (what the convolutions read: reference models.py:186-192 applies
// F.leaky_relu before every conv, here once per tensor).  One workgroup per (8-channel block, 1024-frame slab, batch element).
__global__ void __launch_bounds__(256) to_k4p_act_kernel(const float* __restrict__ in, float* __restrict__ raw, float* __restrict__ act,
                                                         float slope, int C, int T, int pad, const int* __restrict__ vlen) {
    const int q = blockIdx.x, t0 = blockIdx.y * 1024, b = blockIdx.z;
    const int Tv = vlen ? vlen[b] : T;      // (ragged batch: zeros from the utterance's length on)
    const int Tp = T + 2 * pad;
    const long long ro = (((long long)b * (C >> 3) + q) * 2) * Tp * 4;
    const float* ib = in + ((long long)b * C + q * 8) * T;
    for (int idx = threadIdx.x; idx < 2 * 1024; idx += 256) {
        const int hh = idx >> 10, t = t0 + (idx & 1023);
        if (t >= T) continue;
        f32x4 v, a;
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = (t < Tv) ? ib[(long long)(2 * j + hh) * T + t] : 0.f; a[j] = (v[j] >= 0.f) ? v[j] : v[j] * slope; }
        const long long o = ro + ((long long)hh * Tp + t + pad) * 4;
        if (raw) *reinterpret_cast<f32x4*>(raw + o) = v;
        if (act) *reinterpret_cast<f32x4*>(act + o) = a;
    }
}
hipError_t launch_to_k4p_act(const float* in, float* raw, float* act, float slope, int B, int C, int T, int pad, hipStream_t s, const int* vlen) {
    if ((C & 7) || pad < 1) return hipErrorInvalidValue;
    ProfScope ps(s, "to_k4p_act", 0.0, 4.0 * B * (double)C * T * (1.0 + (raw ? 1.0 : 0.0) + (act ? 1.0 : 0.0)));
    hipLaunchKernelGGL(to_k4p_act_kernel, dim3(C / 8, (T + 1023) / 1024, B), dim3(256), 0, s, in, raw, act, slope, C, T, pad, vlen);
    return hipGetLastError();
}

// one workgroup per (b, 8-channel block): both rows' left and right pads
__global__ void __launch_bounds__(256) k4p_zero_pads_kernel(float* __restrict__ x, int T, int pad) {
    const int Tp = T + 2 * pad;
    float* xb = x + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * Tp * 4;
    for (int idx = threadIdx.x; idx < 4 * pad; idx += 256) {
        const int hh = idx / (2 * pad), e = idx - hh * 2 * pad;
        const int entry = (e < pad) ? e : T + e;                      // left pad entries 0..pad-1, right pad entries T+pad..T+2pad-1
        *reinterpret_cast<f32x4*>(xb + ((long long)hh * Tp + entry) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
hipError_t launch_k4p_zero_pads(float* x, int B, int C, int T, int pad, hipStream_t s) {
    if ((C & 7) || pad < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k4p_zero_pads_kernel, dim3(C / 8, B), dim3(256), 0, s, x, T, pad);
    return hipGetLastError();
}

// test support (lds_test_wino_conv): NaN / Inf into both pad frames of every row and into the frames at and beyond the utterance's length
__global__ void __launch_bounds__(256) k4p_poison_kernel(float* __restrict__ x, int T, const int* __restrict__ lens) {
    const int Tp = T + 2, Tv = ragged_len(lens, blockIdx.y, 0, T);
    float* xb = x + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * Tp * 4;
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    for (int idx = threadIdx.x; idx < 2 * Tp; idx += 256) {
        const int hh = idx / Tp, e = idx - hh * Tp;
        if (e == 0 || e > Tv) *reinterpret_cast<f32x4*>(xb + (long long)idx * 4) = f32x4{nan, inf, -inf, nan};
    }
}
hipError_t launch_k4p_poison(float* x, int B, int C, int T, const int* lens, hipStream_t s) {
    if (C & 7) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k4p_poison_kernel, dim3(C / 8, B), dim3(256), 0, s, x, T, lens);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) from_k4p_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int T) {
    const int q = blockIdx.x, b = blockIdx.y;
    const int Tp = T + 2;
    const float* ib = in + (((long long)b * (C >> 3) + q) * 2) * Tp * 4;
    float* ob = out + ((long long)b * C + q * 8) * T;
    for (int idx = threadIdx.x; idx < 2 * T; idx += 256) {
        const int hh = idx / T, t = idx - hh * T;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ib + ((long long)hh * Tp + t + 1) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[(long long)(2 * j + hh) * T + t] = v[j];
    }
}
// K4P with `pad` frames per side -> plain [B][C][T] (test entry points of the vocoder path)
__global__ void __launch_bounds__(256) from_k4p_pad_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int T, int pad) {
    const int q = blockIdx.x, b = blockIdx.y;
    const int Tp = T + 2 * pad;
    const float* ib = in + (((long long)b * (C >> 3) + q) * 2) * Tp * 4;
    float* ob = out + ((long long)b * C + q * 8) * T;
    for (int idx = threadIdx.x; idx < 2 * T; idx += 256) {
        const int hh = idx / T, t = idx - hh * T;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ib + ((long long)hh * Tp + t + pad) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[(long long)(2 * j + hh) * T + t] = v[j];
    }
}
hipError_t launch_from_k4p_pad(const float* in, float* out, int B, int C, int T, int pad, hipStream_t s) {
    if (C & 7) return hipErrorInvalidValue;
    hipLaunchKernelGGL(from_k4p_pad_kernel, dim3(C / 8, B), dim3(256), 0, s, in, out, C, T, pad);
    return hipGetLastError();
}
hipError_t launch_from_k4p(const float* in, float* out, int B, int C, int T, hipStream_t s) {
    if (C & 7) return hipErrorInvalidValue;
    hipLaunchKernelGGL(from_k4p_kernel, dim3(C / 8, B), dim3(256), 0, s, in, out, C, T);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) plain_to_vt_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int T, int D) {
    const int ch = blockIdx.x, b = blockIdx.y;
    const int T4 = (T + 3) & ~3, head = ch / D, d = ch - head * D;
    const float* ib = in + ((long long)b * C + ch) * T;
    float* ob = out + ((long long)b * C + (long long)head * D) * T4 + d * 4;
    for (int n = threadIdx.x; n < T4; n += 256) ob[(long long)(n >> 2) * D * 4 + (n & 3)] = (n < T) ? ib[n] : 0.f;
}
hipError_t launch_plain_to_vt(const float* in, float* out, int B, int C, int T, int D, hipStream_t s) {
    if (D <= 0 || C % D) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plain_to_vt_kernel, dim3(C, B), dim3(256), 0, s, in, out, C, T, D);
    return hipGetLastError();
}

// ---- GroupNorm -------------------------------------------------------------------------------------------------
// Statistics travel as (mean, M2) partials of (16 channels x 32 frames) blocks, [B][C/16][ceil(T/32)] float2.  conv_dma
// writes them from its epilogue for every tensor that feeds a GroupNorm (DmaConvArgs::gnpart_out); gn_partials_kernel
// computes the same from a K4P tensor (stand-alone entry points).  gn_stream_kernel is the only pass over the tensor.

// Wave64 reduction helpers in a fixed order (DPP row shifts + row broadcasts): the result is valid in lane 63.
static __device__ __forceinline__ float wave_sum_to_lane63(float v) {
    v += dpp_get<0x111, 0xf, true>(v);
    v += dpp_get<0x112, 0xf, true>(v);
    v += dpp_get<0x114, 0xf, true>(v);
    v += dpp_get<0x118, 0xf, true>(v);
    v += dpp_get<0x142, 0xa, false>(v);
    v += dpp_get<0x143, 0xc, false>(v);
    return v;
}
// one wave per (16-channel block, 32-frame block)
__global__ void __launch_bounds__(64) gn_partials_kernel(const float* __restrict__ x, int C, int T, float2* __restrict__ gp, const int* __restrict__ lens, int lvl) {
    const int nT = (T + 31) >> 5, kb = blockIdx.x / nT, tb = blockIdx.x - kb * nT, b = blockIdx.y, lane = threadIdx.x;
    const int Tp = T + 2, Tv = ragged_len(lens, b, lvl, T);      // (ragged batch: statistics over the utterance's own frames, as the convolutions' epilogues write them)
    const float* xb = x + (((long long)b * (C >> 3) + 2 * kb) * 2) * Tp * 4;      // 4 rows: (q = 2kb, 2kb+1) x (hh = 0, 1)
    const int t = tb * 32 + (lane & 31), half = lane >> 5;                          // each lane: two rows of one frame
    const bool ok = t < Tv;
    const float k = xb[(long long)(tb * 32 + 1) * 4];                               // element (row 0, first frame of the block, j = 0)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int row = half * 2 + rr;
        f32x4 v = {k, k, k, k};
        if (ok) v = *reinterpret_cast<const f32x4*>(xb + ((long long)row * Tp + t + 1) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = v[j] - k; s1 += d; s2 = fmaf(d, d, s2); }
    }
    s1 = wave_sum_to_lane63(s1);
    s2 = wave_sum_to_lane63(s2);
    const int nv = (Tv - tb * 32 < 32) ? Tv - tb * 32 : 32;
    if (lane == 63 && nv > 0) {      // (a block beyond the utterance's length has no partial: its slot is never read)
        const float cnt = 16.0f * (float)nv, rc = 1.0f / cnt;
        gp[((long long)b * (C >> 4) + kb) * nT + tb] = make_float2(k + s1 * rc, fmaxf(s2 - s1 * s1 * rc, 0.f));
    }
}
hipError_t launch_gn_partials(const float* x, int C, int T, float2* gp, int B, hipStream_t s, const int* lens, int lvl) {
    if (C & 15) return hipErrorInvalidValue;
    ProfScope ps(s, "gn_partials", 0.0, 4.0 * B * (double)C * T);
    hipLaunchKernelGGL(gn_partials_kernel, dim3((C / 16) * ((T + 31) / 32), B), dim3(64), 0, s, x, C, T, gp, lens, lvl);
    return hipGetLastError();
}

// One workgroup per (batch, 8-channel block).  Everything the launch needs is requested at its top, unconditionally, and waited for once:
// the group's first two rounds of partials, E x 256 entries of 16 bytes of the tensor, and the block's eight gamma / beta / scale / shift
// values as four 32-byte scalar loads (the eight channels of a block are contiguous in each array).  A load inside a branch is waited for at
// the end of that branch, so the masks are selects on the loaded values.  The statistics are combined while the tensor's entries are in
// flight (every wave does it redundantly: no LDS, no barrier), then normalise + affine (+scale/shift) (+SiLU) and store; the pad frames
// are written as zeros.  cg16 = 16-channel blocks per group, (gm, gsh) = kernels.h dma_magic of the 8-channel blocks per group,
// inv_nT = 1 / ceil(T / 32): the launcher's, so that no division stands in front of the first load.
typedef float gn_f32x8 __attribute__((ext_vector_type(8)));
typedef float gn_f32x2 __attribute__((ext_vector_type(2)));
typedef gn_f32x8 gn_f32x8_a4 __attribute__((aligned(4)));
// eight consecutive floats as ONE scalar load (dword alignment is all the scalar unit asks for), through the constant address space: the
// arrays do not change during a launch, and so the read stays scalar behind the asm statement that pins the arguments
static __device__ __forceinline__ gn_f32x8 gn_load8(const float* p) {
    return *(const __attribute__((address_space(4))) gn_f32x8_a4*)(unsigned long long)p;
}
template <int E>
__global__ void __launch_bounds__(256) gn_stream_kernel(const float* __restrict__ x1, const float* __restrict__ x2, int C1, int C2, int T,
                                                        int cg16, unsigned gm, unsigned gsh, float inv_nT, float eps,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ ss, int ss_stride, int ss_off, int silu,
                                                        const float2* __restrict__ gp1, const float2* __restrict__ gp2, float* __restrict__ y,
                                                        const int* __restrict__ lens, int lvl) {
    // the arguments in one burst behind one wait (conv_dma.hip load_hot): one empty asm that names them all
    asm volatile("" : "+s"(x1), "+s"(x2), "+s"(C1), "+s"(C2), "+s"(T), "+s"(cg16), "+s"(gm), "+s"(gsh), "+s"(inv_nT), "+s"(eps), "+s"(gamma), "+s"(beta),
                      "+s"(ss), "+s"(ss_stride), "+s"(ss_off), "+s"(silu), "+s"(gp1), "+s"(gp2), "+s"(y), "+s"(lens), "+s"(lvl));
    const int q = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int C = C1 + C2, Tp = T + 2, nq1 = C1 >> 3, nq = C >> 3;
    // ---- 1. the scalar requests: the block's eight gamma / beta / scale / shift values (channels 8q .. 8q + 7 of each array; without
    // scale/shift the two extra loads re-read gamma) and the utterance's length ----
    const float* sp = ss ? ss + (long long)b * ss_stride + ss_off + q * 8 : gamma + q * 8;
    const gn_f32x8 g8 = gn_load8(gamma + q * 8), b8 = gn_load8(beta + q * 8), sc8 = gn_load8(sp), sh8 = gn_load8(ss ? sp + C : sp);
    int Tv = T;      // ragged batch (k4p.h ragged_len): statistics over, and output for, the utterance's own frames; zeros beyond
    if (lens) {
        int n = ((const __attribute__((address_space(4))) int*)(unsigned long long)lens)[b];
        asm volatile("" : "+s"(n));
        for (int i = 0; i < lvl; ++i) n = (n - 1) / 2 + 1;
        Tv = n < T ? n : T;
    }
    const float* xb = (q < nq1) ? x1 + (((long long)b * nq1 + q) * 2) * Tp * 4 : x2 + (((long long)b * (C2 >> 3) + (q - nq1)) * 2) * Tp * 4;
    float* yb = y + (((long long)b * nq + q) * 2) * Tp * 4;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, 2 * Tp * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(yb, 0, 2 * Tp * 16, 0x00020000);
    const int total = 2 * T;                          // real entries of this block: (row hh, frame t) -> idx = hh * T + t
    // ---- 2. request the partials of the first two rounds (<= 128: every shape of the UNet at T <= 1024), in front of the tensor's entries:
    // vmcnt completes in order, and the statistics are the launch's critical path ----
    const int g = (int)dma_magic_div((unsigned)q, gm, gsh);      // the block's group: q / (2 cg16)
    const int nT = (T + 31) >> 5, P = cg16 * nT, nk1 = C1 >> 4;
    // an empty partial (beyond the group's last, or a block beyond the utterance's length, whose partials were never written) is (0, 0, 0);
    // its load reads the group's first partial, a valid address (gn_chan.h gn_part_load)
    auto request = [&](int p0, float& nb, bool& ok) {      // the load, this lane's count and whether the partial takes part
        const int pi = p0 + lane;
        const bool in = pi < P;
        const int pc = in ? pi : 0;
        const int kk = (int)(((float)pc + 0.5f) * inv_nT), tb = pc - kk * nT, kb = g * cg16 + kk;      // pc / nT without the integer-division sequence
        const int nv = (Tv - tb * 32 < 32) ? Tv - tb * 32 : 32;
        const bool f1 = kb < nk1;      // which source's partials (selects of scalars; global pointers again behind the asm above)
        const int off = ((f1 ? b * nk1 : b * (C2 >> 4) - nk1) + kb) * nT + tb;
        ok = in && nv > 0;
        nb = ok ? 16.0f * (float)nv : 0.f;
        return ((const __attribute__((address_space(1))) gn_f32x2*)(unsigned long long)(f1 ? gp1 : gp2))[off];
    };
    auto part = [&](int p0, float& nb, float& mb, float& qb) {
        bool ok;
        const gn_f32x2 pr = request(p0, nb, ok);
        mb = ok ? pr.x : 0.f; qb = ok ? pr.y : 0.f;
    };
    float n0, n1;
    bool ok0, ok1;
    gn_f32x2 pr0 = request(0, n0, ok0), pr1 = request(64, n1, ok1);
    // ---- 3. request the first chunk (an entry beyond the block reads the pad frame or, by the buffer's range check, nothing) ----
    auto entry = [&](int idx) {
        const int hh = idx >= T, t = idx - hh * T;
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (hh * Tp + t + 1) * 16, 0, 0));
    };
    f32x4 v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = entry(tid + 256 * i);
    asm volatile("" : "+v"(pr0), "+v"(pr1));      // both rounds behind one counted wait (the entries stay in flight)
    const float m0 = ok0 ? pr0.x : 0.f, q0 = ok0 ? pr0.y : 0.f, m1 = ok1 ? pr1.x : 0.f, q1 = ok1 ? pr1.y : 0.f;
    float ga[2][4], be[2][4];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float g_ = g8[2 * j + hh], b_ = b8[2 * j + hh];
            if (ss) {
                const float sc = 1.0f + sc8[2 * j + hh];
                g_ *= sc;
                b_ = fmaf(b_, sc, sh8[2 * j + hh]);      // (the roundings are spelled out where the compiler had contracted: results stay bit for bit)
            }
            ga[hh][j] = g_; be[hh][j] = b_;
        }
    // ---- 4. group statistics from the partials ----
    // two plain sums in a fixed order (gn_chan.h gnf_wave_sum): mean = sum(n_i mean_i) / N, var = sum(M2_i + n_i (mean_i - mean)^2) / N with
    // N = 16 cg16 Tv known outright -- a dependent chain of 2 x 6 additions where the Chan tree had 6 steps of a dozen operations with a
    // reciprocal each, on the critical path of a launch that is latency-bound (DESIGN.md sections 3.10, 14.10).  The partials of the first
    // two rounds stay in registers between the sums; further rounds are read twice, each with its own wait.
    float s1 = fmaf(n1, m1, __fmul_rn(n0, m0));
    for (int p0 = 128; p0 < P; p0 += 64) {
        float nb, mb, qb;
        part(p0, nb, mb, qb);
        s1 = fmaf(nb, mb, s1);
    }
    const float rN = __builtin_amdgcn_rcpf(16.0f * (float)cg16 * (float)Tv);
    const float mu = __fmul_rn(gnf_wave_sum(s1), rN);
    const float d0 = __fsub_rn(m0, mu), d1 = __fsub_rn(m1, mu);
    float s2 = __fadd_rn(fmaf(__fmul_rn(n0, d0), d0, q0), fmaf(__fmul_rn(n1, d1), d1, q1));      // (an empty partial carries n = 0, mean = 0, M2 = 0)
    for (int p0 = 128; p0 < P; p0 += 64) {
        float nb, mb, qb;
        part(p0, nb, mb, qb);
        const float d = __fsub_rn(mb, mu);
        s2 = __fadd_rn(s2, fmaf(__fmul_rn(nb, d), d, qb));
    }
    const float rstd = __builtin_amdgcn_rsqf(fmaf(gnf_wave_sum(s2), rN, eps));      // var = sum * rN, + eps in one rounding
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int j = 0; j < 4; ++j) ga[hh][j] *= rstd;
    // ---- 5. normalise and store ----
    if (tid < 4) {                                    // the four pad entries (frames -1 and T of both rows)
        const int hh = tid >> 1, e = (tid & 1) ? T + 1 : 0;
        k4p_store16(ry, (hh * Tp + e) * 16, k4p_f32x4{0.f, 0.f, 0.f, 0.f});
    }
    for (int base = 0; base < total; base += 256 * E) {
        if (base > 0) {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = entry(base + tid + 256 * i);
        }
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int idx = base + tid + 256 * i;
            if (idx < total) {
                const int hh = idx >= T, t = idx - hh * T;
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float r = fmaf(v[i][j] - mu, hh ? ga[1][j] : ga[0][j], hh ? be[1][j] : be[0][j]);
                    if (silu) r = r * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(r * -1.4426950408889634f));
                    o[j] = (t < Tv) ? r : 0.f;
                }
                // write-through 16-byte store (sc1): no dirty lines left for the end-of-kernel write-back (k4p.h, k4p_store_wt)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ry, (int)(((long long)hh * Tp + t + 1) * 16), 0, 16);
            }
        }
    }
}

hipError_t launch_gn_stream(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                            const float* beta, const float* ss, int ss_stride, int ss_off, int silu, const float2* gp1, const float2* gp2,
                            float* y, int B, hipStream_t s, const int* lens, int lvl) {
    const int C = C1 + C2;
    if ((C1 & 15) || (C2 & 15) || groups <= 0 || C % groups || (C / groups) % 16 || !gp1 || (C2 && !gp2)) return hipErrorInvalidValue;
    ProfScope ps(s, "gn_stream", 0.0, 4.0 * 2.0 * B * (double)C * T, true);
    const dim3 grid(C / 8, B), blk(256);
    const int need = (2 * T + 255) / 256;
    // channels per group and the group of a block, for the kernel's scalar unit: 16-channel blocks per group, and the divisor "8-channel
    // blocks per group" as a multiplier / shift pair (kernels.h dma_magic); 1 / ceil(T / 32) for its partial-index arithmetic
    const int cg16 = (C / groups) >> 4;
    const DmaMagic gmg = dma_magic((unsigned)(2 * cg16));
    const float inv_nT = 1.0f / (float)((T + 31) >> 5);
#define GN_ARGS x1, x2 ? x2 : x1, C1, C2, T, cg16, gmg.m, gmg.s, inv_nT, eps, gamma, beta, ss, ss_stride, ss_off, silu, gp1, gp2 ? gp2 : gp1, y, lens, lvl
    hipEvent_t e0, e1;
    if (prof_attach_events(&e0, &e1)) {      // bench.py's instrumented step: the events ride in the dispatch
        if (need <= 1) hipExtLaunchKernelGGL(gn_stream_kernel<1>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
        else if (need <= 2) hipExtLaunchKernelGGL(gn_stream_kernel<2>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
        else hipExtLaunchKernelGGL(gn_stream_kernel<4>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
    } else if (need <= 1) hipLaunchKernelGGL(gn_stream_kernel<1>, grid, blk, 0, s, GN_ARGS);
    else if (need <= 2) hipLaunchKernelGGL(gn_stream_kernel<2>, grid, blk, 0, s, GN_ARGS);
    else hipLaunchKernelGGL(gn_stream_kernel<4>, grid, blk, 0, s, GN_ARGS);
#undef GN_ARGS
    return hipGetLastError();
}

// gn_stream_kernel with the Winograd F(2,3) input transform behind it (conv_wino.hip; kernels.h launch_gn_wino).  The prologue -- scalar
// requests, partials, statistics -- is gn_stream_kernel's, statement for statement, and so is the arithmetic of d = act(GroupNorm(x)): the
// values that enter the transform are bit for bit what gn_stream writes.  A work item is one frame pair i of one row: it loads the row's
// entries of frames 2i-1 .. 2i+2 (the padded input d[2i .. 2i+3]: four 16-byte loads where gn_stream has two per pair, no second pass and
// no exchange across waves), forms d at the four frames -- zero outside [0, Tv) by selects on the computed values, so whatever the pad frames or the frames beyond an
// utterance's length hold never reaches a plane -- and stores one 16-byte entry into each plane:
//   V0 = d[2i] - d[2i+2], V1 = d[2i+1] + d[2i+2], V2 = d[2i+2] - d[2i+1], V3 = d[2i+1] - d[2i+3]      y: [B][C/8][2][4][P][4], P = ceil(T / 2)
//
// PAIR (the conv2 + shortcut launch of a resnet, model.hip run_wconv_pair): the output's batch stride is the caller's -- the planes are the
// first C / 8 blocks of a longer plane tensor -- and, where `side` is given, the pass also writes the shortcut's operand planes from the RAW
// entries it already holds at frames 2i and 2i+1 (x_e, x_o; zero from the utterance's length on, by select): block q of the first half of the
// C / 8 blocks writes planes 0 and 3 of side block q (x_e, x_o), block q of the second half planes 1 and 2 of side block q - C / 16
// (x_e + x_o, x_e - x_o: one fp32 operation each).  Without PAIR the body is gn_wino_kernel's as it was.
template <int E, bool PAIR>
static __device__ __forceinline__ void gn_wino_body(const float* __restrict__ x1, const float* __restrict__ x2, int C1, int C2, int T, int cg16, unsigned gm,
                                                    unsigned gsh, float inv_nT, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    const float* __restrict__ ss, int ss_stride, int ss_off, int silu, const float2* __restrict__ gp1,
                                                    const float2* __restrict__ gp2, float* __restrict__ y, const int* __restrict__ lens, int lvl,
                                                    long long y_bstride, float* __restrict__ side, long long side_bstride) {
    const int q = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int C = C1 + C2, Tp = T + 2, nq1 = C1 >> 3, nq = C >> 3, Pn = (T + 1) >> 1;
    const float* sp = ss ? ss + (long long)b * ss_stride + ss_off + q * 8 : gamma + q * 8;
    const gn_f32x8 g8 = gn_load8(gamma + q * 8), b8 = gn_load8(beta + q * 8), sc8 = gn_load8(sp), sh8 = gn_load8(ss ? sp + C : sp);
    int Tv = T;
    if (lens) {
        int n = ((const __attribute__((address_space(4))) int*)(unsigned long long)lens)[b];
        asm volatile("" : "+s"(n));
        for (int i = 0; i < lvl; ++i) n = (n - 1) / 2 + 1;
        Tv = n < T ? n : T;
    }
    const float* xb = (q < nq1) ? x1 + (((long long)b * nq1 + q) * 2) * Tp * 4 : x2 + (((long long)b * (C2 >> 3) + (q - nq1)) * 2) * Tp * 4;
    float* yb = PAIR ? y + (long long)b * y_bstride + (long long)q * 2 * 4 * Pn * 4 : y + (((long long)b * nq + q) * 2) * 4 * Pn * 4;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, 2 * Tp * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(yb, 0, 2 * 4 * Pn * 16, 0x00020000);
    // the side block of this block (a launch without side output gets a buffer of zero bytes: its stores are dropped, and none is issued)
    const bool side_a = q < (nq >> 1);
    __amdgpu_buffer_rsrc_t rs = ry;
    if constexpr (PAIR)
        rs = __builtin_amdgcn_make_buffer_rsrc(side ? side + (long long)b * side_bstride + (long long)(side_a ? q : q - (nq >> 1)) * 2 * 4 * Pn * 4 : side, 0,
                                               side ? 2 * 4 * Pn * 16 : 0, 0x00020000);
    const int total = 2 * Pn;                         // work items of this block: (row hh, pair i) -> idx = hh * Pn + i
    const int g = (int)dma_magic_div((unsigned)q, gm, gsh);
    const int nT = (T + 31) >> 5, P = cg16 * nT, nk1 = C1 >> 4;
    auto request = [&](int p0, float& nb, bool& ok) {
        const int pi = p0 + lane;
        const bool in = pi < P;
        const int pc = in ? pi : 0;
        const int kk = (int)(((float)pc + 0.5f) * inv_nT), tb = pc - kk * nT, kb = g * cg16 + kk;
        const int nv = (Tv - tb * 32 < 32) ? Tv - tb * 32 : 32;
        const bool f1 = kb < nk1;
        const int off = ((f1 ? b * nk1 : b * (C2 >> 4) - nk1) + kb) * nT + tb;
        ok = in && nv > 0;
        nb = ok ? 16.0f * (float)nv : 0.f;
        return ((const __attribute__((address_space(1))) gn_f32x2*)(unsigned long long)(f1 ? gp1 : gp2))[off];
    };
    auto part = [&](int p0, float& nb, float& mb, float& qb) {
        bool ok;
        const gn_f32x2 pr = request(p0, nb, ok);
        mb = ok ? pr.x : 0.f; qb = ok ? pr.y : 0.f;
    };
    float n0, n1;
    bool ok0, ok1;
    gn_f32x2 pr0 = request(0, n0, ok0), pr1 = request(64, n1, ok1);
    // entry of frame 2i - 1 + f of the item's row = entry 2i + f of the padded row (frame -1 is the left pad frame; a frame beyond the row
    // reads the right pad frame or the next row: the selects below never let such a value through)
    auto entry = [&](int idx, int f) {
        const int hh = idx >= Pn, i = idx - hh * Pn;
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (hh * Tp + 2 * i + f) * 16, 0, 0));
    };
    f32x4 v[E][4];
#pragma unroll
    for (int i = 0; i < E; ++i)
#pragma unroll
        for (int f = 0; f < 4; ++f) v[i][f] = entry(tid + 256 * i, f);
    asm volatile("" : "+v"(pr0), "+v"(pr1));
    const float m0 = ok0 ? pr0.x : 0.f, q0 = ok0 ? pr0.y : 0.f, m1 = ok1 ? pr1.x : 0.f, q1 = ok1 ? pr1.y : 0.f;
    float ga[2][4], be[2][4];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float g_ = g8[2 * j + hh], b_ = b8[2 * j + hh];
            if (ss) {
                const float sc = 1.0f + sc8[2 * j + hh];
                g_ *= sc;
                b_ = fmaf(b_, sc, sh8[2 * j + hh]);
            }
            ga[hh][j] = g_; be[hh][j] = b_;
        }
    float s1 = fmaf(n1, m1, __fmul_rn(n0, m0));
    for (int p0 = 128; p0 < P; p0 += 64) {
        float nb, mb, qb;
        part(p0, nb, mb, qb);
        s1 = fmaf(nb, mb, s1);
    }
    const float rN = __builtin_amdgcn_rcpf(16.0f * (float)cg16 * (float)Tv);
    const float mu = __fmul_rn(gnf_wave_sum(s1), rN);
    const float d0 = __fsub_rn(m0, mu), d1 = __fsub_rn(m1, mu);
    float s2 = __fadd_rn(fmaf(__fmul_rn(n0, d0), d0, q0), fmaf(__fmul_rn(n1, d1), d1, q1));
    for (int p0 = 128; p0 < P; p0 += 64) {
        float nb, mb, qb;
        part(p0, nb, mb, qb);
        const float d = __fsub_rn(mb, mu);
        s2 = __fadd_rn(s2, fmaf(__fmul_rn(nb, d), d, qb));
    }
    const float rstd = __builtin_amdgcn_rsqf(fmaf(gnf_wave_sum(s2), rN, eps));
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int j = 0; j < 4; ++j) ga[hh][j] *= rstd;
    for (int base = 0; base < total; base += 256 * E) {
        if (base > 0) {
#pragma unroll
            for (int i = 0; i < E; ++i)
#pragma unroll
                for (int f = 0; f < 4; ++f) v[i][f] = entry(base + tid + 256 * i, f);
        }
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int idx = base + tid + 256 * i;
            if (idx < total) {
                const int hh = idx >= Pn, pi = idx - hh * Pn;
                f32x4 d[4];
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const int t = 2 * pi - 1 + f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float r = fmaf(v[i][f][j] - mu, hh ? ga[1][j] : ga[0][j], hh ? be[1][j] : be[0][j]);
                        if (silu) r = r * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(r * -1.4426950408889634f));
                        d[f][j] = (t >= 0 && t < Tv) ? r : 0.f;
                    }
                }
                const f32x4 pl[4] = {d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pl[j]), ry, ((hh * 4 + j) * Pn + pi) * 16, 0, 16);
                if constexpr (PAIR) {
                    if (side) {
                        f32x4 xe, xo;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            xe[j] = (2 * pi < Tv) ? v[i][1][j] : 0.f;
                            xo[j] = (2 * pi + 1 < Tv) ? v[i][2][j] : 0.f;
                        }
                        const f32x4 sa = side_a ? xe : xe + xo, sb = side_a ? xo : xe - xo;
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sa), rs, ((hh * 4 + (side_a ? 0 : 1)) * Pn + pi) * 16, 0, 16);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sb), rs, ((hh * 4 + (side_a ? 3 : 2)) * Pn + pi) * 16, 0, 16);
                    }
                }
            }
        }
    }
}

#define GN_WINO_PARAMS                                                                                                                               \
    const float *__restrict__ x1, const float *__restrict__ x2, int C1, int C2, int T, int cg16, unsigned gm, unsigned gsh, float inv_nT, float eps, \
        const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ ss, int ss_stride, int ss_off, int silu,         \
        const float2 *__restrict__ gp1, const float2 *__restrict__ gp2, float *__restrict__ y, const int *__restrict__ lens, int lvl
#define GN_WINO_PIN                                                                                                                                        \
    asm volatile("" : "+s"(x1), "+s"(x2), "+s"(C1), "+s"(C2), "+s"(T), "+s"(cg16), "+s"(gm), "+s"(gsh), "+s"(inv_nT), "+s"(eps), "+s"(gamma), "+s"(beta), \
                      "+s"(ss), "+s"(ss_stride), "+s"(ss_off), "+s"(silu), "+s"(gp1), "+s"(gp2), "+s"(y), "+s"(lens), "+s"(lvl))
#define GN_WINO_PASS x1, x2, C1, C2, T, cg16, gm, gsh, inv_nT, eps, gamma, beta, ss, ss_stride, ss_off, silu, gp1, gp2, y, lens, lvl
template <int E>
__global__ void __launch_bounds__(256) gn_wino_kernel(GN_WINO_PARAMS) {
    GN_WINO_PIN;
    gn_wino_body<E, false>(GN_WINO_PASS, 0, nullptr, 0);
}
template <int E>
__global__ void __launch_bounds__(256) gn_wino_pair_kernel(GN_WINO_PARAMS, long long y_bstride, float* __restrict__ side, long long side_bstride) {
    GN_WINO_PIN;
    asm volatile("" : "+s"(y_bstride), "+s"(side), "+s"(side_bstride));
    gn_wino_body<E, true>(GN_WINO_PASS, y_bstride, side, side_bstride);
}
#undef GN_WINO_PARAMS
#undef GN_WINO_PIN
#undef GN_WINO_PASS

hipError_t launch_gn_wino(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma, const float* beta,
                          const float* ss, int ss_stride, int ss_off, int silu, const float2* gp1, const float2* gp2, float* y, int B, hipStream_t s,
                          const int* lens, int lvl) {
    const int C = C1 + C2;
    if ((C1 & 15) || (C2 & 15) || groups <= 0 || C % groups || (C / groups) % 16 || !gp1 || (C2 && !gp2)) return hipErrorInvalidValue;
    const int Pn = (T + 1) / 2;
    ProfScope ps(s, "gn_wino", 0.0, 4.0 * B * (double)C * (T + 4.0 * Pn), true);
    const dim3 grid(C / 8, B), blk(256);
    const int need = (2 * Pn + 255) / 256;
    const int cg16 = (C / groups) >> 4;
    const DmaMagic gmg = dma_magic((unsigned)(2 * cg16));
    const float inv_nT = 1.0f / (float)((T + 31) >> 5);
#define GN_ARGS x1, x2 ? x2 : x1, C1, C2, T, cg16, gmg.m, gmg.s, inv_nT, eps, gamma, beta, ss, ss_stride, ss_off, silu, gp1, gp2 ? gp2 : gp1, y, lens, lvl
    hipEvent_t e0, e1;
    if (prof_attach_events(&e0, &e1)) {
        if (need <= 1) hipExtLaunchKernelGGL(gn_wino_kernel<1>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
        else if (need <= 2) hipExtLaunchKernelGGL(gn_wino_kernel<2>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
        else hipExtLaunchKernelGGL(gn_wino_kernel<4>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
    } else if (need <= 1) hipLaunchKernelGGL(gn_wino_kernel<1>, grid, blk, 0, s, GN_ARGS);
    else if (need <= 2) hipLaunchKernelGGL(gn_wino_kernel<2>, grid, blk, 0, s, GN_ARGS);
    else hipLaunchKernelGGL(gn_wino_kernel<4>, grid, blk, 0, s, GN_ARGS);
#undef GN_ARGS
    return hipGetLastError();
}

hipError_t launch_gn_wino_pair(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma, const float* beta,
                               const float* ss, int ss_stride, int ss_off, int silu, const float2* gp1, const float2* gp2, float* y, long long y_bstride,
                               float* side, long long side_bstride, int B, hipStream_t s, const int* lens, int lvl) {
    const int C = C1 + C2;
    if ((C1 & 15) || (C2 & 15) || groups <= 0 || C % groups || (C / groups) % 16 || !gp1 || (C2 && !gp2) || !y) return hipErrorInvalidValue;
    const int Pn = (T + 1) / 2;
    if (y_bstride < (long long)C * 4 * Pn || (side && side_bstride < (long long)(C / 2) * 4 * Pn)) return hipErrorInvalidValue;
    // conv1's pass keeps its name (one gn_wino per conv_wino) and counts the two side stores per item; conv2's pass is gn_wpair
    ProfScope ps(s, side ? "gn_wino" : "gn_wpair", 0.0, 4.0 * B * (double)C * (T + 4.0 * Pn + (side ? 2.0 * Pn : 0.0)), true);
    const dim3 grid(C / 8, B), blk(256);
    const int need = (2 * Pn + 255) / 256;
    const int cg16 = (C / groups) >> 4;
    const DmaMagic gmg = dma_magic((unsigned)(2 * cg16));
    const float inv_nT = 1.0f / (float)((T + 31) >> 5);
#define GN_ARGS                                                                                                                                  \
    x1, x2 ? x2 : x1, C1, C2, T, cg16, gmg.m, gmg.s, inv_nT, eps, gamma, beta, ss, ss_stride, ss_off, silu, gp1, gp2 ? gp2 : gp1, y, lens, lvl, \
        y_bstride, side, side_bstride
    hipEvent_t e0, e1;
    if (prof_attach_events(&e0, &e1)) {
        if (need <= 1) hipExtLaunchKernelGGL(gn_wino_pair_kernel<1>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
        else if (need <= 2) hipExtLaunchKernelGGL(gn_wino_pair_kernel<2>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
        else hipExtLaunchKernelGGL(gn_wino_pair_kernel<4>, grid, blk, 0, s, e0, e1, 0, GN_ARGS);
    } else if (need <= 1) hipLaunchKernelGGL(gn_wino_pair_kernel<1>, grid, blk, 0, s, GN_ARGS);
    else if (need <= 2) hipLaunchKernelGGL(gn_wino_pair_kernel<2>, grid, blk, 0, s, GN_ARGS);
    else hipLaunchKernelGGL(gn_wino_pair_kernel<4>, grid, blk, 0, s, GN_ARGS);
#undef GN_ARGS
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) resample_k4p_kernel(const float* __restrict__ in, float* __restrict__ out, int Tin, int Tout, int rows_per_b,
                                                           const int* __restrict__ lens, int lvl_in, int lvl_out) {
    const long long row = blockIdx.x;                // (b, q, hh) flattened
    const int b = (int)(row / rows_per_b);
    // ragged batch: every utterance is resampled from ITS input length to ITS output length (F.interpolate(size=) of the utterance alone)
    const int Ti = ragged_len(lens, b, lvl_in, Tin), To = ragged_len(lens, b, lvl_out, Tout);
    const float sc = (float)Ti / (float)To;
    const float* ib = in + row * (Tin + 2) * 4;
    float* ob = out + row * (Tout + 2) * 4;
    for (int e = threadIdx.x; e < Tout + 2; e += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (e >= 1 && e <= To) {
            int src = (int)floorf((float)(e - 1) * sc);
            if (src > Ti - 1) src = Ti - 1;
            v = *reinterpret_cast<const f32x4*>(ib + (long long)(src + 1) * 4);
        }
        *reinterpret_cast<f32x4*>(ob + (long long)e * 4) = v;
    }
}
hipError_t launch_resample_k4p(const float* in, float* out, int B, int C, int Tin, int Tout, hipStream_t s, const int* lens, int lvl_in, int lvl_out) {
    ProfScope ps(s, "resample", 0.0, 4.0 * B * (double)C * (Tin + Tout));
    hipLaunchKernelGGL(resample_k4p_kernel, dim3((unsigned)((long long)B * C / 4)), dim3(256), 0, s, in, out, Tin, Tout, C / 4, lens, lvl_in, lvl_out);
    return hipGetLastError();
}

}  // namespace lds
