// The small kernels around DiffusionSVC.infer_from_long_audio (reference tools/infer_tools.py:83-117): the slicer's frame RMS
// (tools/slicer.py:40, librosa.feature.rms), the volume and its mask (tools/tools.py:23-41, 225-229), the per-clip frame alignment and the
// masked cross-fading join (infer_tools.py:105-115, tools/tools.py:231-238).  fp32, gfx950.  Every one is bandwidth-trivial; what they buy is
// that the segments of a recording stay on the device from the audio to the waveform.  No atomics: each output is one thread's or one
// wave's sum in a fixed order, so a repeat gives the same bits.  The two mean squares are summed in fp64 (a square of an fp32 sample is
// exact there) and rounded to fp32 once, after the root: a frame of three samples then meets the same relative bound as one of 3528.
#include <cmath>

#include "../../include/lds.h"
#include "kernels.h"

namespace lds {

constexpr int kSvcThreads = 256;
constexpr int kSvcWaves = kSvcThreads / 64;
constexpr int kRmsSpanCap = 12288;      // floats of squared input a workgroup stages (48 KB)
constexpr int kRmsTileMax = 64;         // frames per workgroup, halved down to 1 until the span fits

// lanes' partial sums -> the wave's sum in lane 0 .. 63 alike, in a fixed butterfly order
static __device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// index of padded position p (pad samples in front) in x[0, L): -1 = a zero (mode 0), else the reflected sample (mode 1; the even
// reflection of period 2 (L - 1) that np.pad(mode='reflect') repeats when the pad exceeds the signal; L = 1 repeats the sample)
static __device__ __forceinline__ long long rms_src(long long p, int pad, long long L, int mode) {
    long long q = p - pad;
    if (q >= 0 && q < L) return q;
    if (mode == 0) return -1;
    if (L == 1) return 0;
    const long long P = 2 * (L - 1);
    q %= P;
    if (q < 0) q += P;
    return q < L ? q : P - q;
}

// grid ceil(n / tile): the workgroup reads the padded samples [t0 hop, (t0 + tile - 1) hop + fl) once into LDS (staged = 1) and wave w
// sums frames t0 + w, t0 + w + 4, ...: lane l takes elements l, l + 64, ... in increasing order, then the butterfly.  staged = 0 (one
// frame alone exceeds the staging buffer; tile = 1): the same sums straight from global memory.
__global__ void __launch_bounds__(kSvcThreads) frame_rms_kernel(const float* __restrict__ x, float* __restrict__ rms, long long L, int fl, int hop, int pad,
                                                                int mode, long long n, int tile, int staged) {
    extern __shared__ float svc_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long t0 = (long long)blockIdx.x * tile;
    const int cnt = (int)(n - t0 < tile ? n - t0 : tile);
    const long long p0 = t0 * hop;
    if (staged) {
        const int span = (cnt - 1) * hop + fl;      // <= kRmsSpanCap by the launcher's choice of tile
        for (int r = tid; r < span; r += kSvcThreads) {
            const long long q = rms_src(p0 + r, pad, L, mode);
            svc_smem[r] = q >= 0 ? x[q] : 0.f;
        }
        __syncthreads();
    }
    for (int f = w; f < cnt; f += kSvcWaves) {
        double acc = 0.0;
        if (staged) {
            const float* s = svc_smem + f * hop;
            for (int i = lane; i < fl; i += 64) acc = fma((double)s[i], (double)s[i], acc);
        } else {
            for (int i = lane; i < fl; i += 64) {
                const long long q = rms_src(p0 + (long long)f * hop + i, pad, L, mode);
                const double v = q >= 0 ? (double)x[q] : 0.0;
                acc = fma(v, v, acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) rms[t0 + f] = (float)sqrt(acc / (double)fl);
    }
}

// One wave per frame k: padded x^2 over [int(k hop), min(int((k + 1) hop), Lp)), the bounds in fp64 as Python computes them; the padding is
// np.pad(mode='reflect') by (pl, pr), a single reflection (pr < L is checked by the entry).
__global__ void __launch_bounds__(kSvcThreads) volume_kernel(const float* __restrict__ x, float* __restrict__ vol, long long L, double hop, int pl, int pr,
                                                             long long n) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * kSvcWaves + (threadIdx.x >> 6);
    if (k >= n) return;
    const long long Lp = L + pl + pr;
    long long a = (long long)((double)k * hop), b = (long long)((double)(k + 1) * hop);
    if (b > Lp) b = Lp;
    if (a > b) a = b;
    double acc = 0.0;
    for (long long p = a + lane; p < b; p += 64) {
        long long q = p - pl;
        if (q < 0) q = -q;
        if (q >= L) q = 2 * (L - 1) - q;
        q = q < 0 ? 0 : (q >= L ? L - 1 : q);      // (never taken with pl <= pr < L; keeps the read inside x whatever the arguments)
        const double v = (double)x[q];
        acc = fma(v, v, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) vol[k] = (float)sqrt(acc / (double)(b - a));
}

// out[j] = M[i] (1 - f) + M[min(i + 1, n - 1)] f, i = j / factor, f = (j % factor) / factor; M[k] = any volume > thr within 4 frames of k
static __device__ __forceinline__ float mask_dilated(const float* __restrict__ vol, long long k, long long n, float thr) {
    const long long lo = k - 4 < 0 ? 0 : k - 4, hi = k + 4 > n - 1 ? n - 1 : k + 4;
    float m = 0.f;
    for (long long i = lo; i <= hi; ++i) m = vol[i] > thr ? 1.f : m;
    return m;
}
__global__ void __launch_bounds__(kSvcThreads) volume_mask_kernel(const float* __restrict__ vol, float* __restrict__ out, long long n, int factor, float thr) {
    const long long j = (long long)blockIdx.x * kSvcThreads + threadIdx.x;
    if (j >= n * factor) return;
    const long long i = j / factor;
    const float f = (float)(j - i * factor) / (float)factor;
    const float m0 = mask_dilated(vol, i, n, thr), m1 = mask_dilated(vol, i + 1 < n ? i + 1 : n - 1, n, thr);
    out[j] = __fadd_rn(__fmul_rn(m0, 1.f - f), __fmul_rn(m1, f));
}

struct RfLens { int tin[64]; int tout[64]; };

// lds_resample_frames per clip: grid (Tout, B); rows of `in` at and beyond tin[b] are never read, rows of out beyond tout[b] are zeros
__global__ void resample_frames_ragged_kernel(const float* __restrict__ in, float* __restrict__ out, int Tin, int Tout, int C, const RfLens lens) {
    const int i = blockIdx.x, b = blockIdx.y;
    const int tin = lens.tin[b], tout = lens.tout[b];
    float* ob = out + ((long long)b * Tout + i) * C;
    if (i >= tout) {
        for (int cc = threadIdx.x; cc < C; cc += blockDim.x) ob[cc] = 0.f;
        return;
    }
    const float step = (float)tin / (float)tout;
    int src = (int)floorf((float)i * step);
    if (src > tin - 1) src = tin - 1;
    const float* ib = in + ((long long)b * Tin + src) * C;
    for (int cc = threadIdx.x; cc < C; cc += blockDim.x) ob[cc] = ib[cc];
}

// The reference's sequential join as a closed form (include/lds.h lds_overlap_assemble): with the preconditions at most two segments
// meet at a sample j.  s = the last segment with start <= j; the sample is v_s[j - start_s], cross-faded with v_{s-1} where j lies before
// segment s - 1's end, and zero in a gap.  tab = dev int64 [3][S]: offset, start, len.
__global__ void __launch_bounds__(kSvcThreads) overlap_assemble_kernel(const float* __restrict__ segs, const long long* __restrict__ tab, int S,
                                                                       const float* __restrict__ mask, float* __restrict__ out, long long N) {
    const long long j = (long long)blockIdx.x * kSvcThreads + threadIdx.x;
    if (j >= N) return;
    const long long* off = tab;
    const long long* start = tab + S;
    const long long* len = tab + 2 * (long long)S;
    int lo = 0, hi = S - 1;      // the last s with start[s] <= j, or -1 (a leading gap)
    int s = -1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= j) { s = mid; lo = mid + 1; } else hi = mid - 1;
    }
    float r = 0.f;
    if (s >= 0 && j < start[s] + len[s]) {
        const float m = mask ? mask[j] : 1.f;
        const float b = mask ? __fmul_rn(segs[off[s] + (j - start[s])], m) : segs[off[s] + (j - start[s])];
        r = b;
        if (s > 0) {
            const long long F = start[s - 1] + len[s - 1] - start[s];      // samples of segment s that fall on the result so far
            const long long i = j - start[s];
            if (i < F) {
                const float av = segs[off[s - 1] + (j - start[s - 1])];
                const float a = mask ? __fmul_rn(av, m) : av;
                const float k = F > 1 ? (float)((double)i / (double)(F - 1)) : 0.f;
                r = __fadd_rn(__fmul_rn(1.f - k, a), __fmul_rn(k, b));
            }
        }
    }
    out[j] = r;
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

using lds::set_error;

constexpr long long kSvcMaxL = 1LL << 30;
constexpr int kSvcMaxFrame = 1 << 24;

int launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LDS_OK : set_error(LDS_EHIP, "%s: %s", fn, hipGetErrorString(e));
}

// Python's float floor division a // b for b > 0 (CPython float_divmod), so that frame counts and pads equal the reference's
double py_floordiv(double a, double b) {
    double mod = std::fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && mod < 0) div -= 1.0;
    if (div == 0.0) return 0.0;
    double fd = std::floor(div);
    if (div - fd > 0.5) fd += 1.0;
    return fd;
}

}  // namespace

extern "C" int lds_frame_rms(const float* x, float* rms, int64_t L, int frame_length, int hop_length, int pad_mode, int64_t n, void* stream) {
    const char* fn = "lds_frame_rms";
    if (L < 1 || L > kSvcMaxL) return set_error(LDS_EINVAL, "%s: L %lld outside 1 .. %lld", fn, (long long)L, kSvcMaxL);
    if (frame_length < 1 || frame_length > kSvcMaxFrame || hop_length < 1 || hop_length > kSvcMaxFrame)
        return set_error(LDS_EINVAL, "%s: frame_length %d, hop_length %d outside 1 .. %d", fn, frame_length, hop_length, kSvcMaxFrame);
    if (pad_mode != 0 && pad_mode != 1) return set_error(LDS_EINVAL, "%s: pad_mode %d (0 zeros, 1 reflect)", fn, pad_mode);
    const int pad = frame_length / 2;
    const long long need = 1 + (L + 2LL * pad - frame_length) / hop_length;
    if (n != need) return set_error(LDS_EINVAL, "%s: n %lld, must be %lld = 1 + (L + 2 (fl / 2) - fl) / hop", fn, (long long)n, need);
    if (!x || !rms) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    int tile = lds::kRmsTileMax;
    auto span_of = [&](int t) { return (long long)(t - 1) * hop_length + frame_length; };
    while (tile > 1 && span_of(tile) > lds::kRmsSpanCap) tile >>= 1;
    const int staged = span_of(tile) <= lds::kRmsSpanCap;
    const size_t smem = staged ? 4 * (size_t)span_of(tile) : 0;
    hipStream_t s = (hipStream_t)stream;
    lds::ProfScope ps(s, "frame_rms", 2.0 * (double)n * frame_length, 4.0 * ((double)L + (double)n));
    hipLaunchKernelGGL(lds::frame_rms_kernel, dim3((unsigned)((n + tile - 1) / tile)), dim3(lds::kSvcThreads), smem, s, x, rms, (long long)L, frame_length,
                       hop_length, pad, pad_mode, (long long)n, tile, staged);
    return launched(fn);
}

namespace {
// n = int(L // hop) + 1 after the checks that lds_volume_extract shares with nothing else
int volume_frames(const char* fn, int64_t L, double hop, int64_t* n) {
    if (L < 1 || L > kSvcMaxL) return set_error(LDS_EINVAL, "%s: L %lld outside 1 .. %lld", fn, (long long)L, kSvcMaxL);
    if (!(hop >= 1.0) || hop > (double)kSvcMaxFrame) return set_error(LDS_EINVAL, "%s: hop %g outside 1 .. %d", fn, hop, kSvcMaxFrame);
    const long long pr = (long long)py_floordiv(hop + 1.0, 2.0);
    if (L <= pr) return set_error(LDS_EINVAL, "%s: L %lld must exceed int((hop + 1) // 2) = %lld (the reflect padding)", fn, (long long)L, pr);
    *n = (long long)py_floordiv((double)L, hop) + 1;
    return LDS_OK;
}
}  // namespace

extern "C" int lds_volume_extract(const float* x, float* volume, int64_t L, const double* hop_size, int64_t n, void* stream) {
    const char* fn = "lds_volume_extract";
    if (!hop_size) return set_error(LDS_EINVAL, "%s: null hop_size", fn);
    const double hop = *hop_size;
    int64_t need = 0;
    if (volume_frames(fn, L, hop, &need) != LDS_OK) return LDS_EINVAL;
    if (n != need) return set_error(LDS_EINVAL, "%s: n %lld, must be %lld = int(L // hop) + 1", fn, (long long)n, (long long)need);
    if (!x || !volume) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const int pl = (int)py_floordiv(hop, 2.0), pr = (int)py_floordiv(hop + 1.0, 2.0);
    hipStream_t s = (hipStream_t)stream;
    lds::ProfScope ps(s, "volume_extract", 2.0 * (double)L, 4.0 * ((double)L + (double)n));
    hipLaunchKernelGGL(lds::volume_kernel, dim3((unsigned)((n + lds::kSvcWaves - 1) / lds::kSvcWaves)), dim3(lds::kSvcThreads), 0, s, x, volume, (long long)L,
                       hop, pl, pr, (long long)n);
    return launched(fn);
}

extern "C" int lds_volume_mask(const float* volume, float* mask, int64_t n, int factor, float threshold, void* stream) {
    const char* fn = "lds_volume_mask";
    if (n < 1 || n > kSvcMaxL) return set_error(LDS_EINVAL, "%s: n %lld outside 1 .. %lld", fn, (long long)n, kSvcMaxL);
    if (factor < 1 || factor > 65536) return set_error(LDS_EINVAL, "%s: factor %d outside 1 .. 65536", fn, factor);
    if ((long long)n * factor > (1LL << 40)) return set_error(LDS_EINVAL, "%s: %lld x %d output samples above 2^40", fn, (long long)n, factor);
    if (!volume || !mask) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const long long total = (long long)n * factor;
    if ((total + lds::kSvcThreads - 1) / lds::kSvcThreads > 2147483647LL) return set_error(LDS_EINVAL, "%s: %lld output samples above one grid", fn, total);
    hipStream_t s = (hipStream_t)stream;
    lds::ProfScope ps(s, "volume_mask", 4.0 * (double)total, 4.0 * ((double)n + (double)total));
    hipLaunchKernelGGL(lds::volume_mask_kernel, dim3((unsigned)((total + lds::kSvcThreads - 1) / lds::kSvcThreads)), dim3(lds::kSvcThreads), 0, s, volume, mask,
                       (long long)n, factor, threshold);
    return launched(fn);
}

extern "C" int lds_resample_frames_ragged(const float* in, const int32_t* tin, const int32_t* tout, float* out, int B, int Tin, int Tout, int C,
                                          void* stream) {
    const char* fn = "lds_resample_frames_ragged";
    if (B < 1 || B > 64) return set_error(LDS_EINVAL, "%s: B %d outside 1 .. 64", fn, B);
    if (Tin < 1 || Tout < 1 || C < 1) return set_error(LDS_EINVAL, "%s: Tin %d, Tout %d, C %d must be positive", fn, Tin, Tout, C);
    if (!tin || !tout) return set_error(LDS_EINVAL, "%s: null lengths", fn);
    lds::RfLens lens;
    for (int b = 0; b < 64; ++b) lens.tin[b] = 1, lens.tout[b] = 0;
    for (int b = 0; b < B; ++b) {
        if (tin[b] < 1 || tin[b] > Tin) return set_error(LDS_EINVAL, "%s: tin[%d] = %d outside 1 .. %d", fn, b, tin[b], Tin);
        if (tout[b] < 0 || tout[b] > Tout) return set_error(LDS_EINVAL, "%s: tout[%d] = %d outside 0 .. %d", fn, b, tout[b], Tout);
        lens.tin[b] = tin[b];
        lens.tout[b] = tout[b];
    }
    if (!in || !out) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipStream_t s = (hipStream_t)stream;
    lds::ProfScope ps(s, "resample_frames_ragged", 0.0, 8.0 * (double)B * Tout * C);
    hipLaunchKernelGGL(lds::resample_frames_ragged_kernel, dim3(Tout, B), dim3(256), 0, s, in, out, Tin, Tout, C, lens);
    return launched(fn);
}

extern "C" int lds_overlap_assemble(const float* segs, int64_t segs_len, const int64_t* host_tab, const int64_t* dev_tab, int S, const float* mask,
                                    int64_t mask_len, float* out, int64_t N, void* stream) {
    const char* fn = "lds_overlap_assemble";
    if (S < 1 || S > (1 << 20)) return set_error(LDS_EINVAL, "%s: S %d outside 1 .. 2^20", fn, S);
    if (!host_tab) return set_error(LDS_EINVAL, "%s: null host table", fn);
    const int64_t* off = host_tab;
    const int64_t* start = host_tab + S;
    const int64_t* len = host_tab + 2 * (int64_t)S;
    for (int s = 0; s < S; ++s) {
        if (start[s] < 0 || len[s] < 0 || start[s] > kSvcMaxL * 4 || len[s] > kSvcMaxL)
            return set_error(LDS_EINVAL, "%s: segment %d: start %lld, len %lld out of range", fn, s, (long long)start[s], (long long)len[s]);
        if (off[s] < 0 || off[s] + len[s] > segs_len)
            return set_error(LDS_EINVAL, "%s: segment %d: offset %lld + len %lld outside the packed buffer of %lld", fn, s, (long long)off[s], (long long)len[s],
                             (long long)segs_len);
        if (s > 0 && start[s] < start[s - 1])
            return set_error(LDS_EINVAL, "%s: segment %d: start %lld below segment %d's %lld (starts must not decrease)", fn, s, (long long)start[s], s - 1,
                             (long long)start[s - 1]);
        if (s > 0 && start[s - 1] + len[s - 1] - start[s] > len[s])
            return set_error(LDS_EINVAL, "%s: segment %d: the overlap of %lld samples with segment %d exceeds its own %lld", fn, s,
                             (long long)(start[s - 1] + len[s - 1] - start[s]), s - 1, (long long)len[s]);
        if (s > 1 && start[s] < start[s - 2] + len[s - 2])
            return set_error(LDS_EINVAL, "%s: segment %d: start %lld inside segment %d (ends at %lld): three segments would meet", fn, s, (long long)start[s],
                             s - 2, (long long)(start[s - 2] + len[s - 2]));
    }
    const int64_t need = start[S - 1] + len[S - 1];
    if (N != need) return set_error(LDS_EINVAL, "%s: N %lld, must be %lld = start + len of the last segment", fn, (long long)N, (long long)need);
    if (mask && mask_len < N) return set_error(LDS_EINVAL, "%s: the mask holds %lld samples, fewer than the %lld of the result", fn, (long long)mask_len, (long long)N);
    if (N == 0) return LDS_OK;
    if ((N + lds::kSvcThreads - 1) / lds::kSvcThreads > 2147483647LL) return set_error(LDS_EINVAL, "%s: N %lld above one grid", fn, (long long)N);
    if (!segs || !dev_tab || !out) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipStream_t s = (hipStream_t)stream;
    lds::ProfScope ps(s, "overlap_assemble", 4.0 * (double)N, 4.0 * 3.0 * (double)N);
    hipLaunchKernelGGL(lds::overlap_assemble_kernel, dim3((unsigned)((N + lds::kSvcThreads - 1) / lds::kSvcThreads)), dim3(lds::kSvcThreads), 0, s, segs,
                       (const long long*)dev_tab, S, mask, out, (long long)N);
    return launched(fn);
}
