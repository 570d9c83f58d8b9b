// Polyphase sinc resampler in front of the audio encoders (reference torchaudio.transforms.Resample(orig, new) with its defaults, called at
// tools/tools.py:78-84, diffusion/vocoder.py:24-27 and batch_proccessor/semantic_extract.py:49-68), exact fp32, gfx950.
//   out[m] = sum_n x[n] g(n/O - m/N), 0 <= m < ceil(N len / O), x zero outside [0, len).  With m = q N + i the filter depends on the phase i
//   only: out[m] = sum_{k < T} x[q O + first[i] + k] bankT[k][i].  The bank (float64 on the host, rounded once: lds/arch.py resample_bank)
//   holds the T = `taps` columns from the first one inside the filter's support; it is stored tap-major [T][N], so that the consecutive
//   outputs of a wave read consecutive phases: conflict-free from LDS, coalesced from global memory.
//   One fmaf chain per output in tap order, no atomics: an output's bits depend on its clip's samples alone -- not on the batch, the
//   position in it, the tile or which of the two kernels ran.  Every index is an integer: m O and q O in 64 bits, never a float centre.
#include "../../include/lds.h"
#include "kernels.h"

namespace lds {

constexpr int kRsThreads = 256;
constexpr int kRsSpanCap = 8192;       // floats of input a workgroup stages (32 KB)
constexpr int kRsBankCap = 8192;       // a bank of at most this many floats is copied to LDS (32 KB); a larger one is read from global memory
constexpr int kRsTileMax = 2048;       // outputs per workgroup, halved down to 64 until the input span fits

struct RsLens { int n; int v[64]; };      // ragged form: n = B clips, v[b] valid samples; n = 0: every clip has L

// The R outputs t = tid + r * 256 of a thread, their R chains advanced together tap by tap: 2 R independent LDS reads in flight per step
// instead of a chain that waits for each.  Every chain is the same fmaf sequence whatever R.  An output beyond `live` (the clip's own
// end) runs the chain of the tile's first output and stores zero; one beyond `cnt` (the row's end) stores nothing.
template <int R>
static __device__ __forceinline__ void rs_chains(const float* xs, const float* bk, const int* __restrict__ first, float* __restrict__ yt, int i0, int fi0, int O, int N,
                                                 int T, int span, int cnt, int live) {
    const float* xp[R];
    const float* bp[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = threadIdx.x + r * kRsThreads;
        const unsigned it = (unsigned)i0 + (unsigned)(t < live ? t : 0);
        const int dq = (int)(it / (unsigned)N), i = (int)(it - (unsigned)dq * (unsigned)N);
        int rel = dq * O + (first[i] - fi0);
        rel = rel < 0 ? 0 : (rel > span - T ? span - T : rel);
        xp[r] = xs + rel;
        bp[r] = bk + i;
        acc[r] = 0.f;
    }
    for (int k = 0; k < T; ++k) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(xp[r][k], bp[r][k * N], acc[r]);      // (T N <= 2^24)
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = threadIdx.x + r * kRsThreads;
        if (t < cnt) yt[t] = t < live ? acc[r] : 0.f;
    }
}

static __device__ __forceinline__ void rs_outputs(const float* xs, const float* bk, const int* __restrict__ first, float* __restrict__ yt, int i0, int O, int N, int T,
                                                  int span, int cnt, int live) {
    const int fi0 = first[i0];
    const int nr = (cnt + kRsThreads - 1) / kRsThreads;
    if (nr <= 1) rs_chains<1>(xs, bk, first, yt, i0, fi0, O, N, T, span, cnt, live);
    else if (nr <= 2) rs_chains<2>(xs, bk, first, yt, i0, fi0, O, N, T, span, cnt, live);
    else if (nr <= 4) rs_chains<4>(xs, bk, first, yt, i0, fi0, O, N, T, span, cnt, live);
    else rs_chains<8>(xs, bk, first, yt, i0, fi0, O, N, T, span, cnt, live);
}

// grid (ceil(M / tile), B).  The workgroup stages x[b][s0 .. s0 + span) (zeros outside [0, len)) and, when it fits, the bank; thread t takes
// outputs m0 + t, m0 + t + 256, ... (rs_chains).  LDS: xs[span_cap] then bank[T * N] (bank_lds) -- every LDS index is clamped into the allocation, so a
// malformed offset table cannot reach outside it (the global reads are guarded by [0, len) anyway).
__global__ void __launch_bounds__(kRsThreads) resample_tile_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ bankT,
                                                                   const int* __restrict__ first, int O, int N, int T, long long L, long long M, int tile,
                                                                   int span_cap, int bank_lds, int vec, const RsLens lens) {
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    float* xs = rs_smem;
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long len = lens.n > 0 ? (long long)lens.v[b] : L;
    const long long Mb = (len * N + O - 1) / O;
    const long long m0 = (long long)blockIdx.x * tile;
    float* yr = y + (long long)b * M;
    const int cnt = (int)(M - m0 < tile ? M - m0 : tile);      // outputs of this tile inside the row
    if (m0 >= Mb) {                                            // beyond the clip's own output: zeros
        for (int t = tid; t < cnt; t += kRsThreads) yr[m0 + t] = 0.f;
        return;
    }
    const int live = (int)(Mb - m0 < cnt ? Mb - m0 : cnt);
    const long long q0 = m0 / N, ml = m0 + live - 1;
    const int i0 = (int)(m0 - q0 * N);
    const long long s0 = q0 * O + first[i0];                  // first sample of the first output; first samples never decrease with m
    long long s1 = (ml / N) * O + first[(int)(ml % N)] + T;   // one past the last sample of the last output
    int span = (int)(s1 - s0 < span_cap ? s1 - s0 : span_cap);
    if (span < T) span = T;
    const float* xr = x + (long long)b * L;
    if (vec) {      // L % 4 == 0 and x 16-byte aligned: whole 16-byte pieces from the aligned sample at or before s0
        const long long a0 = s0 & ~3LL;
        const int lead = (int)(s0 - a0);
        for (int p = tid; p * 4 < span + lead; p += kRsThreads) {
            const long long n = a0 + 4LL * p;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n >= 0 && n < len) v = *reinterpret_cast<const float4*>(xr + n);      // n + 3 < L: both are multiples of 4
            const float e[4] = {v.x, n + 1 < len ? v.y : 0.f, n + 2 < len ? v.z : 0.f, n + 3 < len ? v.w : 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int r = 4 * p + c - lead;
                if (r >= 0 && r < span) xs[r] = e[c];
            }
        }
    } else {
        for (int r = tid; r < span; r += kRsThreads) {
            const long long n = s0 + r;
            xs[r] = n >= 0 && n < len ? xr[n] : 0.f;
        }
    }
    float* bl = rs_smem + span_cap;
    if (bank_lds)
        for (int e = tid; e < T * N; e += kRsThreads) bl[e] = bankT[e];
    __syncthreads();
    // (two calls, so that each copy of the loop knows its bank's address space: LDS reads in one, global loads in the other)
    if (bank_lds) rs_outputs(xs, bl, first, yr + m0, i0, O, N, T, span, cnt, live);
    else rs_outputs(xs, bankT, first, yr + m0, i0, O, N, T, span, cnt, live);
}

// One thread per output, everything from global memory: the pairs whose input span per 64 outputs does not fit the staging buffer (a
// narrow filter in front of a deep decimation).  The same chain in the same order as the tiled kernel.
__global__ void __launch_bounds__(kRsThreads) resample_direct_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ bankT,
                                                                     const int* __restrict__ first, int O, int N, int T, long long L, long long M,
                                                                     const RsLens lens) {
    const int b = blockIdx.y;
    const long long m = (long long)blockIdx.x * kRsThreads + threadIdx.x;
    if (m >= M) return;
    const long long len = lens.n > 0 ? (long long)lens.v[b] : L;
    const long long Mb = (len * N + O - 1) / O;
    float acc = 0.f;
    if (m < Mb) {
        const long long q = m / N;
        const int i = (int)(m - q * N);
        const long long s = q * O + first[i];
        const float* xr = x + (long long)b * L;
        for (int k = 0; k < T; ++k) {
            const long long n = s + k;
            acc = fmaf(n >= 0 && n < len ? xr[n] : 0.f, bankT[(long long)k * N + i], acc);
        }
    }
    y[(long long)b * M + m] = acc;
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

using lds::set_error;

constexpr int kRsMaxRate = 384000;
constexpr int kRsMaxTaps = 1024;
constexpr long long kRsMaxBank = 1LL << 24;
constexpr long long kRsMaxL = 1LL << 30;
constexpr long long kRsMaxM = 2147483647LL;

int rs_run(const char* fn, const float* x, const int32_t* lengths, bool ragged, float* y, int64_t* new_lengths, const float* bankT, const int32_t* first,
           int O, int N, int taps, int B, long long L, long long M, hipStream_t s) {
    if (O < 1 || O > kRsMaxRate || N < 1 || N > kRsMaxRate) return set_error(LDS_EINVAL, "%s: rates O %d, N %d outside 1 .. %d", fn, O, N, kRsMaxRate);
    if (taps < 1 || taps > kRsMaxTaps) return set_error(LDS_EINVAL, "%s: taps %d outside 1 .. %d", fn, taps, kRsMaxTaps);
    if ((long long)N * taps > kRsMaxBank) return set_error(LDS_EINVAL, "%s: bank of %lld entries (N %d x taps %d) above %lld", fn, (long long)N * taps, N, taps, kRsMaxBank);
    if (L < 1 || L > kRsMaxL) return set_error(LDS_EINVAL, "%s: L %lld outside 1 .. %lld", fn, L, kRsMaxL);
    if (ragged ? (B < 1 || B > 64) : (B < 1 || B > 65535)) return set_error(LDS_EINVAL, "%s: B %d outside 1 .. %d", fn, B, ragged ? 64 : 65535);
    if (ragged && !lengths) return set_error(LDS_EINVAL, "%s: null lengths", fn);
    if (!x || !y || !bankT || !first) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    lds::RsLens lens;
    lens.n = ragged ? B : 0;
    for (int i = 0; i < 64; ++i) lens.v[i] = 0;
    long long need = (L * N + O - 1) / O;      // (L N < 2^49)
    if (ragged) {
        need = 0;
        for (int b = 0; b < B; ++b) {
            if (lengths[b] < 0 || lengths[b] > L) return set_error(LDS_EINVAL, "%s: lengths[%d] = %d outside 0 .. %lld", fn, b, lengths[b], L);
            lens.v[b] = lengths[b];
            const long long mb = ((long long)lengths[b] * N + O - 1) / O;
            need = mb > need ? mb : need;
        }
    }
    if (need > kRsMaxM) return set_error(LDS_EINVAL, "%s: %lld output samples per clip above %lld", fn, need, kRsMaxM);
    if (ragged ? (M < need || M < 1 || M > kRsMaxM) : M != need)
        return set_error(LDS_EINVAL, "%s: M %lld, the output row, must be %s %lld = ceil(N len / O)", fn, M, ragged ? "at least" : "exactly", need);
    if (new_lengths)
        for (int b = 0; b < B; ++b) new_lengths[b] = ((long long)lens.v[b] * N + O - 1) / O;
    // outputs per workgroup: the most whose input span, at most ceil(tile O / N) + taps + 1 samples, fits the staging buffer
    int tile = lds::kRsTileMax;
    auto span_of = [&](int t) { return ((long long)t * O + N - 1) / N + taps + 1; };
    while (tile > 64 && span_of(tile) > lds::kRsSpanCap) tile >>= 1;
    lds::ProfScope ps(s, "resample", 2.0 * (double)B * M * taps, 4.0 * ((double)B * L + (double)B * M));
    if (span_of(tile) > lds::kRsSpanCap) {
        hipLaunchKernelGGL(lds::resample_direct_kernel, dim3((unsigned)((M + lds::kRsThreads - 1) / lds::kRsThreads), B), dim3(lds::kRsThreads), 0, s, x, y, bankT,
                           (const int*)first, O, N, taps, L, M, lens);
    } else {
        const int span_cap = (int)((span_of(tile) + 3) & ~3LL);
        const int bank_lds = (long long)N * taps <= lds::kRsBankCap;
        const int vec = L % 4 == 0 && ((uintptr_t)x & 15) == 0;
        const size_t smem = 4 * ((size_t)span_cap + (bank_lds ? (size_t)N * taps : 0));      // <= 64 KB
        hipLaunchKernelGGL(lds::resample_tile_kernel, dim3((unsigned)((M + tile - 1) / tile), B), dim3(lds::kRsThreads), smem, s, x, y, bankT, (const int*)first, O,
                           N, taps, L, M, tile, span_cap, bank_lds, vec, lens);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LDS_OK : set_error(LDS_EHIP, "%s: %s", fn, hipGetErrorString(e));
}

}  // namespace

extern "C" int lds_resample(const float* x, float* y, const float* bankT, const int32_t* first, int O, int N, int taps, int B, int64_t L, int64_t M,
                            void* stream) {
    return rs_run("lds_resample", x, nullptr, false, y, nullptr, bankT, first, O, N, taps, B, L, M, (hipStream_t)stream);
}

extern "C" int lds_resample_ragged(const float* x, const int32_t* lengths, float* y, int64_t* new_lengths, const float* bankT, const int32_t* first, int O,
                                   int N, int taps, int B, int64_t L, int64_t M, void* stream) {
    return rs_run("lds_resample_ragged", x, lengths, true, y, new_lengths, bankT, first, O, N, taps, B, L, M, (hipStream_t)stream);
}
