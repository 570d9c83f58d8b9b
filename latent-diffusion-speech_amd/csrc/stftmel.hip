// The vocoder's log-mel analysis (reference modules/nvSTFT.py:69-118, STFT.get_mel with center = False) as one launch:
//   stft_mel_kernel   audio -> pad (reflect / constant) -> framed DFT -> magnitude -> keyshift cut and scale -> mel -> log, frame-major
//
// The DFT is a product of the frames with a windowed (cos, -sin) basis [n_fft_new][bins] that the host builds in float64, so one kernel
// covers every transform size a keyshift produces (1024 .. 4096, 1367 included).  The product runs on the f64 matrix pipe
// (v_mfma_f64_16x16x4_f64): A = 16 frames x 4 samples widened from fp32, B = 4 samples x 16 bins of the double basis.  A product of two
// fp32-representable values accumulated in double is exact to 1e-16, so what is left of the error against a float64 evaluation of the
// reference's lines is the fp32 tail (magnitude, mel product; the log is taken in double and rounded once) -- the choice of logmel.hip, on the matrix pipe because 2 * 2048 * 2050
// flop per frame is too much for one double VALU chain per bin.
// Padding and framing are index arithmetic on the clip's own length: a workgroup stages the contiguous span of its 16 frames in LDS once
// and reads the overlapping windows from there; nothing at or beyond a clip's length is loaded.  Per pass of 128 bins the magnitudes go
// through LDS straight into the mel accumulators of the frame tile, so the [frames][bins] spectrum never reaches memory.
// Every clip's frames are tiled from its own frame 0 with one fixed tile, so a clip's rows do not depend on the batch it is in.
#include "kernels.h"
#include "../../include/lds_test.h"

#include <math.h>

#include <atomic>

namespace lds {

constexpr int SM_FB = 16;                  // frames per workgroup: the M of the MFMA
constexpr int SM_BB = 128;                 // bins per pass: 4 waves x 2 tiles of 16
constexpr int SM_MAGLD = SM_FB + 1;
constexpr int SM_MAX_LDS = 160 * 1024;

typedef double sm_d4 __attribute__((ext_vector_type(4)));

struct SmLens { int n; int v[64]; };       // n = 0: every clip has L samples
struct SmGeom {
    int nfft, hop;                         // transform size and hop after keyshift / speed
    int pad_left, pad_right_min, win;      // (win - hop) / 2, (win - hop + 1) / 2, the window length after keyshift
    int bins;                              // bins computed: min(nfft / 2 + 1, n_fft / 2 + 1); the mel basis' further rows meet zeros
    int n_mels, span;                      // span = (SM_FB - 1) hop + nfft samples staged per workgroup
    int scaled;                            // keyshift != 0: magnitude * mul / div
    float mul, div, clip, log_clip;
};

// the clip's own right pad, padding mode and frame count (nvSTFT.py:98-105 and torch.stft's frame count)
static __device__ __forceinline__ void sm_clip_geometry(const SmGeom& g, long long len, bool& reflect, long long& F) {
    long long pr = (long long)g.win - len - g.pad_left;
    if (pr < g.pad_right_min) pr = g.pad_right_min;
    reflect = pr < len;
    const long long total = len + g.pad_left + pr - g.nfft;
    F = total < 0 ? 0 : 1 + total / g.hop;
}

// grid (ceil(Fmax / SM_FB), B), 256 threads, dynamic LDS: xs[span] then mag[SM_BB][SM_MAGLD].  basis [nfft][bins] (cos, -sin) pairs with
// the window folded in; melT [n_fft / 2 + 1][n_mels] (rows < bins are read); out [B][Fmax][n_mels], zero rows at and beyond the clip's frames.
// DUMP: dft [B][Fmax][bins] receives the raw (re, im) sums of the clip's frames (tests: the fragment map).
template <bool DUMP>
__global__ void __launch_bounds__(256) stft_mel_kernel(const float* __restrict__ audio, const SmLens lens, long long L, int Fmax,
                                                       const double2* __restrict__ basis, const float* __restrict__ melT, const SmGeom g,
                                                       float* __restrict__ out, double2* __restrict__ dft) {
#pragma clang fp contract(off)      // (the fp32 tail's roundings are the reference's: a product and a sum each on its own; fmaf is explicit)
    extern __shared__ __attribute__((aligned(16))) float sm_smem[];
    float* xs = sm_smem;
    float* mag = sm_smem + g.span;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, f0 = blockIdx.x * SM_FB;
    const long long len = lens.n > 0 ? (long long)lens.v[b] : L;
    bool reflect;
    long long Fb;
    sm_clip_geometry(g, len, reflect, Fb);
    const int n_mels = g.n_mels;
    const int rows = Fmax - f0 < SM_FB ? Fmax - f0 : SM_FB;      // rows of this tile inside the output
    const int om = tid % n_mels, og = tid / n_mels;                // this thread's mel channel and half (8 frames) of the tile
    if (f0 >= Fb) {
        if (og < 2)
            for (int e = 0; e < 8; ++e)
                if (og * 8 + e < rows) out[((long long)b * Fmax + f0 + og * 8 + e) * n_mels + om] = 0.f;
        return;
    }
    const int nf = Fb - f0 < rows ? (int)(Fb - f0) : rows;
    const int used = g.hop * (nf - 1) + g.nfft;
    const float* xr = audio + (long long)b * L;
    for (int i = tid; i < g.span; i += 256) {
        long long s = (long long)f0 * g.hop + i - g.pad_left;
        if (reflect) {                           // edge sample not repeated; both pads are shorter than the clip
            if (s < 0) s = -s;
            if (s >= len) s = 2 * (len - 1) - s;
        }
        xs[i] = (i < used && s >= 0 && s < len) ? xr[s] : 0.f;
    }
    __syncthreads();

    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const int ar = lane & 15, ak = lane >> 4;      // A: frame ar, sample ak of the step; B: sample ak, bin ar of the tile
    const float* xa = xs + ar * g.hop;
    for (int bb = 0; bb < g.bins; bb += SM_BB) {
        const int t0 = bb + wave * 32;
        if (t0 < g.bins) {                       // (wave-uniform)
            sm_d4 re[2], im[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) { re[j] = (sm_d4){0.0, 0.0, 0.0, 0.0}; im[j] = re[j]; }
            // a column of B reaches its own column of D only: the columns beyond `bins` read the last bin's and are dropped below
            const int c0 = t0 + ar < g.bins ? t0 + ar : g.bins - 1, c1 = t0 + 16 + ar < g.bins ? t0 + 16 + ar : g.bins - 1;
            auto step = [&](int kk, double a) {
                const double2* br = basis + (long long)kk * g.bins;
                const double2 b0 = br[c0], b1 = br[c1];
                re[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0.x, re[0], 0, 0, 0);
                im[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0.y, im[0], 0, 0, 0);
                re[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1.x, re[1], 0, 0, 0);
                im[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1.y, im[1], 0, 0, 0);
            };
            const int n_main = g.nfft & ~15;
            for (int n0 = 0; n0 < n_main; n0 += 16) {
#pragma unroll
                for (int u = 0; u < 4; ++u) step(n0 + 4 * u + ak, (double)xa[n0 + 4 * u + ak]);
            }
            for (int n0 = n_main; n0 < g.nfft; n0 += 4) {      // a sample beyond the transform: a zero times the last row
                const int kk = n0 + ak;
                step(kk < g.nfft ? kk : g.nfft - 1, kk < g.nfft ? (double)xa[kk] : 0.0);
            }
            // f64 C/D map: column (bin) = lane & 15, row (frame) = (lane >> 4) + 4 r
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int kl = wave * 32 + 16 * j + ar, k = bb + kl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = ak + 4 * r;
                    float m = 0.f;
                    if (k < g.bins) {
                        const float fr = (float)re[j][r], fi = (float)im[j][r];
                        m = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(fr, fr), __fmul_rn(fi, fi)), 1e-9f));
                        if (g.scaled) m = __fdiv_rn(__fmul_rn(m, g.mul), g.div);
                        if (DUMP && f < nf) dft[((long long)b * Fmax + f0 + f) * g.bins + k] = make_double2(re[j][r], im[j][r]);
                    }
                    mag[kl * SM_MAGLD + f] = m;
                }
            }
        }
        __syncthreads();
        if (og < 2) {
            const int kn = g.bins - bb < SM_BB ? g.bins - bb : SM_BB;
            const float* wp = melT + (long long)bb * n_mels + om;
            const float* mp = mag + og * 8;
            for (int kl = 0; kl < kn; ++kl) {
                const float w = wp[(long long)kl * n_mels];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, mp[kl * SM_MAGLD + e], acc[e]);
            }
        }
        __syncthreads();
    }
    if (og < 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = og * 8 + e;
            if (f < rows) {
                const float v = acc[e];
                // (the log in double, rounded once: 2048 values per workgroup)
                out[((long long)b * Fmax + f0 + f) * n_mels + om] = f < nf ? (v <= g.clip ? g.log_clip : (float)log((double)v)) : 0.f;
            }
        }
    }
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h, include/lds_test.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

using lds::set_error;

constexpr long long kSmMaxL = 1LL << 30;
constexpr int kSmMaxFft = 1 << 15;

std::atomic<unsigned long long> g_sm_lds_done{0}, g_sm_dump_lds_done{0};

long long sm_frames(const lds::SmGeom& g, long long len) {
    long long pr = (long long)g.win - len - g.pad_left;
    if (pr < g.pad_right_min) pr = g.pad_right_min;
    const long long total = len + g.pad_left + pr - g.nfft;
    return total < 0 ? 0 : 1 + total / g.hop;
}

int sm_geometry(const char* fn, int n_fft_new, int win_new, int hop_new, int n_fft, int win, int n_mels, float clip_val, lds::SmGeom& g) {
    if (n_fft_new < 4 || n_fft_new > kSmMaxFft || n_fft < 4 || n_fft > kSmMaxFft)
        return set_error(LDS_EINVAL, "%s: transform sizes %d / %d outside 4 .. %d", fn, n_fft_new, n_fft, kSmMaxFft);
    if (win_new < 1 || win_new > n_fft_new || win < 1) return set_error(LDS_EINVAL, "%s: window %d (of %d) must be 1 .. n_fft_new %d", fn, win_new, win, n_fft_new);
    if (hop_new < 1 || hop_new > win_new) return set_error(LDS_EINVAL, "%s: hop %d outside 1 .. the window %d", fn, hop_new, win_new);
    if (n_mels < 1 || n_mels > 128) return set_error(LDS_EINVAL, "%s: n_mels %d outside 1 .. 128", fn, n_mels);
    if (!(clip_val > 0.f)) return set_error(LDS_EINVAL, "%s: clip_val must be positive", fn);
    g.nfft = n_fft_new; g.hop = hop_new; g.win = win_new;
    g.pad_left = (win_new - hop_new) / 2;
    g.pad_right_min = (win_new - hop_new + 1) / 2;
    const int b_new = n_fft_new / 2 + 1, b_out = n_fft / 2 + 1;
    g.bins = b_new < b_out ? b_new : b_out;
    g.n_mels = n_mels;
    g.span = (lds::SM_FB - 1) * hop_new + n_fft_new;
    g.scaled = win_new != win;
    g.mul = (float)win; g.div = (float)win_new;
    g.clip = clip_val;
    g.log_clip = (float)log((double)clip_val);
    const size_t smem = 4 * ((size_t)g.span + lds::SM_BB * lds::SM_MAGLD);
    if (smem > (size_t)lds::SM_MAX_LDS)
        return set_error(LDS_EINVAL, "%s: %d frames of hop %d and size %d need %zu bytes of LDS (at most %d)", fn, lds::SM_FB, hop_new, n_fft_new, smem, lds::SM_MAX_LDS);
    return LDS_OK;
}

int sm_run(const char* fn, const float* audio, const int32_t* lengths, const double* basis, const float* melT, const lds::SmGeom& g, int Fmax, float* out,
           double* dft, int B, long long L, hipStream_t s) {
    if (!audio || !basis || !melT || !out) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    if (L < 1 || L > kSmMaxL) return set_error(LDS_EINVAL, "%s: L %lld outside 1 .. %lld", fn, L, kSmMaxL);
    if (lengths ? (B < 1 || B > 64) : (B < 1 || B > 65535)) return set_error(LDS_EINVAL, "%s: B %d outside 1 .. %d", fn, B, lengths ? 64 : 65535);
    lds::SmLens lens;
    lens.n = lengths ? B : 0;
    for (int i = 0; i < 64; ++i) lens.v[i] = 0;
    long long need = sm_frames(g, L);
    if (lengths) {
        need = 0;
        for (int b = 0; b < B; ++b) {
            if (lengths[b] < 1 || lengths[b] > L) return set_error(LDS_EINVAL, "%s: lengths[%d] = %d outside 1 .. %lld", fn, b, lengths[b], L);
            lens.v[b] = lengths[b];
            const long long fb = sm_frames(g, lengths[b]);
            need = fb > need ? fb : need;
        }
    }
    if (Fmax < 1 || Fmax < need || (long long)Fmax > 2147483647LL / 256)
        return set_error(LDS_EINVAL, "%s: F %d, the output's rows, must be at least %lld frames", fn, Fmax, need);
    const size_t smem = 4 * ((size_t)g.span + lds::SM_BB * lds::SM_MAGLD);
    const dim3 grid((unsigned)((Fmax + lds::SM_FB - 1) / lds::SM_FB), B);
    const double fl = 2.0 * B * (double)Fmax * g.bins * (2.0 * g.nfft + g.n_mels);
    lds::ProfScope ps(s, "stft_mel", fl, 4.0 * B * ((double)L + (double)Fmax * g.n_mels) + 16.0 * g.nfft * (double)g.bins);
    hipError_t e;
    if (dft) {
        e = lds::ensure_max_dynamic_lds(reinterpret_cast<const void*>(&lds::stft_mel_kernel<true>), g_sm_dump_lds_done);
        if (e == hipSuccess)
            hipLaunchKernelGGL(lds::stft_mel_kernel<true>, grid, dim3(256), smem, s, audio, lens, L, Fmax, reinterpret_cast<const double2*>(basis), melT, g, out,
                               reinterpret_cast<double2*>(dft));
    } else {
        e = lds::ensure_max_dynamic_lds(reinterpret_cast<const void*>(&lds::stft_mel_kernel<false>), g_sm_lds_done);
        if (e == hipSuccess)
            hipLaunchKernelGGL(lds::stft_mel_kernel<false>, grid, dim3(256), smem, s, audio, lens, L, Fmax, reinterpret_cast<const double2*>(basis), melT, g, out,
                               (double2*)nullptr);
    }
    if (e == hipSuccess) e = hipGetLastError();
    return e == hipSuccess ? LDS_OK : set_error(LDS_EHIP, "%s: %s", fn, hipGetErrorString(e));
}

}  // namespace

extern "C" int lds_stft_mel_workspace_bytes(int n_fft_new, int hop_new, int n_mels, int B, int64_t L, size_t* out) {
    if (!out) return set_error(LDS_EINVAL, "lds_stft_mel_workspace_bytes: null out");
    if (n_fft_new < 4 || hop_new < 1 || n_mels < 1 || B < 1 || L < 1) return set_error(LDS_EINVAL, "lds_stft_mel_workspace_bytes: bad argument");
    *out = 0;      // the spectrum stays in the workgroup: nothing is parked in memory between stages
    return LDS_OK;
}

extern "C" int lds_stft_mel(const float* audio, const int32_t* lengths, const double* basis, const float* mel_basisT, int n_fft_new, int win_new, int hop_new,
                            int n_fft, int win, int n_mels, float clip_val, int F, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    (void)ws; (void)ws_bytes;
    lds::SmGeom g;
    if (int rc = sm_geometry("lds_stft_mel", n_fft_new, win_new, hop_new, n_fft, win, n_mels, clip_val, g)) return rc;
    return sm_run("lds_stft_mel", audio, lengths, basis, mel_basisT, g, F, out, nullptr, B, L, (hipStream_t)stream);
}

extern "C" int lds_test_stft_dft(const float* audio, const double* basis, const float* mel_basisT, int n_fft_new, int hop_new, int n_mels, int F, float* out,
                                 double* dft, int B, int64_t L, void* stream) {
    if (!dft) return set_error(LDS_EINVAL, "lds_test_stft_dft: null pointer");
    lds::SmGeom g;
    if (int rc = sm_geometry("lds_test_stft_dft", n_fft_new, n_fft_new, hop_new, n_fft_new, n_fft_new, n_mels, 1e-5f, g)) return rc;
    g.pad_left = 0;          // frames of the clip as it is
    g.pad_right_min = 0;
    if (int rc = sm_run("lds_test_stft_dft", audio, nullptr, basis, mel_basisT, g, F, out, dft, B, L, (hipStream_t)stream)) return rc;
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? LDS_OK : set_error(LDS_EHIP, "lds_test_stft_dft: %s", hipGetErrorString(e));
}
