// CTC heads on the speech encoders (transformers Wav2Vec2ForCTC / HubertForCTC / WavLMForCTC: lm_head over the last hidden state, then
// torch.nn.functional.ctc_loss / the greedy collapse of Wav2Vec2CTCTokenizer), exact fp32, gfx950.  include/lds.h states the semantics.
//   head     z[n][v] = x_n . w_v + b_v on v_mfma_f32_32x32x2_f32 with kmeans.hip's assign tiling (both operand tiles HBM/L2 -> LDS by
//            LDS-DMA, the same swizzle, the same fmaf chain for every (n, v)) and another epilogue: per frame the running (max, lowest
//            arg-max, rescaled sum of exp) triple lives in registers across the column blocks a workgroup walks.  The N x V matrix is never
//            stored (MODE 1, the optional log-probs, writes z - lse in a second pass of the same tile).  The cut of V into column splits
//            depends on V alone (kCtcCbps blocks per split), so the order of every merge -- and every bit of a frame's result -- is
//            independent of N, T, B and the frame's position.
//   gather   MODE 2: the emissions of the L + 1 distinct columns of a clip (blank, then its labels), W's rows picked by label through the
//            per-lane source address of the DMA; written minus lse as E [B][T][Lmax + 1].
//   collapse one workgroup per clip, a prefix sum over the run heads.
//   forward / viterbi  ONE wave per clip: a lane owns 16 contiguous states of the S = 2 L + 1 trellis in registers (state 16 lane is a
//            blank), only alpha[15] of the lower lane crosses lanes each frame, no workgroup barrier in the time loop, emission rows
//            fetched kCtcAhead frames ahead.  Viterbi back-pointers are 2 bits per state = one dword per lane per frame (one 256-byte
//            store); the backtrace fetches 16 whole back-pointer rows at a time (they do not depend on the state walked) and picks the
//            dword by lane.
#include "../../include/lds.h"
#include "../../include/lds_test.h"
#include "kernels.h"
#include "host.h"

#include <math.h>

namespace lds {

typedef float cf32x16 __attribute__((ext_vector_type(16)));
typedef float cf32x4 __attribute__((ext_vector_type(4)));

constexpr int kCtcB = 128;                 // frames / columns per tile
constexpr int kCtcBK = 32;                 // d per K-step: one 128-byte line of every row
constexpr int kCtcTile = kCtcB * kCtcBK;   // floats per operand tile
constexpr int kCtcOob = 0x7fff0000;        // a buffer offset beyond every slab: the DMA stores zeros
constexpr int kCtcCbps = 4;                // column blocks per split: a function of nothing, so the merge order depends on V alone
constexpr int kCtcAhead = 4;               // frames of emissions in flight in the recursions
constexpr int kCtcMaxL = 511;

struct CtcLens { int B, T; int v[64]; };                    // B clips of T rows, v[b] valid rows
struct CtcLabs { int Lmax, blank, V; int len[64]; };        // the gathered form: labels dev int64 [B][Lmax], len[b] of them used

// (max, lowest index among equal maxima, sum of exp(z - max)) of two disjoint column sets -> of their union.  exp never sees a positive
// argument; an empty side (max = -inf) is skipped, so nothing computes -inf - -inf.
static __device__ __forceinline__ void ctc_merge(float& m, int& i, float& s, float m2, int i2, float s2) {
    if (m2 == -INFINITY) return;
    if (m == -INFINITY) { m = m2; i = i2; s = s2; return; }
    if (m2 > m || (m2 == m && i2 < i)) {
        s = __fadd_rn(__fmul_rn(s, expf(m - m2)), s2);
        m = m2;
        i = i2;
    } else {
        s = __fadd_rn(s, __fmul_rn(s2, expf(m2 - m)));
    }
}

// 256 threads = 2 x 2 waves; wave (wm, wn) owns columns wm*64 .. +64 (MFMA rows, spread over the accumulator registers) and frames
// wn*64 .. +64 (MFMA columns, one per lane) of a 128 x 128 tile: kmeans_assign_kernel's tiling, LDS image and DMA addressing.
// MODE 0: grid (row blocks of N = B T, column splits): (arg, m, lse) per frame, or the split's partial triple into `part`.
// MODE 1: the same grid: out[n][v] = z - lse[n] (zeros in padded rows).
// MODE 2: grid (row blocks of T, column blocks of Lmax + 1, B): out[b][t][j] = x . w_{col(j)} + b_{col(j)} - lse, col(0) = blank,
//         col(j) = labels[b][j - 1]; a label outside [0, V) or equal to blank reads the blank's row and raises bad[b].
template <int MODE>
__global__ void __launch_bounds__(256) ctc_head_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias, int V, int D,
                                                       int cb_per_split, int* __restrict__ arg_out, float* __restrict__ m_out, float* __restrict__ lse,
                                                       float* __restrict__ part, float* __restrict__ out, const long long* __restrict__ labels,
                                                       int* __restrict__ bad, const CtcLens lens, const CtcLabs labs) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kCtcTile];      // 2 stages x (X tile, W tile) = 64 KB
    __shared__ float sbias[kCtcB];
    __shared__ int ssrc[kCtcB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const long long N = (long long)lens.B * lens.T;
    const int clip = MODE == 2 ? (int)blockIdx.z : 0;
    long long n0;
    int rows;
    if constexpr (MODE == 2) {
        const int t0 = blockIdx.x * kCtcB;
        rows = lens.v[clip] - t0;
        if (rows <= 0) return;                                              // (uniform: before any barrier)
        rows = rows < kCtcB ? rows : kCtcB;
        n0 = (long long)clip * lens.T + t0;
    } else {
        n0 = (long long)blockIdx.x * kCtcB;
        rows = (int)((N - n0) < kCtcB ? (N - n0) : kCtcB);
    }
    const int ncol = MODE == 2 ? labs.Lmax + 1 : V;                         // columns of the product
    const int nCB = (ncol + kCtcB - 1) / kCtcB;
    const int cb0 = blockIdx.y * cb_per_split;
    const int cb1 = cb0 + cb_per_split < nCB ? cb0 + cb_per_split : nCB;
    const int nk = (D + kCtcBK - 1) / kCtcBK;
    if constexpr (MODE == 2) {                                              // (cb_per_split is 1: one column block per workgroup)
        if (tid < kCtcB) {
            const int j = cb0 * kCtcB + tid;
            int src = labs.blank;
            if (j >= 1 && j <= labs.len[clip]) {
                const long long l = labels[(long long)clip * labs.Lmax + j - 1];
                if (l < 0 || l >= labs.V || l == labs.blank) bad[clip] = 1;      // (every writer stores the same value)
                else src = (int)l;
            }
            ssrc[tid] = src;
            sbias[tid] = bias[src];
        }
        __syncthreads();
    }
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X + n0 * D), 0, rows * D * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, V * D * 4, 0x00020000);
    int xoff[4], crow[4], kch[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        crow[i] = row;
        kch[i] = ch * 4;
        xoff[i] = (row < rows ? row : rows - 1) * D * 4 + ch * 16;      // rows beyond N read the last row (their results are not stored)
        if constexpr (MODE != 2) {                                      // a padded row is not read: the DMA stores zeros for it
            const long long n = n0 + (row < rows ? row : rows - 1);
            if ((int)(n % lens.T) >= lens.v[n / lens.T]) xoff[i] = kCtcOob;
        }
        if constexpr (MODE == 2) crow[i] = ssrc[row];                   // the gathered source row of W
    }
    auto issue = [&](int cb, int ks, float* st) {
        const int k0 = ks * kCtcBK;
        const bool tail = k0 + kCtcBK > D;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int kr;
            if constexpr (MODE == 2) {
                kr = crow[i];
            } else {
                kr = cb * kCtcB + crow[i];
                kr = kr < V ? kr : V - 1;                               // columns beyond V read the last one (masked in the epilogue)
            }
            int vx = xoff[i], vc = kr * D * 4 + kch[i] * 4;
            if (tail && k0 + kch[i] >= D) vx = vc = kCtcOob;            // d beyond D: zeros for both operands
            float* dst = st + (wave * 4 + i) * 256;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)dst, 16, vx, k0 * 4, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, (__attribute__((address_space(3))) void*)(dst + kCtcTile), 16, vc, k0 * 4, 0, 0);
        }
    };
    int pos[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) pos[g] = ((2 * g + h) ^ ((c >> 1) & 7)) * 4;
    cf32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float rm[2] = {-INFINITY, -INFINITY}, rs[2] = {0.f, 0.f};      // running maximum and sum of exp(z - maximum) of the lane's columns
    int ri[2] = {0, 0};
    // the lane's two frames (MODE 1 / 2: their lse and whether they are stored)
    float flse[2] = {0.f, 0.f};
    bool fpad[2] = {false, false};
    if constexpr (MODE != 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = wn * 64 + j * 32 + c;
            if (row < rows) {
                const long long n = n0 + row;
                fpad[j] = MODE == 1 && (int)(n % lens.T) >= lens.v[n / lens.T];
                if (!fpad[j]) flse[j] = lse[n];
            }
        }
    }

    const int total = (cb1 - cb0) * nk;
    int cb = cb0, ks = 0;           // the tile being computed
    int icb = cb0, iks = 0;         // the tile being fetched
    if (total > 0) issue(icb, iks, smem);
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();            // tile s has landed for everyone; everyone has finished reading tile s - 1
        if (s + 1 < total) {
            if (++iks == nk) { iks = 0; ++icb; }
            issue(icb, iks, smem + ((s + 1) & 1) * 2 * kCtcTile);
        }
        const float* xs = smem + (s & 1) * 2 * kCtcTile + (wn * 64 + c) * kCtcBK;
        const float* cs = smem + (s & 1) * 2 * kCtcTile + kCtcTile + (wm * 64 + c) * kCtcBK;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            cf32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const cf32x4*>(cs + i * 32 * kCtcBK + pos[g]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const cf32x4*>(xs + j * 32 * kCtcBK + pos[g]);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][jj], b[j][jj], acc[i][j], 0, 0, 0);
        }
        if (++ks == nk) {           // a column block is complete
            if constexpr (MODE == 0) {
                // z = dot + bias (-inf beyond V); the block's maximum in increasing column order (strict >: lowest index), then the sum
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kidx = cb * kCtcB + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const float bv = kidx < V ? bias[kidx] : -INFINITY;
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j][r] = kidx < V ? __fadd_rn(acc[i][j][r], bv) : -INFINITY;
                    }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float bm = -INFINITY;
                    int bi = 0;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int kidx = cb * kCtcB + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            if (acc[i][j][r] > bm) { bm = acc[i][j][r]; bi = kidx; }
                        }
                    if (bm != -INFINITY) {
                        float bs = 0.f;
                        const float nm = fmaxf(rm[j], bm);
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) bs = __fadd_rn(bs, expf(acc[i][j][r] - nm));
                        rs[j] = __fadd_rn(rm[j] == -INFINITY ? 0.f : __fmul_rn(rs[j], expf(rm[j] - nm)), bs);
                        if (bm > rm[j]) { rm[j] = bm; ri[j] = bi; }
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kloc = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const int kidx = cb * kCtcB + kloc;
                        if (kidx < ncol) {
                            const float bv = MODE == 2 ? sbias[kloc] : bias[kidx];
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const int row = wn * 64 + j * 32 + c;
                                if (row < rows) out[(n0 + row) * ncol + kidx] = fpad[j] ? 0.f : __fsub_rn(__fadd_rn(acc[i][j][r], bv), flse[j]);
                            }
                        }
                    }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
            ks = 0;
            ++cb;
        }
    }
    if constexpr (MODE == 0) {
        __syncthreads();
        float* qv = smem;
        float* qs = smem + 4 * kCtcB;
        int* qi = reinterpret_cast<int*>(smem + 8 * kCtcB);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int at = (wm * 2 + h) * kCtcB + wn * 64 + j * 32 + c;
            qv[at] = rm[j];
            qs[at] = rs[j];
            qi[at] = ri[j];
        }
        __syncthreads();
        if (tid < rows) {
            float bm = qv[tid], bs = qs[tid];
            int bi = qi[tid];
#pragma unroll
            for (int q = 1; q < 4; ++q) ctc_merge(bm, bi, bs, qv[q * kCtcB + tid], qi[q * kCtcB + tid], qs[q * kCtcB + tid]);
            const long long n = n0 + tid;
            if (part) {
                float* p = part + ((long long)blockIdx.y * N + n) * 3;
                p[0] = bm;
                p[1] = bs;
                reinterpret_cast<int*>(p)[2] = bi;
            } else {
                const bool padded = (int)(n % lens.T) >= lens.v[n / lens.T];
                arg_out[n] = padded ? -1 : bi;
                m_out[n] = padded ? 0.f : bm;
                lse[n] = padded ? 0.f : __fadd_rn(bm, logf(bs));
            }
        }
    }
}

// joins the per-split partial triples of a frame in split order
__global__ void __launch_bounds__(256) ctc_join_kernel(const float* __restrict__ part, int KS, int* __restrict__ arg_out, float* __restrict__ m_out,
                                                       float* __restrict__ lse, const CtcLens lens) {
    const long long N = (long long)lens.B * lens.T;
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const bool padded = (int)(n % lens.T) >= lens.v[n / lens.T];
    float bm = 0.f, bs = 1.f;
    int bi = -1;
    if (!padded) {
        const float* p = part + n * 3;
        bm = p[0]; bs = p[1]; bi = reinterpret_cast<const int*>(p)[2];
        for (int q = 1; q < KS; ++q) {
            p = part + ((long long)q * N + n) * 3;
            ctc_merge(bm, bi, bs, p[0], reinterpret_cast<const int*>(p)[2], p[1]);
        }
    }
    arg_out[n] = bi;
    m_out[n] = bm;
    lse[n] = padded ? 0.f : __fadd_rn(bm, logf(bs));
}

// ---- greedy collapse: one workgroup per clip ----
// a run head is a frame whose arg differs from the frame before; it emits when its arg is not the blank.  Thread t owns a contiguous
// piece of the clip; the emitted heads before a piece come from a prefix sum over the pieces' counts.  logprob = the mean of m - lse over
// the run, summed in double in frame order.
__global__ void __launch_bounds__(256) ctc_collapse_kernel(const int* __restrict__ arg, const float* __restrict__ mx, const float* __restrict__ lse, int blank,
                                                           long long pad_id, long long* __restrict__ tokens, int* __restrict__ n_tokens, int* __restrict__ start,
                                                           int* __restrict__ length, float* __restrict__ logprob, const CtcLens lens) {
    __shared__ int cnt[256];
    __shared__ int tot;
    const int b = blockIdx.x, tid = threadIdx.x, T = lens.T, n = lens.v[b];
    const long long base = (long long)b * T;
    const int per = (n + 255) / 256;
    const int t0 = tid * per < n ? tid * per : n, t1 = t0 + per < n ? t0 + per : n;
    int mine = 0;
    for (int t = t0; t < t1; ++t) {
        const int a = arg[base + t];
        mine += a != blank && (t == 0 || arg[base + t - 1] != a);
    }
    cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = cnt[i]; cnt[i] = run; run += v; }
        n_tokens[b] = run;
        tot = run;
    }
    __syncthreads();
    int at = cnt[tid];
    for (int t = t0; t < t1; ++t) {
        const int a = arg[base + t];
        if (a == blank || (t > 0 && arg[base + t - 1] == a)) continue;
        double s = 0.0;
        int e = t;
        for (; e < n && arg[base + e] == a; ++e) s += (double)__fsub_rn(mx[base + e], lse[base + e]);
        tokens[base + at] = a;
        start[base + at] = t;
        length[base + at] = e - t;
        logprob[base + at] = (float)(s / (double)(e - t));
        ++at;
    }
    for (int i = tot + tid; i < T; i += 256) {      // (slots at and beyond the count: no thread writes a token there)
        tokens[base + i] = pad_id;
        start[base + i] = -1;
        length[base + i] = 0;
        logprob[base + i] = 0.f;
    }
}

// ---- the two recursions: one wave per clip ----
// log(exp a + exp b [+ exp c]) around the maximum, whose own term is exactly 1 and is not computed.  The arguments of exp are <= 0 and the
// argument of log lies in [1, 3], where the hardware forms are as good as the library's in ABSOLUTE terms: __expf(x) = exp2(x log2 e) is off
// by at most (1 + |x|) 2^-24 e^x <= 1.4 * 2^-24, __logf(y) = log2(y) ln 2 by at most 2 * 2^-24 (tests/ctc_numpy.py, bound 3).
static __device__ __forceinline__ float ctc_lse2(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return __fadd_rn(m, __logf(__fadd_rn(1.f, __expf(n - m))));
}
static __device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    const float m = fmaxf(hi, c), mid = fminf(hi, c);
    if (m == -INFINITY) return -INFINITY;
    return __fadd_rn(m, __logf(__fadd_rn(__fadd_rn(1.f, __expf(mid - m)), __expf(lo - m))));
}

// E [B][T][Lmax + 1] (column 0 the blank, column j label j - 1), labels dev int64 [B][Lmax] (read for the repeats only), bad dev [B] or
// NULL.  grid (B), 64 threads.  Lane k owns states 16 k .. 16 k + 15; state s even = blank, odd = label (s - 1) / 2, so the lane's labels
// are 8 k .. 8 k + 7 and its emissions are 8 consecutive floats of a row plus the row's first.
// VIT: the maximum instead of the log-sum, ties stay > step > skip; bp dev [B][T][64] receives 2 bits per state (0 stay, 1 step, 2 skip).
template <bool VIT>
__global__ void __launch_bounds__(64) ctc_trellis_kernel(const float* __restrict__ E, const long long* __restrict__ labels, const int* __restrict__ bad,
                                                         float* __restrict__ score, unsigned* __restrict__ bp, int* __restrict__ frame_label,
                                                         int* __restrict__ segments, float* __restrict__ label_logprob, const CtcLens lens,
                                                         const CtcLabs labs) {
    __shared__ int seg0[kCtcMaxL + 1], seg1[kCtcMaxL + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = lens.T, n = lens.v[b], L = labs.len[b], Lmax = labs.Lmax, S = 2 * L + 1, W1 = Lmax + 1;
    const float* Eb = E + (long long)b * T * W1;
    const bool isbad = bad != nullptr && bad[b] != 0;
    // per-lane masks over its 8 labels: bit k = label 8 lane + k exists / may be reached by a skip (it differs from the label before)
    unsigned have = 0, skip = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int l = 8 * lane + k;
        if (l < L) {
            have |= 1u << k;
            if (l >= 1 && labels[(long long)b * Lmax + l] != labels[(long long)b * Lmax + l - 1]) skip |= 1u << k;
        }
    }
    if constexpr (VIT) {
        for (int l = lane; l <= kCtcMaxL; l += 64) { seg0[l] = -1; seg1[l] = -1; }
        for (int t = n + lane; t < T; t += 64) frame_label[(long long)b * T + t] = -1;
        __syncthreads();
    }
    float a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = -INFINITY;
    float eb[kCtcAhead], el[kCtcAhead][8];
    // every load is unconditional and in bounds (a column beyond Lmax reads the row's last, a frame beyond n - 1 the last frame): the mask is
    // applied where the value is used, so no load sits behind a branch and the frames in flight are counted, not waited out
    int col[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k] = 1 + 8 * lane + k < W1 ? 1 + 8 * lane + k : W1 - 1;
    auto fetch = [&](int t, float& ebt, float (&elt)[8]) {
        const float* row = Eb + (long long)t * W1;
        ebt = row[0];
#pragma unroll
        for (int k = 0; k < 8; ++k) elt[k] = row[col[k]];
    };
    if (n > 0 && !isbad) {
        {
            float e0, l0[8];
            fetch(0, e0, l0);
            if (lane == 0) { a[0] = e0; a[1] = L >= 1 ? l0[0] : -INFINITY; }
        }
#pragma unroll
        for (int u = 0; u < kCtcAhead; ++u)
            fetch(1 + u < n ? 1 + u : n - 1, eb[u], el[u]);
        for (int tb = 1; tb < n; tb += kCtcAhead) {
#pragma unroll
            for (int u = 0; u < kCtcAhead; ++u) {
                const int t = tb + u;
                if (t < n) {
                    float below = __shfl_up(a[15], 1, 64);      // the state under this lane's first
                    if (lane == 0) below = -INFINITY;
                    unsigned word = 0;
#pragma unroll
                    for (int q = 15; q >= 0; --q) {             // descending: a[q - 1], a[q - 2] are still the frame before
                        const float x0 = a[q];
                        const float x1 = q >= 1 ? a[q - 1] : below;
                        float v;
                        if (q & 1) {
                            const int k = q >> 1;
                            const float x2 = (skip >> k) & 1 ? (q >= 2 ? a[q - 2] : below) : -INFINITY;
                            if constexpr (VIT) {
                                v = x0;
                                unsigned p = 0;
                                if (x1 > v) { v = x1; p = 1; }
                                if (x2 > v) { v = x2; p = 2; }
                                word |= p << (2 * q);
                            } else {
                                v = ctc_lse3(x0, x1, x2);
                            }
                            v = (have >> k) & 1 ? __fadd_rn(v, el[u][k]) : -INFINITY;
                        } else {
                            if constexpr (VIT) {
                                v = x0;
                                if (x1 > v) { v = x1; word |= 1u << (2 * q); }
                            } else {
                                v = ctc_lse2(x0, x1);
                            }
                            v = 16 * lane + q < S ? __fadd_rn(v, eb[u]) : -INFINITY;
                        }
                        a[q] = v;
                    }
                    if constexpr (VIT) bp[((long long)b * T + t) * 64 + lane] = word;
                    fetch(t + kCtcAhead < n ? t + kCtcAhead : n - 1, eb[u], el[u]);
                }
            }
        }
    }
    // the two final states: S - 1 (the last blank) and S - 2 (the last label)
    float v1 = -INFINITY, v2 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (16 * lane + q == S - 1) v1 = a[q];
        if (16 * lane + q == S - 2) v2 = a[q];
    }
    v1 = __shfl(v1, (S - 1) >> 4, 64);
    v2 = L >= 1 ? __shfl(v2, (S - 2) >> 4, 64) : -INFINITY;
    if (n == 0) v1 = (L == 0 && !isbad) ? 0.f : -INFINITY;
    if constexpr (!VIT) {
        if (lane == 0) score[b] = -ctc_lse2(v1, v2);
        return;
    } else {
        const float best = fmaxf(v1, v2);
        if (lane == 0) score[b] = best;
        const bool feasible = best != -INFINITY && n > 0;
        int s = __builtin_amdgcn_readfirstlane(v1 >= v2 ? S - 1 : S - 2);      // a tie ends in the blank
        int* fl = frame_label + (long long)b * T;
        const unsigned* bpb = bp + (long long)b * T * 64;
        int above = -2;      // the label of the frame after the chunk (-2: none)
        for (int tc = n > 0 ? ((n - 1) >> 6) << 6 : -1; tc >= 0; tc -= 64) {
            const int hi = tc + 63 < n - 1 ? tc + 63 : n - 1;
            int mylab = -1;
            if (feasible) {
                for (int tg = hi; tg >= tc; tg -= 16) {
                    unsigned w[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) w[u] = bpb[(long long)(tg - u > 0 ? tg - u : 0) * 64 + lane];      // (unconditional; row 0 is never used)
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int t = tg - u;
                        if (t >= tc) {
                            if (lane == (t & 63)) mylab = s & 1 ? (s - 1) >> 1 : -1;
                            if (t >= 1) {
                                const unsigned word = __builtin_amdgcn_readlane(w[u], s >> 4);
                                s = __builtin_amdgcn_readfirstlane(s - (int)((word >> (2 * (s & 15))) & 3u));
                            }
                        }
                    }
                }
            }
            const int t = tc + lane;
            if (t <= hi) fl[t] = mylab;
            // run boundaries of the chunk: a label's frames are contiguous
            int up = __shfl_down(mylab, 1, 64);
            if (lane == 63 || t == hi) up = above;
            const int dn = __shfl_up(mylab, 1, 64);
            if (t <= hi && mylab >= 0) {
                if (up != mylab) seg1[mylab] = t + 1;
                if (lane > 0 ? dn != mylab : tc == 0) seg0[mylab] = t;
            }
            // the start of a run whose first frame is the first of the chunk above shows only now
            const int top = __shfl(mylab, hi - tc, 64);
            if (lane == 0 && above >= 0 && above != top) seg0[above] = hi + 1;
            above = __shfl(mylab, 0, 64);
        }
        __syncthreads();
        for (int l = lane; l < Lmax; l += 64) {
            const int f0 = l < L ? seg0[l] : -1, f1 = l < L ? seg1[l] : -1;
            segments[((long long)b * Lmax + l) * 2] = f0;
            segments[((long long)b * Lmax + l) * 2 + 1] = f1;
            double sum = 0.0;
            for (int t = f0; t < f1; ++t) sum += (double)Eb[(long long)t * W1 + 1 + l];
            label_logprob[(long long)b * Lmax + l] = f1 > f0 ? (float)(sum / (double)(f1 - f0)) : 0.f;
        }
    }
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h, include/lds_test.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

using lds::set_error;

struct CtcPlan {
    int KS;                     // column splits of the head
    size_t o_part, o_arg, o_m, o_lse, o_E, o_bad, o_bp, bytes;
};

int ctc_check_bt(const char* fn, int B, int T) {
    LDS_TRY(range_check(fn, "B", B, 1, 64));
    if (T < 1) return set_error(LDS_EINVAL, "%s: T %d < 1", fn, T);
    if ((long long)B * T > 2147482648LL) return set_error(LDS_EINVAL, "%s: B * T = %lld beyond 2^31 - 1000", fn, (long long)B * T);
    return LDS_OK;
}

int ctc_check_dims(const char* fn, int B, int T, int V, int D) {
    if (D < 8 || D > 4096 || D % 8) return set_error(LDS_EINVAL, "%s: D %d must be a multiple of 8 in 8 .. 4096", fn, D);
    LDS_TRY(range_check(fn, "V", V, 2, 65536));
    return ctc_check_bt(fn, B, T);
}

int ctc_check_lmax(const char* fn, int Lmax) {
    if (Lmax < 1 || Lmax > lds::kCtcMaxL) return set_error(LDS_EINVAL, "%s: Lmax %d outside 1 .. %d", fn, Lmax, lds::kCtcMaxL);
    return LDS_OK;
}

int ctc_lens(const char* fn, int B, int T, const int32_t* n_frames, lds::CtcLens& lens) {
    lens.B = B; lens.T = T;
    return clip_lens_fill(fn, "n_frames", B, T, n_frames, lens.v);
}

int ctc_labs(const char* fn, int B, int Lmax, int blank, int V, const int32_t* label_len, lds::CtcLabs& labs) {
    labs.Lmax = Lmax; labs.blank = blank; labs.V = V;
    return clip_lens_fill(fn, "label_len", B, Lmax, label_len, labs.len);
}

// Lmax = 0: the head alone; align: also the back-pointers
CtcPlan ctc_plan(int B, int T, int V, int Lmax, bool align) {
    CtcPlan p;
    const size_t N = (size_t)B * T;
    const int nCB = (V + lds::kCtcB - 1) / lds::kCtcB;
    p.KS = (nCB + lds::kCtcCbps - 1) / lds::kCtcCbps;
    Slots S;
    p.o_part = S.take(p.KS > 1 ? (size_t)p.KS * N * 12 : 0);
    p.o_arg = S.take(Lmax ? N * 4 : 0);
    p.o_m = S.take(Lmax ? N * 4 : 0);
    p.o_lse = S.take(Lmax ? N * 4 : 0);
    p.o_E = S.take(Lmax ? N * (size_t)(Lmax + 1) * 4 : 0);
    p.o_bad = S.take(Lmax ? 256 : 0);
    p.o_bp = S.take(align ? N * 256 : 0);
    p.bytes = S.o > 256 ? S.o : 256;
    return p;
}

// the statistics of every frame into (arg, m, lse); logprobs may be NULL
void ctc_head_launch(const float* X, const float* W, const float* bias, int V, int D, int32_t* arg, float* m, float* lse, float* logprobs, char* w, const CtcPlan& p,
                     const lds::CtcLens& lens, hipStream_t s) {
    const long long N = (long long)lens.B * lens.T;
    float* part = p.KS > 1 ? (float*)(w + p.o_part) : nullptr;
    lds::CtcLabs none;
    none.Lmax = 0; none.blank = 0; none.V = V;
    for (int i = 0; i < 64; ++i) none.len[i] = 0;
    const dim3 grid((unsigned)((N + lds::kCtcB - 1) / lds::kCtcB), p.KS);
    {
        lds::ProfScope ps(s, "ctc_head", 2.0 * (double)N * V * D, 4.0 * ((double)N * D + (double)V * D * ((N + 127) / 128)));
        hipLaunchKernelGGL(lds::ctc_head_kernel<0>, grid, dim3(256), 0, s, X, W, bias, V, D, lds::kCtcCbps, (int*)arg, m, lse, part, (float*)nullptr,
                           (const long long*)nullptr, (int*)nullptr, lens, none);
    }
    if (p.KS > 1) hipLaunchKernelGGL(lds::ctc_join_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, part, p.KS, (int*)arg, m, lse, lens);
    if (logprobs)
        hipLaunchKernelGGL(lds::ctc_head_kernel<1>, grid, dim3(256), 0, s, X, W, bias, V, D, lds::kCtcCbps, (int*)nullptr, (float*)nullptr, lse, (float*)nullptr,
                           logprobs, (const long long*)nullptr, (int*)nullptr, lens, none);
}

// shared by lds_ctc_score and lds_ctc_align: head statistics, gathered emissions, then the recursion
int ctc_score_align(const char* fn, bool align, const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int blank,
                    const int64_t* labels, const int32_t* label_len, int Lmax, float* score, int32_t* frame_label, int32_t* segments, float* label_logprob,
                    void* ws, size_t ws_bytes, void* stream) {
    if (int rc = ctc_check_dims(fn, B, T, V, D)) return rc;
    if (int rc = ctc_check_lmax(fn, Lmax)) return rc;
    if (blank < 0 || blank >= V) return set_error(LDS_EINVAL, "%s: blank %d outside 0 .. %d", fn, blank, V - 1);
    lds::CtcLens lens;
    lds::CtcLabs labs;
    if (int rc = ctc_lens(fn, B, T, n_frames, lens)) return rc;
    if (int rc = ctc_labs(fn, B, Lmax, blank, V, label_len, labs)) return rc;
    if (!X || !W || !bias || !labels || !score || !ws || (align && (!frame_label || !segments || !label_logprob))) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const CtcPlan p = ctc_plan(B, T, V, Lmax, align);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    int32_t* arg = (int32_t*)(w + p.o_arg);
    float* m = (float*)(w + p.o_m);
    float* lse = (float*)(w + p.o_lse);
    float* E = (float*)(w + p.o_E);
    int* bad = (int*)(w + p.o_bad);
    if (hipMemsetAsync(bad, 0, 256, s) != hipSuccess) return set_error(LDS_EHIP, "%s: hipMemsetAsync failed", fn);
    ctc_head_launch(X, W, bias, V, D, arg, m, lse, nullptr, w, p, lens, s);
    {
        lds::ProfScope ps(s, "ctc_gather", 2.0 * (double)B * T * (Lmax + 1) * D, 4.0 * (double)B * T * D);
        const dim3 grid((unsigned)((T + lds::kCtcB - 1) / lds::kCtcB), (Lmax + 1 + lds::kCtcB - 1) / lds::kCtcB, B);
        hipLaunchKernelGGL(lds::ctc_head_kernel<2>, grid, dim3(256), 0, s, X, W, bias, V, D, 1, (int*)nullptr, (float*)nullptr, lse, (float*)nullptr, E,
                           (const long long*)labels, bad, lens, labs);
    }
    lds::ProfScope ps(s, align ? "ctc_viterbi" : "ctc_forward", 0.0, 4.0 * (double)B * T * (Lmax + 1));
    if (align)
        hipLaunchKernelGGL(lds::ctc_trellis_kernel<true>, dim3(B), dim3(64), 0, s, E, (const long long*)labels, bad, score, (unsigned*)(w + p.o_bp), (int*)frame_label,
                           (int*)segments, label_logprob, lens, labs);
    else
        hipLaunchKernelGGL(lds::ctc_trellis_kernel<false>, dim3(B), dim3(64), 0, s, E, (const long long*)labels, bad, score, (unsigned*)nullptr, (int*)nullptr,
                           (int*)nullptr, (float*)nullptr, lens, labs);
    return launched(fn);
}

}  // namespace

extern "C" int lds_ctc_head_workspace_bytes(int B, int T, int V, int D, size_t* out) {
    if (!out) return set_error(LDS_EINVAL, "lds_ctc_head_workspace_bytes: null out");
    if (int rc = ctc_check_dims("lds_ctc_head_workspace_bytes", B, T, V, D)) return rc;
    *out = ctc_plan(B, T, V, 0, false).bytes;
    return LDS_OK;
}

extern "C" int lds_ctc_head(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int32_t* arg, float* m,
                            float* lse, float* logprobs_out, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "lds_ctc_head";
    if (int rc = ctc_check_dims(fn, B, T, V, D)) return rc;
    lds::CtcLens lens;
    if (int rc = ctc_lens(fn, B, T, n_frames, lens)) return rc;
    if (!X || !W || !bias || !arg || !m || !lse || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const CtcPlan p = ctc_plan(B, T, V, 0, false);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    ctc_head_launch(X, W, bias, V, D, arg, m, lse, logprobs_out, (char*)ws, p, lens, (hipStream_t)stream);
    return launched(fn);
}

extern "C" int lds_ctc_greedy(const int32_t* arg, const float* m, const float* lse, int B, int T, const int32_t* n_frames, int blank, int64_t pad_id,
                              int64_t* tokens, int32_t* n_tokens, int32_t* start, int32_t* length, float* logprob, void* stream) {
    const char* fn = "lds_ctc_greedy";
    if (int rc = ctc_check_bt(fn, B, T)) return rc;
    if (blank < 0 || blank >= 65536) return set_error(LDS_EINVAL, "%s: blank %d outside 0 .. 65535", fn, blank);
    lds::CtcLens lens;
    if (int rc = ctc_lens(fn, B, T, n_frames, lens)) return rc;
    if (!arg || !m || !lse || !tokens || !n_tokens || !start || !length || !logprob) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipLaunchKernelGGL(lds::ctc_collapse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const int*)arg, m, lse, blank, (long long)pad_id, (long long*)tokens,
                       (int*)n_tokens, (int*)start, (int*)length, logprob, lens);
    return launched(fn);
}

extern "C" int lds_ctc_score_workspace_bytes(int B, int T, int V, int D, int Lmax, size_t* out) {
    const char* fn = "lds_ctc_score_workspace_bytes";
    if (!out) return set_error(LDS_EINVAL, "%s: null out", fn);
    if (int rc = ctc_check_dims(fn, B, T, V, D)) return rc;
    if (int rc = ctc_check_lmax(fn, Lmax)) return rc;
    *out = ctc_plan(B, T, V, Lmax, false).bytes;
    return LDS_OK;
}

extern "C" int lds_ctc_score(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int blank,
                             const int64_t* labels, const int32_t* label_len, int Lmax, float* nll, void* ws, size_t ws_bytes, void* stream) {
    return ctc_score_align("lds_ctc_score", false, X, B, T, n_frames, W, bias, V, D, blank, labels, label_len, Lmax, nll, nullptr, nullptr, nullptr, ws, ws_bytes,
                           stream);
}

extern "C" int lds_ctc_align_workspace_bytes(int B, int T, int V, int D, int Lmax, size_t* out) {
    const char* fn = "lds_ctc_align_workspace_bytes";
    if (!out) return set_error(LDS_EINVAL, "%s: null out", fn);
    if (int rc = ctc_check_dims(fn, B, T, V, D)) return rc;
    if (int rc = ctc_check_lmax(fn, Lmax)) return rc;
    *out = ctc_plan(B, T, V, Lmax, true).bytes;
    return LDS_OK;
}

extern "C" int lds_ctc_align(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int blank,
                             const int64_t* labels, const int32_t* label_len, int Lmax, float* path_score, int32_t* frame_label, int32_t* segments,
                             float* label_logprob, void* ws, size_t ws_bytes, void* stream) {
    return ctc_score_align("lds_ctc_align", true, X, B, T, n_frames, W, bias, V, D, blank, labels, label_len, Lmax, path_score, frame_label, segments,
                           label_logprob, ws, ws_bytes, stream);
}

namespace {
int ctc_test_common(const char* fn, int B, int T, const int32_t* n_frames, const int32_t* label_len, int Lmax, lds::CtcLens& lens, lds::CtcLabs& labs) {
    if (int rc = ctc_check_bt(fn, B, T)) return rc;
    if (int rc = ctc_check_lmax(fn, Lmax)) return rc;
    if (int rc = ctc_lens(fn, B, T, n_frames, lens)) return rc;
    return ctc_labs(fn, B, Lmax, 0, 0, label_len, labs);
}
}  // namespace

extern "C" int lds_test_ctc_forward(const float* E, int B, int T, const int32_t* n_frames, const int64_t* labels, const int32_t* label_len, int Lmax, float* nll,
                                    void* stream) {
    const char* fn = "lds_test_ctc_forward";
    lds::CtcLens lens;
    lds::CtcLabs labs;
    if (int rc = ctc_test_common(fn, B, T, n_frames, label_len, Lmax, lens, labs)) return rc;
    if (!E || !labels || !nll) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipLaunchKernelGGL(lds::ctc_trellis_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, E, (const long long*)labels, (const int*)nullptr, nll,
                       (unsigned*)nullptr, (int*)nullptr, (int*)nullptr, (float*)nullptr, lens, labs);
    return launched(fn);
}

extern "C" int lds_test_ctc_viterbi(const float* E, int B, int T, const int32_t* n_frames, const int64_t* labels, const int32_t* label_len, int Lmax,
                                    float* path_score, int32_t* frame_label, int32_t* segments, float* label_logprob, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "lds_test_ctc_viterbi";
    lds::CtcLens lens;
    lds::CtcLabs labs;
    if (int rc = ctc_test_common(fn, B, T, n_frames, label_len, Lmax, lens, labs)) return rc;
    if (!E || !labels || !path_score || !frame_label || !segments || !label_logprob || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const size_t need = (size_t)B * T * 256;
    if (ws_bytes < need) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    hipLaunchKernelGGL(lds::ctc_trellis_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream, E, (const long long*)labels, (const int*)nullptr, path_score,
                       (unsigned*)ws, (int*)frame_label, (int*)segments, label_logprob, lens, labs);
    return launched(fn);
}
