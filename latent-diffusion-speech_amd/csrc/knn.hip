// Units retrieval (the "units index" of the Diffusion-SVC / RVC tool chains, there an approximate faiss index on the host): exact k-NN of
// every query frame over a speaker's unit pool and the inverse-square blend of the k nearest pool rows, fp32, gfx950.
//   search   score of pool row m for query n = x_n . p_m - h_m, h_m = |p_m|^2 / 2 (kmeans.hip's assign score: its arg-max is the arg-min of the
//            squared distance); the k best in descending score order, the lower pool index first among equal scores.  kmeans_assign_kernel's
//            tiling (128 x 128 tiles, both operands by LDS-DMA with the source-side swizzle, v_mfma_f32_32x32x2_f32), so every score of a query
//            row is the same fmaf chain whatever N, the row's position, the slab or the split; the N x M matrix is never stored.  Each lane
//            keeps a sorted list of KT (score, index) pairs for each of its two query columns in registers (KT = k rounded up to 1, 2, 4, 8).
//   slabs    a buffer descriptor addresses 2^31 bytes: the pool is cut into slabs of whole 128-row blocks, each with its own descriptor base.
//   splits   a workgroup walks a contiguous range of pool blocks; the per-split lists go to the workspace as [split][N][KT].
//   blend    one wave per query row merges the splits' lists in split order, recomputes the k distances directly as sum (x - p)^2, forms
//            w = (1 / max(d, 1e-12))^2, normalises and writes y = (1 - ratio) x + ratio sum w_j p_j.
//   cosine   (kNN-VC's matching) the same tiles with another epilogue: score = (x_n . p_m) r_m, r_m = 1 / max(|p_m|, 1e-12) in the per-row array
//            that holds h_m otherwise; the reported score is multiplied by r(x_n) after the order is decided (the cosine similarity); the
//            blend's distance is 1/2 sum (x r_x - p_j r_j)^2 = 1 - cos, recomputed directly, and its weights are the inverse squares of the
//            distances or uniform (kNN-VC's plain mean) -- over the ORIGINAL pool rows in both cases.
// No floating-point atomics; every slot of the workspace that is read was written by the same call.
#include "../../include/lds.h"
#include "../../include/lds_test.h"
#include "kernels.h"
#include "host.h"

#include <math.h>

namespace lds {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kKnB = 128;                  // query rows / pool rows per tile
constexpr int kKnBK = 32;                  // d per K-step: one 128-byte line of every row
constexpr int kKnTile = kKnB * kKnBK;      // floats per operand tile
constexpr int kKnOob = 0x7fff0000;         // a buffer offset beyond every slab (slabs are cut below it): the DMA stores zeros
constexpr int kKnNone = 0x7fffffff;        // the index of an empty list entry (score -inf): sorts behind every pool row
constexpr int kKnMaxK = 8;

struct KnLens { int n, T; int v[64]; };    // ragged form: B = n clips of T rows, v[b] valid rows; n = 0: plain

// the cosine row constant of a row whose fp32 sum of squares is s (kmeans.hip km_row_const; include/lds.h): 1 / max(sqrt(s), 1e-12)
static __device__ __forceinline__ float kn_row_const(float s) { return __frcp_rn(fmaxf(__fsqrt_rn(s), 1e-12f)); }
// a row's sum of squares by one wave: lanes stride the columns, one fmaf chain per lane, fixed butterfly (knn_prepare_kernel's order,
// so that a query equal to a pool row gets that row's constant)
static __device__ __forceinline__ float kn_row_sumsq(const float* __restrict__ r, int D, int lane) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(r[d], r[d], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// (score, index) order of the lists: higher score first, the lower index among equal scores
static __device__ __forceinline__ bool kn_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// 256 threads = 2 x 2 waves; wave (wm, wn) owns pool rows wm*64 .. +64 (MFMA rows, spread over the accumulator registers) and queries
// wn*64 .. +64 (MFMA columns, one per lane) of a 128 x 128 tile.  grid (query row blocks, splits).  The LDS image of a tile and the swizzle
// on the source address are kmeans_assign_kernel's.  Pool block b (128 rows) lies in slab b / slab_blocks; a block never straddles two slabs.
// A lane meets the pool rows of a query column in increasing index order, so inserting on a strictly greater score keeps the lower index first.
// MET (LDS_METRIC_*) selects the epilogue only: acc - h_m, or acc * r_m.
template <int KT, int MET>
__global__ void __launch_bounds__(256) knn_topk_kernel(const float* __restrict__ X, long long N, const float* __restrict__ P, const float* __restrict__ hh,
                                                       int M, int D, int slab_blocks, int pb_per_split, float* __restrict__ lval, int* __restrict__ lidx) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kKnTile];      // 2 stages x (X tile, P tile) = 64 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const long long n0 = (long long)blockIdx.x * kKnB;
    const int rows = (int)((N - n0) < kKnB ? (N - n0) : kKnB);
    const int nPB = (M + kKnB - 1) / kKnB;
    const int pb0 = blockIdx.y * pb_per_split;
    const int pb1 = pb0 + pb_per_split < nPB ? pb0 + pb_per_split : nPB;
    const int nk = (D + kKnBK - 1) / kKnBK;
    const int slab_rows = slab_blocks * kKnB;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X + n0 * D), 0, rows * D * 4, 0x00020000);
    int xoff[4], crow[4], kch[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        crow[i] = row;
        kch[i] = ch * 4;
        xoff[i] = (row < rows ? row : rows - 1) * D * 4 + ch * 16;      // rows beyond N read the last row (their lists are not stored)
    }
    auto issue = [&](int pb, int ks, float* st) {
        const int k0 = ks * kKnBK;
        const bool tail = k0 + kKnBK > D;
        const int slab = pb / slab_blocks;                                     // wave-uniform: the descriptor lives in scalar registers
        const int r0 = slab * slab_rows;                                       // the slab's first pool row; it holds srows of them
        const int srows = M - r0 < slab_rows ? M - r0 : slab_rows;
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P + (long long)r0 * D), 0, srows * D * 4, 0x00020000);
        const int b0 = pb * kKnB - r0;                                         // the block's first row inside the slab
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int pr = b0 + crow[i];
            pr = pr < srows ? pr : srows - 1;                                  // pool rows beyond M read the last one (masked in the epilogue)
            int vx = xoff[i], vp = pr * D * 4 + kch[i] * 4;
            if (tail && k0 + kch[i] >= D) vx = vp = kKnOob;                     // d beyond D: zeros for both operands
            float* dst = st + (wave * 4 + i) * 256;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)dst, 16, vx, k0 * 4, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rp, (__attribute__((address_space(3))) void*)(dst + kKnTile), 16, vp, k0 * 4, 0, 0);
        }
    };
    int pos[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) pos[g] = ((2 * g + h) ^ ((c >> 1) & 7)) * 4;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float lv[2][KT];
    int li[2][KT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < KT; ++p) { lv[j][p] = -INFINITY; li[j][p] = kKnNone; }

    const int total = (pb1 - pb0) * nk;
    int pb = pb0, ks = 0;           // the tile being computed
    int ipb = pb0, iks = 0;         // the tile being fetched
    issue(ipb, iks, smem);
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();            // tile s has landed for everyone; everyone has finished reading tile s - 1
        if (s + 1 < total) {
            if (++iks == nk) { iks = 0; ++ipb; }
            issue(ipb, iks, smem + ((s + 1) & 1) * 2 * kKnTile);
        }
        const float* xs = smem + (s & 1) * 2 * kKnTile + (wn * 64 + c) * kKnBK;
        const float* ps = smem + (s & 1) * 2 * kKnTile + kKnTile + (wm * 64 + c) * kKnBK;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const f32x4*>(ps + i * 32 * kKnBK + pos[g]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f32x4*>(xs + j * 32 * kKnBK + pos[g]);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][jj], b[j][jj], acc[i][j], 0, 0, 0);
        }
        if (++ks == nk) {           // a pool block is complete: scores into the lists, in increasing pool index
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = pb * kKnB + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float hv = m < M ? hh[m] : (MET == LDS_METRIC_COSINE ? 0.f : INFINITY);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        float v;
                        if constexpr (MET == LDS_METRIC_COSINE) v = m < M ? acc[i][j][r] * hv : -INFINITY;
                        else v = acc[i][j][r] - hv;
                        acc[i][j][r] = 0.f;
                        if (v > lv[j][KT - 1]) {      // (a NaN score, or -inf beyond M, never enters)
#pragma unroll
                            for (int p = KT - 1; p >= 0; --p) {
                                const bool up = p > 0 && v > lv[j][p > 0 ? p - 1 : 0];      // the entry above moves down into p
                                const bool here = v > lv[j][p];
                                lv[j][p] = up ? lv[j][p > 0 ? p - 1 : 0] : (here ? v : lv[j][p]);
                                li[j][p] = up ? li[j][p > 0 ? p - 1 : 0] : (here ? m : li[j][p]);
                            }
                        }
                    }
                }
            ks = 0;
            ++pb;
        }
    }
    __syncthreads();
    // the four lists of a query (two wm waves x two half-waves) meet in LDS: [list q][entry p][query], 4 * KT * 128 values and as many indices
    float* rv = smem;
    int* ri = reinterpret_cast<int*>(smem + 4 * KT * kKnB);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < KT; ++p) {
            rv[((wm * 2 + h) * KT + p) * kKnB + wn * 64 + j * 32 + c] = lv[j][p];
            ri[((wm * 2 + h) * KT + p) * kKnB + wn * 64 + j * 32 + c] = li[j][p];
        }
    __syncthreads();
    if (tid < rows) {
        int at[4] = {0, 0, 0, 0};
        const long long o = ((long long)blockIdx.y * N + n0 + tid) * KT;
        for (int p = 0; p < KT; ++p) {
            float bv = -INFINITY;
            int bi = kKnNone, bq = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int a = at[q] < KT ? at[q] : KT - 1;
                const float v = at[q] < KT ? rv[(q * KT + a) * kKnB + tid] : -INFINITY;
                const int i = at[q] < KT ? ri[(q * KT + a) * kKnB + tid] : kKnNone;
                if (kn_before(v, i, bv, bi)) { bv = v; bi = i; bq = q; }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) at[q] += (q == bq && bi != kKnNone) ? 1 : 0;
            lval[o + p] = bv;
            lidx[o + p] = bi;
        }
    }
}

// the final list of a query row: the splits' lists merged in split order under the same rule.  Entries whose index is not a pool row (the
// empty entries of a split that holds fewer than KT rows) are dropped.  bv / bi: 8 entries, (-inf, kKnNone) where fewer than 8 exist.
static __device__ __forceinline__ void kn_merge(const float* __restrict__ lval, const int* __restrict__ lidx, int S, int KT, long long N, long long n, int M,
                                                float (&bv)[kKnMaxK], int (&bi)[kKnMaxK]) {
#pragma unroll
    for (int q = 0; q < kKnMaxK; ++q) { bv[q] = -INFINITY; bi[q] = kKnNone; }
    for (int s = 0; s < S; ++s) {
        const long long o = ((long long)s * N + n) * KT;
        for (int p = 0; p < KT; ++p) {
            const float v = lval[o + p];
            const int i = lidx[o + p];
            if (i < 0 || i >= M) break;                                        // the list is sorted: only empty entries follow
            if (!kn_before(v, i, bv[kKnMaxK - 1], bi[kKnMaxK - 1])) break;     // nor can a later entry of this list enter
#pragma unroll
            for (int q = kKnMaxK - 1; q >= 0; --q) {
                const bool up = q > 0 && kn_before(v, i, bv[q > 0 ? q - 1 : 0], bi[q > 0 ? q - 1 : 0]);
                const bool here = kn_before(v, i, bv[q], bi[q]);
                bv[q] = up ? bv[q > 0 ? q - 1 : 0] : (here ? v : bv[q]);
                bi[q] = up ? bi[q > 0 ? q - 1 : 0] : (here ? i : bi[q]);
            }
        }
    }
}

// search only: one thread per query row writes idx [N][k] (-1 where the row has fewer than k comparable scores: a NaN query) and the scores
__global__ void __launch_bounds__(256) knn_select_kernel(const float* __restrict__ lval, const int* __restrict__ lidx, int S, int KT, long long N, int M, int k,
                                                         int* __restrict__ idx, float* __restrict__ score) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float bv[kKnMaxK];
    int bi[kKnMaxK];
    kn_merge(lval, lidx, S, KT, N, n, M, bv, bi);
#pragma unroll
    for (int q = 0; q < kKnMaxK; ++q)
        if (q < k) {
            idx[n * k + q] = bi[q] == kKnNone ? -1 : bi[q];
            if (score) score[n * k + q] = bv[q];
        }
}

// the cosine search's select: one wave per query row (4 rows per workgroup), every lane merges the row's lists; the scores leave multiplied
// by r(x_n) -- after the order is decided -- so that they are cosine similarities.  A missing place keeps -1 / -inf.
__global__ void __launch_bounds__(256) knn_select_cos_kernel(const float* __restrict__ X, int D, const float* __restrict__ lval, const int* __restrict__ lidx, int S,
                                                             int KT, long long N, int M, int k, int* __restrict__ idx, float* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float bv[kKnMaxK];
    int bi[kKnMaxK];
    kn_merge(lval, lidx, S, KT, N, n, M, bv, bi);
    const float rx = kn_row_const(kn_row_sumsq(X + n * D, D, lane));
#pragma unroll
    for (int q = 0; q < kKnMaxK; ++q)
        if (q < k && lane == q) {
            idx[n * k + q] = bi[q] == kKnNone ? -1 : bi[q];
            if (score) score[n * k + q] = bi[q] == kKnNone ? -INFINITY : __fmul_rn(bv[q], rx);
        }
}

// One wave per query row (4 rows per workgroup).  Every lane merges the row's lists (the same addresses in all lanes); lane l then takes the
// columns 4 (l + 64 t) .. + 4 of x and of the k pool rows: d_j = sum (x - p_j)^2 by one fmaf chain per lane in ascending column order and
// a fixed butterfly over the lanes, d_j = max(d_j, 1e-12), w_j = (1 / d_j)^2, normalised by their sum taken for j ascending;
// z = w_0 p_0, then fmaf for j ascending; y = x at ratio 0, z at ratio 1, fmaf(ratio, z, (1 - ratio) x) between.  Every pool index is clamped
// into [0, M) before it forms an address; an entry that is no pool row has weight 0.  Rows at and beyond a clip's length: y = 0, idx = -1, dist = 0.
// MET = cosine: r_x = the row constant of x formed by this wave, r_j = hh[index] (lds_knn_prepare_metric's, original pool order),
// d_j = 1/2 sum (x r_x - p_j r_j)^2 in the same order, floored alike.  WTS = uniform: w_j = 1 / found over the entries that are pool rows.
template <int MET, int WTS>
__global__ void __launch_bounds__(256) knn_blend_kernel(const float* __restrict__ X, long long N, const float* __restrict__ P, const float* __restrict__ hh, int M, int D,
                                                        const float* __restrict__ lval, const int* __restrict__ lidx, int S, int KT, int k, float ratio,
                                                        float* __restrict__ Y, int* __restrict__ idx, float* __restrict__ dist, const KnLens lens) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int D4 = D >> 2;
    f32x4* y = reinterpret_cast<f32x4*>(Y + n * D);
    if (lens.n > 0 && (int)(n % lens.T) >= lens.v[n / lens.T]) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int t = lane; t < D4; t += 64) y[t] = zero;
        if (lane < k) {
            if (idx) idx[n * k + lane] = -1;
            if (dist) dist[n * k + lane] = 0.f;
        }
        return;
    }
    float bv[kKnMaxK];
    int bi[kKnMaxK];
    kn_merge(lval, lidx, S, KT, N, n, M, bv, bi);
    const f32x4* x = reinterpret_cast<const f32x4*>(X + n * D);
    const f32x4* pr[kKnMaxK];
    bool ok[kKnMaxK];
#pragma unroll
    for (int j = 0; j < kKnMaxK; ++j) {
        ok[j] = j < k && bi[j] >= 0 && bi[j] < M;
        const int m = bi[j] < 0 ? 0 : (bi[j] >= M ? M - 1 : bi[j]);
        pr[j] = reinterpret_cast<const f32x4*>(P + (long long)m * D);
    }
    float d[kKnMaxK];
#pragma unroll
    for (int j = 0; j < kKnMaxK; ++j) d[j] = 0.f;
    if constexpr (MET == LDS_METRIC_COSINE) {
        const float rx = kn_row_const(kn_row_sumsq(X + n * D, D, lane));
        float rj[kKnMaxK];
#pragma unroll
        for (int j = 0; j < kKnMaxK; ++j) rj[j] = ok[j] ? hh[bi[j]] : 0.f;
        for (int t = lane; t < D4; t += 64) {
            const f32x4 xv = x[t];
#pragma unroll
            for (int j = 0; j < kKnMaxK; ++j)
                if (j < k) {
                    const f32x4 pv = pr[j][t];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float u = __fsub_rn(__fmul_rn(xv[e], rx), __fmul_rn(pv[e], rj[j]));
                        d[j] = fmaf(u, u, d[j]);
                    }
                }
        }
    } else {
        for (int t = lane; t < D4; t += 64) {
            const f32x4 xv = x[t];
#pragma unroll
            for (int j = 0; j < kKnMaxK; ++j)
                if (j < k) {
                    const f32x4 pv = pr[j][t];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float u = xv[e] - pv[e];
                        d[j] = fmaf(u, u, d[j]);
                    }
                }
        }
    }
    float w[kKnMaxK], sum = 0.f;
    int found = 0;
#pragma unroll
    for (int j = 0; j < kKnMaxK; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d[j] += __shfl_xor(d[j], o, 64);
        if constexpr (MET == LDS_METRIC_COSINE) d[j] = __fmul_rn(0.5f, d[j]);
        d[j] = fmaxf(d[j], 1e-12f);
        const float r = __fdiv_rn(1.0f, d[j]);
        w[j] = ok[j] ? __fmul_rn(r, r) : 0.f;
        if (j < k) sum = __fadd_rn(sum, w[j]);
        found += ok[j] ? 1 : 0;
    }
    if constexpr (WTS == LDS_WEIGHTS_UNIFORM) {
        const float u = __fdiv_rn(1.0f, (float)(found > 0 ? found : 1));
#pragma unroll
        for (int j = 0; j < kKnMaxK; ++j) w[j] = ok[j] ? u : 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < kKnMaxK; ++j) w[j] = __fdiv_rn(w[j], sum);
    }
    const float keep = 1.0f - ratio;
    for (int t = lane; t < D4; t += 64) {
        const f32x4 xv = x[t];
        f32x4 z;
        {
            const f32x4 pv = pr[0][t];
#pragma unroll
            for (int e = 0; e < 4; ++e) z[e] = __fmul_rn(w[0], pv[e]);
        }
#pragma unroll
        for (int j = 1; j < kKnMaxK; ++j)
            if (j < k) {
                const f32x4 pv = pr[j][t];
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = fmaf(w[j], pv[e], z[e]);
            }
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = ratio == 0.f ? xv[e] : (ratio == 1.f ? z[e] : fmaf(ratio, z[e], __fmul_rn(keep, xv[e])));
        y[t] = out;
    }
#pragma unroll
    for (int j = 0; j < kKnMaxK; ++j)
        if (j < k && lane == j) {
            if (idx) idx[n * k + j] = ok[j] ? bi[j] : -1;
            if (dist) dist[n * k + j] = d[j];
        }
}

// h[m] = |p_m|^2 / 2 (metric L2) or r_m = 1 / max(|p_m|, 1e-12) (cosine): one wave per pool row, lanes stride the columns, fixed butterfly
// (a duplicated row gets the same value)
__global__ void __launch_bounds__(256) knn_prepare_kernel(const float* __restrict__ P, long long M, int D, float* __restrict__ hh, int metric) {
    const int lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* r = P + m * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(r[d], r[d], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) hh[m] = metric == LDS_METRIC_COSINE ? kn_row_const(s) : 0.5f * s;
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h, include/lds_test.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

using lds::set_error;

constexpr long long kKnMaxM = 16777216LL;
constexpr long long kKnMaxN = 2147483000LL;
constexpr int kKnMaxSplits = 64;

struct KnPlan {
    int KT;                     // the list length: k rounded up to 1, 2, 4, 8
    int slab_blocks;            // 128-row pool blocks per slab
    int S, pbps;                // splits, pool blocks per split
    size_t o_val, o_idx, bytes;
};

int kn_check_dims(const char* fn, long long N, long long M, int D, int k) {
    if (D < 8 || D > 4096 || D % 8) return set_error(LDS_EINVAL, "%s: D %d must be a multiple of 8 in 8 .. 4096", fn, D);
    if (M < 1 || M > kKnMaxM) return set_error(LDS_EINVAL, "%s: M %lld outside 1 .. 16777216", fn, M);
    if (k < 1 || k > lds::kKnMaxK || k > M) return set_error(LDS_EINVAL, "%s: k %d outside 1 .. min(8, M = %lld)", fn, k, M);
    if (N < 1 || N > kKnMaxN) return set_error(LDS_EINVAL, "%s: N %lld outside 1 .. 2147483000", fn, N);
    return LDS_OK;
}

// the most pool rows one buffer descriptor takes: whole 128-row blocks below the out-of-range offset the DMA tail uses (itself below 2^31 - 1)
int kn_slab_rows(int D) {
    const long long r = ((long long)lds::kKnOob / (4LL * D)) / lds::kKnB * lds::kKnB;
    return (int)(r < kKnMaxM ? r : kKnMaxM);
}

// slab_rows / splits 0: the library's choice
KnPlan kn_plan(long long N, long long M, int D, int k, int slab_rows, int splits) {
    KnPlan p;
    p.KT = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8;
    p.slab_blocks = (slab_rows > 0 ? slab_rows : kn_slab_rows(D)) / lds::kKnB;
    const long long rb = (N + lds::kKnB - 1) / lds::kKnB;
    const int nPB = (int)((M + lds::kKnB - 1) / lds::kKnB);
    long long s = splits > 0 ? splits : (rb >= 512 ? 1 : 512 / rb);      // enough workgroups for two per CU when the row blocks alone do not give them
    if (s > kKnMaxSplits) s = kKnMaxSplits;
    if (s > nPB) s = nPB;
    p.pbps = (int)((nPB + s - 1) / s);
    p.S = (nPB + p.pbps - 1) / p.pbps;
    Slots S;
    p.o_val = S.take((size_t)p.S * (size_t)N * p.KT * 4);
    p.o_idx = S.take((size_t)p.S * (size_t)N * p.KT * 4);
    p.bytes = S.o;
    return p;
}

bool kn_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int kn_check_metric(const char* fn, int metric, int weights) {
    if (metric != LDS_METRIC_L2 && metric != LDS_METRIC_COSINE) return set_error(LDS_EINVAL, "%s: metric %d is neither LDS_METRIC_L2 nor LDS_METRIC_COSINE", fn, metric);
    if (weights != LDS_WEIGHTS_INVERSE_SQUARE && weights != LDS_WEIGHTS_UNIFORM)
        return set_error(LDS_EINVAL, "%s: weights %d is neither LDS_WEIGHTS_INVERSE_SQUARE nor LDS_WEIGHTS_UNIFORM", fn, weights);
    return LDS_OK;
}

void kn_topk(const KnPlan& p, int metric, const float* X, long long N, const float* P, const float* h, int M, int D, float* lval, int* lidx, hipStream_t s) {
    lds::ProfScope ps(s, "knn_topk", 2.0 * (double)N * M * D, 4.0 * ((double)N * D + (double)M * D * ((N + 127) / 128)));
    const dim3 grid((unsigned)((N + lds::kKnB - 1) / lds::kKnB), p.S);
#define LDS_KNN_TOPK(KT_)                                                                                                                              \
    if (metric == LDS_METRIC_COSINE)                                                                                                                   \
        hipLaunchKernelGGL((lds::knn_topk_kernel<KT_, LDS_METRIC_COSINE>), grid, dim3(256), 0, s, X, N, P, h, M, D, p.slab_blocks, p.pbps, lval, lidx); \
    else                                                                                                                                               \
        hipLaunchKernelGGL((lds::knn_topk_kernel<KT_, LDS_METRIC_L2>), grid, dim3(256), 0, s, X, N, P, h, M, D, p.slab_blocks, p.pbps, lval, lidx)
    switch (p.KT) {
        case 1: LDS_KNN_TOPK(1); break;
        case 2: LDS_KNN_TOPK(2); break;
        case 4: LDS_KNN_TOPK(4); break;
        default: LDS_KNN_TOPK(8); break;
    }
#undef LDS_KNN_TOPK
}

// the search's last step: the merged lists as idx / score; the cosine scores leave as similarities
void kn_select(int metric, const float* X, int D, const float* lval, const int* lidx, int S, int KT, long long N, int M, int k, int32_t* idx, float* score, hipStream_t s) {
    if (metric == LDS_METRIC_COSINE)
        hipLaunchKernelGGL(lds::knn_select_cos_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, X, D, lval, lidx, S, KT, N, M, k, (int*)idx, score);
    else
        hipLaunchKernelGGL(lds::knn_select_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, lval, lidx, S, KT, N, M, k, (int*)idx, score);
}

// h: the per-row array of the ORIGINAL pool (read in cosine mode only)
void kn_blend(int metric, int weights, const float* X, long long N, const float* P, const float* h, int M, int D, const float* lval, const int* lidx, int S, int KT,
              int k, float ratio, float* Y, int32_t* idx, float* dist, const lds::KnLens& lens, hipStream_t s) {
    lds::ProfScope ps(s, "knn_blend", 5.0 * (double)N * k * D, 4.0 * (double)N * D * (2.0 * k + 3.0));
    const dim3 grid((unsigned)((N + 3) / 4));
#define LDS_KNN_BLEND(MET_, WTS_) \
    hipLaunchKernelGGL((lds::knn_blend_kernel<MET_, WTS_>), grid, dim3(256), 0, s, X, N, P, h, M, D, lval, lidx, S, KT, k, ratio, Y, (int*)idx, dist, lens)
    if (metric == LDS_METRIC_COSINE) {
        if (weights == LDS_WEIGHTS_UNIFORM) LDS_KNN_BLEND(LDS_METRIC_COSINE, LDS_WEIGHTS_UNIFORM);
        else LDS_KNN_BLEND(LDS_METRIC_COSINE, LDS_WEIGHTS_INVERSE_SQUARE);
    } else {
        if (weights == LDS_WEIGHTS_UNIFORM) LDS_KNN_BLEND(LDS_METRIC_L2, LDS_WEIGHTS_UNIFORM);
        else LDS_KNN_BLEND(LDS_METRIC_L2, LDS_WEIGHTS_INVERSE_SQUARE);
    }
#undef LDS_KNN_BLEND
}

int kn_search(const char* fn, int metric, const float* X, long long N, const float* P, const float* h, long long M, int D, int k, int slab_rows, int splits,
              int32_t* idx, float* score, void* ws, size_t ws_bytes, hipStream_t s) {
    if (int rc = kn_check_metric(fn, metric, LDS_WEIGHTS_INVERSE_SQUARE)) return rc;
    if (int rc = kn_check_dims(fn, N, M, D, k)) return rc;
    if (!X || !P || !h || !idx || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    if (kn_misaligned(X) || kn_misaligned(P)) return set_error(LDS_EINVAL, "%s: X and P must be 16-byte aligned", fn);
    const KnPlan p = kn_plan(N, M, D, k, slab_rows, splits);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    float* lval = (float*)((char*)ws + p.o_val);
    int* lidx = (int*)((char*)ws + p.o_idx);
    kn_topk(p, metric, X, N, P, h, (int)M, D, lval, lidx, s);
    kn_select(metric, X, D, lval, lidx, p.S, p.KT, N, (int)M, k, idx, score, s);
    return launched(fn);
}

int kn_retrieve(const char* fn, int metric, int weights, const float* X, long long N, const float* P, const float* h, long long M, int D, int k, float ratio,
                float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, const lds::KnLens& lens, hipStream_t s) {
    if (int rc = kn_check_metric(fn, metric, weights)) return rc;
    if (int rc = kn_check_dims(fn, N, M, D, k)) return rc;
    if (!(ratio >= 0.f && ratio <= 1.f)) return set_error(LDS_EINVAL, "%s: ratio %g outside 0 .. 1", fn, (double)ratio);
    if (!X || !P || !h || !Y || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    if (kn_misaligned(X) || kn_misaligned(P) || kn_misaligned(Y)) return set_error(LDS_EINVAL, "%s: X, P and Y must be 16-byte aligned", fn);
    const KnPlan p = kn_plan(N, M, D, k, 0, 0);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    float* lval = (float*)((char*)ws + p.o_val);
    int* lidx = (int*)((char*)ws + p.o_idx);
    kn_topk(p, metric, X, N, P, h, (int)M, D, lval, lidx, s);
    kn_blend(metric, weights, X, N, P, h, (int)M, D, lval, lidx, p.S, p.KT, k, ratio, Y, idx, dist, lens, s);
    return launched(fn);
}

lds::KnLens kn_plain() {
    lds::KnLens lens;
    lens.n = 0; lens.T = 1;
    for (int i = 0; i < 64; ++i) lens.v[i] = 0;
    return lens;
}

}  // namespace

namespace {
int kn_prepare(const char* fn, int metric, const float* P, int64_t M, int D, float* h, void* stream) {
    if (int rc = kn_check_metric(fn, metric, LDS_WEIGHTS_INVERSE_SQUARE)) return rc;
    if (int rc = kn_check_dims(fn, 1, M, D, 1)) return rc;
    if (!P || !h) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipLaunchKernelGGL(lds::knn_prepare_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P, (long long)M, D, h, metric);
    return launched(fn);
}

int kn_ragged_lens(const char* fn, int B, int T, const int32_t* lengths, lds::KnLens& lens) {
    if (B < 1 || B > 64 || T < 1) return set_error(LDS_EINVAL, "%s: B %d outside 1 .. 64 or T %d < 1", fn, B, T);
    lens.n = B; lens.T = T;
    return clip_lens_fill(fn, "lengths", B, T, lengths, lens.v);
}
}  // namespace

extern "C" int lds_knn_prepare(const float* P, int64_t M, int D, float* h, void* stream) {
    return kn_prepare("lds_knn_prepare", LDS_METRIC_L2, P, M, D, h, stream);
}
extern "C" int lds_knn_prepare_metric(const float* P, int64_t M, int D, int metric, float* h, void* stream) {
    return kn_prepare("lds_knn_prepare_metric", metric, P, M, D, h, stream);
}

extern "C" int lds_knn_workspace_bytes(int64_t N, int64_t M, int D, int k, size_t* out) {
    if (!out) return set_error(LDS_EINVAL, "lds_knn_workspace_bytes: null out");
    if (int rc = kn_check_dims("lds_knn_workspace_bytes", N, M, D, k)) return rc;
    *out = kn_plan(N, M, D, k, 0, 0).bytes;
    return LDS_OK;
}

extern "C" int lds_knn_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int32_t* idx, float* score, void* ws,
                              size_t ws_bytes, void* stream) {
    return kn_search("lds_knn_search", LDS_METRIC_L2, X, N, P, h, M, D, k, 0, 0, idx, score, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int lds_knn_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int metric, int32_t* idx, float* score,
                                     void* ws, size_t ws_bytes, void* stream) {
    return kn_search("lds_knn_search_metric", metric, X, N, P, h, M, D, k, 0, 0, idx, score, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int lds_knn_retrieve(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, float ratio, float* Y, int32_t* idx,
                                float* dist, void* ws, size_t ws_bytes, void* stream) {
    return kn_retrieve("lds_knn_retrieve", LDS_METRIC_L2, LDS_WEIGHTS_INVERSE_SQUARE, X, N, P, h, M, D, k, ratio, Y, idx, dist, ws, ws_bytes, kn_plain(),
                       (hipStream_t)stream);
}
extern "C" int lds_knn_retrieve_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int metric, int weights, float ratio,
                                       float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream) {
    return kn_retrieve("lds_knn_retrieve_metric", metric, weights, X, N, P, h, M, D, k, ratio, Y, idx, dist, ws, ws_bytes, kn_plain(), (hipStream_t)stream);
}

extern "C" int lds_knn_retrieve_ragged(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                                       float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream) {
    lds::KnLens lens;
    if (int rc = kn_ragged_lens("lds_knn_retrieve_ragged", B, T, lengths, lens)) return rc;
    return kn_retrieve("lds_knn_retrieve_ragged", LDS_METRIC_L2, LDS_WEIGHTS_INVERSE_SQUARE, X, (long long)B * T, P, h, M, D, k, ratio, Y, idx, dist, ws, ws_bytes,
                       lens, (hipStream_t)stream);
}
extern "C" int lds_knn_retrieve_ragged_metric(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                                              int metric, int weights, float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes,
                                              void* stream) {
    lds::KnLens lens;
    if (int rc = kn_ragged_lens("lds_knn_retrieve_ragged_metric", B, T, lengths, lens)) return rc;
    return kn_retrieve("lds_knn_retrieve_ragged_metric", metric, weights, X, (long long)B * T, P, h, M, D, k, ratio, Y, idx, dist, ws, ws_bytes, lens,
                       (hipStream_t)stream);
}

namespace {
int kn_test_search(const char* fn, int metric, const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int slab_rows, int splits,
                   int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream) {
    if (slab_rows < lds::kKnB || slab_rows % lds::kKnB || (D >= 8 && D <= 4096 && slab_rows > kn_slab_rows(D)))
        return set_error(LDS_EINVAL, "%s: slab_rows %d must be a multiple of 128 that one descriptor holds", fn, slab_rows);
    if (splits < 1 || splits > kKnMaxSplits) return set_error(LDS_EINVAL, "%s: splits %d outside 1 .. %d", fn, splits, kKnMaxSplits);
    return kn_search(fn, metric, X, N, P, h, M, D, k, slab_rows, splits, idx, score, ws, ws_bytes, (hipStream_t)stream);
}
}  // namespace

extern "C" int lds_test_knn_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int slab_rows, int splits, int32_t* idx,
                                   float* score, void* ws, size_t ws_bytes, void* stream) {
    return kn_test_search("lds_test_knn_search", LDS_METRIC_L2, X, N, P, h, M, D, k, slab_rows, splits, idx, score, ws, ws_bytes, stream);
}
extern "C" int lds_test_knn_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int metric, int slab_rows, int splits,
                                          int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream) {
    return kn_test_search("lds_test_knn_search_metric", metric, X, N, P, h, M, D, k, slab_rows, splits, idx, score, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// IVF coarse index (faiss IndexIVFFlat's role in the RVC / Diffusion-SVC tool chains): probe nprobe lists, not the pool.
//   index    coarse centres C [nlist][D]; pool row m belongs to the list of its best centre; offsets [nlist + 1] / order [M] give every
//            list's rows in ascending original index; PL [Mp][D] is the pool in list order with every list padded to whole 128-row blocks
//            (list l starts at block sum_{j < l} ceil(len_j / 128)), hl its h in the same order.  A block belongs to one list and, as the
//            slabs are cut at whole blocks, to one slab.
//   coarse   the exact search above over the centres with k = nprobe, unchanged: probe [N][nprobe].
//   buckets  the N x nprobe (query, list) pairs grouped by list: count (integer atomics), one scan, fill (integer atomics).  The slot a
//            pair lands in decides which tile column scores it, and a column's scores do not depend on the column: no result depends on it.
//   scan     knn_topk_kernel's tile with the query operand GATHERED -- tile row i is the X row that bucket entry i names, by the per-lane
//            source address of the LDS-DMA -- over the pool blocks of one list.  A workgroup takes one list and up to 128 of its bucket's
//            queries; a list of more than kIvfSegBlocks blocks is cut into up to kIvfSegs block ranges ("segments"), each walked by workgroups
//            of its own, so that the longest list is not one workgroup's serial walk.  List rows are numbered 0 .. len - 1 inside the kernel (ascending original index, so the insertion rule keeps the
//            lower original index first) and translated through `order` on the way out: the lists go to the workspace as
//            [probe slot * kIvfSegs + segment][N][KT] (empty where a list has fewer segments), the layout kn_merge reads with
//            S = nprobe * kIvfSegs, and knn_select_kernel / knn_blend_kernel run as they are.
// No floating-point atomics; every slot of the workspace that is read was written by the same call.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace lds {

constexpr int kIvfSegs = 8;          // the most block ranges a list is cut into
constexpr int kIvfSegBlocks = 4;     // the fewest 128-row blocks in a range (but the last)

// the blocks per segment of a list of nblk blocks, and its segments (1 for an empty list: its workgroups still write empty result lists)
static __host__ __device__ __forceinline__ int ivf_seg_blocks(int nblk) {
    const int per = (nblk + kIvfSegs - 1) / kIvfSegs;
    return per > kIvfSegBlocks ? per : kIvfSegBlocks;
}
static __host__ __device__ __forceinline__ int ivf_segs(int nblk) {
    const int n = (nblk + ivf_seg_blocks(nblk) - 1) / ivf_seg_blocks(nblk);
    return n > 0 ? n : 1;
}

// one thread per (query, probe slot) pair: the list's count, or -- a slot without a list (a NaN query) -- the pair's empty result list
__global__ void __launch_bounds__(256) ivf_count_kernel(const int* __restrict__ probe, long long pairs, long long N, int nprobe, int nlist, int KT,
                                                        int* __restrict__ cnt, float* __restrict__ lval, int* __restrict__ lidx) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pairs) return;
    const int l = probe[t];
    if (l >= 0 && l < nlist) {
        atomicAdd(&cnt[l], 1);
        return;
    }
    for (int g = 0; g < kIvfSegs; ++g) {
        const long long o = (((t % nprobe) * kIvfSegs + g) * N + t / nprobe) * KT;
        for (int p = 0; p < KT; ++p) { lval[o + p] = -INFINITY; lidx[o + p] = kKnNone; }
    }
}

// One workgroup.  Checks the offsets table (starts at 0, never decreases, ends at M, and its lists padded to whole blocks fill exactly the
// Mp rows of the copy); a table that fails gives every list the length 0, so that every query comes back without neighbours and no address
// is formed from it.  Then three exclusive scans over the lists: pool blocks (lblk), bucket entries (bstart), workgroups of the scan (wstart:
// one per 128 entries of a bucket and segment of the list); cnt is zeroed again to serve the fill as cursors.
__global__ void __launch_bounds__(1024) ivf_plan_kernel(const long long* __restrict__ offsets, int nlist, long long M, long long Mp, int* __restrict__ cnt,
                                                        int* __restrict__ llen, int* __restrict__ lrow, int* __restrict__ lblk,
                                                        long long* __restrict__ bstart, int* __restrict__ wstart) {
    __shared__ long long sa[1024], sb[1024], sc[1024];      // per thread: pool blocks, bucket entries, workgroups of its lists
    __shared__ int bad;
    const int t = threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    const int l0 = t * per < nlist ? t * per : nlist, l1 = l0 + per < nlist ? l0 + per : nlist;
    if (t == 0) bad = (offsets[0] != 0 || offsets[nlist] != M) ? 1 : 0;
    __syncthreads();
    long long a = 0, b = 0;
    bool mybad = false;
    for (int l = l0; l < l1; ++l) {
        const long long o0 = offsets[l], o1 = offsets[l + 1];
        if (o0 < 0 || o1 < o0 || o1 > M) mybad = true;
        const long long len = mybad ? 0 : o1 - o0;
        a += (len + kKnB - 1) / kKnB;
        b += cnt[l];
    }
    if (mybad) bad = 1;
    sa[t] = a; sb[t] = b;
    __syncthreads();
    if (t == 0) {
        long long ra = 0, rb = 0;
        for (int i = 0; i < 1024; ++i) {
            const long long va = sa[i], vb = sb[i];
            sa[i] = ra; sb[i] = rb;
            ra += va; rb += vb;
        }
        if (ra * kKnB != Mp) bad = 1;
        bstart[nlist] = rb;
    }
    __syncthreads();
    const bool ok = bad == 0;      // known to all: the workgroups of a list depend on its length as it will be used
    long long c = 0;
    for (int l = l0; l < l1; ++l) {
        const long long len = ok ? offsets[l + 1] - offsets[l] : 0;
        c += (long long)((cnt[l] + kKnB - 1) / kKnB) * ivf_segs((int)((len + kKnB - 1) / kKnB));
    }
    sc[t] = c;
    __syncthreads();
    if (t == 0) {
        long long rc = 0;
        for (int i = 0; i < 1024; ++i) {
            const long long vc = sc[i];
            sc[i] = rc;
            rc += vc;
        }
        wstart[nlist] = (int)rc;
    }
    __syncthreads();
    a = sa[t]; b = sb[t]; c = sc[t];
    for (int l = l0; l < l1; ++l) {
        const long long o0 = offsets[l], o1 = offsets[l + 1];
        const long long len = ok ? o1 - o0 : 0;
        const int n = cnt[l];
        llen[l] = (int)len;
        lrow[l] = ok ? (int)o0 : 0;
        lblk[l] = ok ? (int)a : 0;
        bstart[l] = b;
        wstart[l] = (int)c;
        cnt[l] = 0;
        a += (len + kKnB - 1) / kKnB;
        b += n;
        c += (long long)((n + kKnB - 1) / kKnB) * ivf_segs((int)((len + kKnB - 1) / kKnB));
    }
}

// one thread per pair again: the pair takes the next slot of its list's bucket (which one does not matter to any result)
__global__ void __launch_bounds__(256) ivf_fill_kernel(const int* __restrict__ probe, long long pairs, int nprobe, int nlist,
                                                       const long long* __restrict__ bstart, int* __restrict__ cursor, long long* __restrict__ bq) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pairs) return;
    const int l = probe[t];
    if (l < 0 || l >= nlist) return;
    const int slot = atomicAdd(&cursor[l], 1);
    bq[bstart[l] + slot] = (t / nprobe) * 8 + t % nprobe;      // query * 8 + probe slot
}

// knn_topk_kernel's tile, waves, LDS image, swizzle, MFMA order and lists; workgroup w takes entries chunk * 128 .. + 128 of list l's bucket
// and segment seg of the list (wstart[l] <= w < wstart[l + 1], w - wstart[l] = chunk * segments + seg) and walks that segment's pool blocks in
// PL; the workgroup of segment 0 also writes the empty lists of the segments the list does not have.  The X descriptor spans all of X
// (N D 4 <= kKnOob bytes, checked by the driver) and a lane's offset is its bucket entry's row: the gather.  Tile columns beyond the bucket
// repeat its last entry and are not stored; tile rows beyond the list's length score -inf and never enter a list.  MET as in knn_topk_kernel.
template <int KT, int MET>
__global__ void __launch_bounds__(256) ivf_scan_kernel(const float* __restrict__ X, long long N, const float* __restrict__ PL, const float* __restrict__ hl,
                                                       int Mp, int D, int slab_blocks, const int* __restrict__ order, int M,
                                                       const int* __restrict__ llen, const int* __restrict__ lrow, const int* __restrict__ lblk,
                                                       const long long* __restrict__ bstart, const int* __restrict__ wstart, int nlist,
                                                       const long long* __restrict__ bq, float* __restrict__ lval, int* __restrict__ lidx) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kKnTile];      // 2 stages x (X tile, P tile) = 64 KB
    const int w = blockIdx.x;
    if (w >= wstart[nlist]) return;                                        // (the grid is the host's upper bound)
    int l = 0;
    for (int hi = nlist; l < hi;) {                                        // the first list whose workgroups end beyond w
        const int mid = (l + hi) >> 1;
        if (wstart[mid + 1] > w) hi = mid; else l = mid + 1;
    }
    const int len = llen[l], row0 = lrow[l];
    const int nblk = (len + kKnB - 1) / kKnB, nseg = ivf_segs(nblk), segb = ivf_seg_blocks(nblk);
    const int seg = (w - wstart[l]) % nseg;
    const long long qbase = bstart[l] + (long long)((w - wstart[l]) / nseg) * kKnB;
    const long long qleft = bstart[l + 1] - qbase;
    const int cols = (int)(qleft < kKnB ? qleft : kKnB);                   // >= 1
    const int lb0 = lblk[l];                                                // the list's first block: rows are numbered from it
    const int pb0 = lb0 + seg * segb, pb1 = lb0 + ((seg + 1) * segb < nblk ? (seg + 1) * segb : nblk);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int nk = (D + kKnBK - 1) / kKnBK;
    const int slab_rows = slab_blocks * kKnB;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X), 0, (int)(N * D * 4), 0x00020000);
    int xoff[4], crow[4], kch[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        crow[i] = row;
        kch[i] = ch * 4;
        const long long q = bq[qbase + (row < cols ? row : cols - 1)] >> 3;      // columns beyond the bucket read its last query (not stored)
        xoff[i] = (int)(q * D * 4) + ch * 16;
    }
    auto issue = [&](int pb, int ks, float* st) {
        const int k0 = ks * kKnBK;
        const bool tail = k0 + kKnBK > D;
        const int slab = pb / slab_blocks;                                     // wave-uniform: the descriptor lives in scalar registers
        const int r0 = slab * slab_rows;
        const int srows = Mp - r0 < slab_rows ? Mp - r0 : slab_rows;
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(PL + (long long)r0 * D), 0, srows * D * 4, 0x00020000);
        const int b0 = pb * kKnB - r0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int pr = b0 + crow[i];
            pr = pr < srows ? pr : srows - 1;
            int vx = xoff[i], vp = pr * D * 4 + kch[i] * 4;
            if (tail && k0 + kch[i] >= D) vx = vp = kKnOob;                     // d beyond D: zeros for both operands
            float* dst = st + (wave * 4 + i) * 256;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)dst, 16, vx, k0 * 4, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rp, (__attribute__((address_space(3))) void*)(dst + kKnTile), 16, vp, k0 * 4, 0, 0);
        }
    };
    int pos[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) pos[g] = ((2 * g + h) ^ ((c >> 1) & 7)) * 4;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float lv[2][KT];
    int li[2][KT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < KT; ++p) { lv[j][p] = -INFINITY; li[j][p] = kKnNone; }

    const int total = (pb1 - pb0) * nk;
    int pb = pb0, ks = 0;           // the tile being computed
    int ipb = pb0, iks = 0;         // the tile being fetched
    if (total > 0) issue(ipb, iks, smem);
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();            // tile s has landed for everyone; everyone has finished reading tile s - 1
        if (s + 1 < total) {
            if (++iks == nk) { iks = 0; ++ipb; }
            issue(ipb, iks, smem + ((s + 1) & 1) * 2 * kKnTile);
        }
        const float* xs = smem + (s & 1) * 2 * kKnTile + (wn * 64 + c) * kKnBK;
        const float* ps = smem + (s & 1) * 2 * kKnTile + kKnTile + (wm * 64 + c) * kKnBK;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const f32x4*>(ps + i * 32 * kKnBK + pos[g]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f32x4*>(xs + j * 32 * kKnBK + pos[g]);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][jj], b[j][jj], acc[i][j], 0, 0, 0);
        }
        if (++ks == nk) {           // a pool block is complete: scores into the lists, in increasing row of the list
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int t = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;      // the row inside the block
                    const int m = (pb - lb0) * kKnB + t;                                   // the row inside the list
                    const float hv = m < len ? hl[(long long)pb * kKnB + t] : (MET == LDS_METRIC_COSINE ? 0.f : INFINITY);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        float v;
                        if constexpr (MET == LDS_METRIC_COSINE) v = m < len ? acc[i][j][r] * hv : -INFINITY;
                        else v = acc[i][j][r] - hv;
                        acc[i][j][r] = 0.f;
                        if (v > lv[j][KT - 1]) {      // (a NaN score, or -inf beyond the list, never enters)
#pragma unroll
                            for (int p = KT - 1; p >= 0; --p) {
                                const bool up = p > 0 && v > lv[j][p > 0 ? p - 1 : 0];
                                const bool here = v > lv[j][p];
                                lv[j][p] = up ? lv[j][p > 0 ? p - 1 : 0] : (here ? v : lv[j][p]);
                                li[j][p] = up ? li[j][p > 0 ? p - 1 : 0] : (here ? m : li[j][p]);
                            }
                        }
                    }
                }
            ks = 0;
            ++pb;
        }
    }
    __syncthreads();
    // the four lists of a query (two wm waves x two half-waves) meet in LDS: [list q][entry p][query], 4 * KT * 128 values and as many indices
    float* rv = smem;
    int* ri = reinterpret_cast<int*>(smem + 4 * KT * kKnB);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < KT; ++p) {
            rv[((wm * 2 + h) * KT + p) * kKnB + wn * 64 + j * 32 + c] = lv[j][p];
            ri[((wm * 2 + h) * KT + p) * kKnB + wn * 64 + j * 32 + c] = li[j][p];
        }
    __syncthreads();
    if (tid < cols) {
        int at[4] = {0, 0, 0, 0};
        const long long pair = bq[qbase + tid];
        const long long o = (((pair & 7) * kIvfSegs + seg) * N + (pair >> 3)) * KT;
        if (seg == 0)
            for (int g = nseg; g < kIvfSegs; ++g) {
                const long long e = (((pair & 7) * kIvfSegs + g) * N + (pair >> 3)) * KT;
                for (int p = 0; p < KT; ++p) { lval[e + p] = -INFINITY; lidx[e + p] = kKnNone; }
            }
        for (int p = 0; p < KT; ++p) {
            float bv = -INFINITY;
            int bi = kKnNone, bq_ = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int a = at[q] < KT ? at[q] : KT - 1;
                const float v = at[q] < KT ? rv[(q * KT + a) * kKnB + tid] : -INFINITY;
                const int i = at[q] < KT ? ri[(q * KT + a) * kKnB + tid] : kKnNone;
                if (kn_before(v, i, bv, bi)) { bv = v; bi = i; bq_ = q; }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) at[q] += (q == bq_ && bi != kKnNone) ? 1 : 0;
            int oi = kKnNone;
            if (bi != kKnNone) {      // the list's row -> the original pool index; both clamped before they are used
                const int at_ = row0 + bi;
                oi = order[at_ < M ? at_ : M - 1];
                oi = oi < 0 ? 0 : (oi < M ? oi : M - 1);
            }
            lval[o + p] = bv;
            lidx[o + p] = oi;
        }
    }
}

}  // namespace lds

namespace {

constexpr int kIvfMaxLists = 65536;

struct IvfPlan {
    KnPlan coarse;              // the exact search over the centres, k = nprobe
    int KT, slab_blocks;
    long long pairs;
    unsigned wmax;              // an upper bound of the scan's workgroups: one per 128 bucket entries (rounded up per list) and segment
    size_t o_probe, o_cnt, o_llen, o_lrow, o_lblk, o_bstart, o_wstart, o_bq, o_val, o_idx, bytes;
};

int ivf_check_dims(const char* fn, long long N, long long M, int D, int k, int nlist, int nprobe) {
    if (int rc = kn_check_dims(fn, N, M, D, k)) return rc;
    if (nlist < 1 || nlist > kIvfMaxLists || nlist > M) return set_error(LDS_EINVAL, "%s: nlist %d outside 1 .. min(65536, M = %lld)", fn, nlist, M);
    if (nprobe < 1 || nprobe > lds::kKnMaxK || nprobe > nlist) return set_error(LDS_EINVAL, "%s: nprobe %d outside 1 .. min(8, nlist = %d)", fn, nprobe, nlist);
    if (N * D * 4 > (long long)lds::kKnOob)
        return set_error(LDS_EINVAL, "%s: N %lld rows of D %d exceed the %d bytes one descriptor of the gathered query operand holds", fn, N, D, lds::kKnOob);
    return LDS_OK;
}

IvfPlan ivf_plan(long long N, int D, int k, int nlist, int nprobe, int slab_rows) {
    IvfPlan p;
    p.coarse = kn_plan(N, nlist, D, nprobe, 0, 0);
    p.KT = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8;
    p.slab_blocks = (slab_rows > 0 ? slab_rows : kn_slab_rows(D)) / lds::kKnB;
    p.pairs = N * nprobe;
    const long long full = p.pairs / lds::kKnB + nlist;
    p.wmax = (unsigned)((full < p.pairs ? full : p.pairs) * lds::kIvfSegs);
    Slots S{Slots::round(p.coarse.bytes)};
    p.o_probe = S.take((size_t)p.pairs * 4);
    p.o_cnt = S.take((size_t)nlist * 4);
    p.o_llen = S.take((size_t)nlist * 4);
    p.o_lrow = S.take((size_t)nlist * 4);
    p.o_lblk = S.take((size_t)nlist * 4);
    p.o_bstart = S.take(((size_t)nlist + 1) * 8);
    p.o_wstart = S.take(((size_t)nlist + 1) * 4);
    p.o_bq = S.take((size_t)p.pairs * 8);
    p.o_val = S.take((size_t)nprobe * lds::kIvfSegs * (size_t)N * p.KT * 4);
    p.o_idx = S.take((size_t)nprobe * lds::kIvfSegs * (size_t)N * p.KT * 4);
    p.bytes = S.o;
    return p;
}

struct IvfIndex {               // the arguments every lds_ivf_* entry adds
    const float *C, *hc;
    int nlist;
    const int64_t* offsets;
    const int32_t* order;
    const float *PL, *hl;
    long long Mp;
    int nprobe;
    int metric;                 // LDS_METRIC_*: hc / hl (and the original pool's h, for the blend) hold h or r accordingly
};

int ivf_check_index(const char* fn, const IvfIndex& ix, long long M) {
    if (!ix.C || !ix.hc || !ix.offsets || !ix.order || !ix.PL || !ix.hl) return set_error(LDS_EINVAL, "%s: null pointer in the index", fn);
    if (kn_misaligned(ix.C) || kn_misaligned(ix.PL)) return set_error(LDS_EINVAL, "%s: the centres and the list-ordered copy must be 16-byte aligned", fn);
    if (ix.Mp < M || ix.Mp % lds::kKnB || ix.Mp > M + (long long)(lds::kKnB - 1) * ix.nlist)
        return set_error(LDS_EINVAL, "%s: copy_rows %lld must be a multiple of 128 in M .. M + 127 nlist (M %lld, nlist %d)", fn, ix.Mp, M, ix.nlist);
    return LDS_OK;
}

// coarse search, buckets and the list scan: the per-(query, probe slot, segment) lists [nprobe * kIvfSegs][N][KT] are in the workspace afterwards
void ivf_lists(const IvfPlan& p, const float* X, long long N, long long M, int D, const IvfIndex& ix, void* ws, hipStream_t s) {
    char* w = (char*)ws;
    int* probe = (int*)(w + p.o_probe);
    int* cnt = (int*)(w + p.o_cnt);
    int *llen = (int*)(w + p.o_llen), *lrow = (int*)(w + p.o_lrow), *lblk = (int*)(w + p.o_lblk), *wstart = (int*)(w + p.o_wstart);
    long long *bstart = (long long*)(w + p.o_bstart), *bq = (long long*)(w + p.o_bq);
    float* lval = (float*)(w + p.o_val);
    int* lidx = (int*)(w + p.o_idx);
    {
        float* cval = (float*)(w + p.coarse.o_val);
        int* cidx = (int*)(w + p.coarse.o_idx);
        kn_topk(p.coarse, ix.metric, X, N, ix.C, ix.hc, ix.nlist, D, cval, cidx, s);
        hipLaunchKernelGGL(lds::knn_select_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, cval, cidx, p.coarse.S, p.coarse.KT, N, ix.nlist, ix.nprobe,
                           probe, (float*)nullptr);
    }
    const dim3 pg((unsigned)((p.pairs + 255) / 256));
    (void)hipMemsetAsync(cnt, 0, (size_t)ix.nlist * 4, s);
    hipLaunchKernelGGL(lds::ivf_count_kernel, pg, dim3(256), 0, s, probe, p.pairs, N, ix.nprobe, ix.nlist, p.KT, cnt, lval, lidx);
    hipLaunchKernelGGL(lds::ivf_plan_kernel, dim3(1), dim3(1024), 0, s, (const long long*)ix.offsets, ix.nlist, M, ix.Mp, cnt, llen, lrow, lblk, bstart, wstart);
    hipLaunchKernelGGL(lds::ivf_fill_kernel, pg, dim3(256), 0, s, probe, p.pairs, ix.nprobe, ix.nlist, bstart, cnt, bq);
    lds::ProfScope ps(s, "ivf_scan", 2.0 * (double)N * ix.nprobe * ((double)M / ix.nlist) * D, 4.0 * ((double)N * ix.nprobe * D + (double)ix.Mp * D));
#define LDS_IVF_SCAN_ARGS dim3(p.wmax), dim3(256), 0, s, X, N, ix.PL, ix.hl, (int)ix.Mp, D, p.slab_blocks, (const int*)ix.order, (int)M, llen, lrow, lblk, bstart, wstart, ix.nlist, bq, lval, lidx
#define LDS_IVF_SCAN(KT_)                                                                                                 \
    if (ix.metric == LDS_METRIC_COSINE) hipLaunchKernelGGL((lds::ivf_scan_kernel<KT_, LDS_METRIC_COSINE>), LDS_IVF_SCAN_ARGS); \
    else hipLaunchKernelGGL((lds::ivf_scan_kernel<KT_, LDS_METRIC_L2>), LDS_IVF_SCAN_ARGS)
    switch (p.KT) {
        case 1: LDS_IVF_SCAN(1); break;
        case 2: LDS_IVF_SCAN(2); break;
        case 4: LDS_IVF_SCAN(4); break;
        default: LDS_IVF_SCAN(8); break;
    }
#undef LDS_IVF_SCAN
#undef LDS_IVF_SCAN_ARGS
}

int ivf_search(const char* fn, const float* X, long long N, long long M, int D, int k, const IvfIndex& ix, int slab_rows, int32_t* idx, float* score, void* ws,
               size_t ws_bytes, hipStream_t s) {
    if (int rc = kn_check_metric(fn, ix.metric, LDS_WEIGHTS_INVERSE_SQUARE)) return rc;
    if (int rc = ivf_check_dims(fn, N, M, D, k, ix.nlist, ix.nprobe)) return rc;
    if (!X || !idx || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    if (int rc = ivf_check_index(fn, ix, M)) return rc;
    if (kn_misaligned(X)) return set_error(LDS_EINVAL, "%s: X must be 16-byte aligned", fn);
    const IvfPlan p = ivf_plan(N, D, k, ix.nlist, ix.nprobe, slab_rows);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    ivf_lists(p, X, N, M, D, ix, ws, s);
    kn_select(ix.metric, X, D, (const float*)((char*)ws + p.o_val), (const int*)((char*)ws + p.o_idx), ix.nprobe * lds::kIvfSegs, p.KT, N, (int)M, k, idx, score, s);
    return launched(fn);
}

int ivf_retrieve(const char* fn, int weights, const float* X, long long N, const float* P, const float* h, long long M, int D, int k, const IvfIndex& ix, float ratio,
                 float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, const lds::KnLens& lens, hipStream_t s) {
    if (int rc = kn_check_metric(fn, ix.metric, weights)) return rc;
    if (int rc = ivf_check_dims(fn, N, M, D, k, ix.nlist, ix.nprobe)) return rc;
    if (ix.metric == LDS_METRIC_COSINE && !h) return set_error(LDS_EINVAL, "%s: null h (the cosine blend reads the pool's row constants)", fn);
    if (!(ratio >= 0.f && ratio <= 1.f)) return set_error(LDS_EINVAL, "%s: ratio %g outside 0 .. 1", fn, (double)ratio);
    if (!X || !P || !Y || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    if (int rc = ivf_check_index(fn, ix, M)) return rc;
    if (kn_misaligned(X) || kn_misaligned(P) || kn_misaligned(Y)) return set_error(LDS_EINVAL, "%s: X, P and Y must be 16-byte aligned", fn);
    const IvfPlan p = ivf_plan(N, D, k, ix.nlist, ix.nprobe, 0);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    ivf_lists(p, X, N, M, D, ix, ws, s);
    kn_blend(ix.metric, weights, X, N, P, h, (int)M, D, (const float*)((char*)ws + p.o_val), (const int*)((char*)ws + p.o_idx), ix.nprobe * lds::kIvfSegs, p.KT, k,
             ratio, Y, idx, dist, lens, s);
    return launched(fn);
}

}  // namespace

extern "C" int lds_ivf_workspace_bytes(int64_t N, int64_t M, int D, int k, int nlist, int nprobe, size_t* out) {
    if (!out) return set_error(LDS_EINVAL, "lds_ivf_workspace_bytes: null out");
    if (int rc = ivf_check_dims("lds_ivf_workspace_bytes", N, M, D, k, nlist, nprobe)) return rc;
    *out = ivf_plan(N, D, k, nlist, nprobe, 0).bytes;
    return LDS_OK;
}

#define LDS_IVF_INDEX_PARAMS const float* C, const float* hc, int nlist, const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe

extern "C" int lds_ivf_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, int32_t* idx,
                              float* score, void* ws, size_t ws_bytes, void* stream) {
    (void)P; (void)h;      // the search scores the list-ordered copy
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, LDS_METRIC_L2};
    return ivf_search("lds_ivf_search", X, N, M, D, k, ix, 0, idx, score, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int lds_ivf_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, int metric,
                                     int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream) {
    (void)P; (void)h;
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, metric};
    return ivf_search("lds_ivf_search_metric", X, N, M, D, k, ix, 0, idx, score, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int lds_ivf_retrieve(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, float ratio,
                                float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream) {
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, LDS_METRIC_L2};
    return ivf_retrieve("lds_ivf_retrieve", LDS_WEIGHTS_INVERSE_SQUARE, X, N, P, h, M, D, k, ix, ratio, Y, idx, dist, ws, ws_bytes, kn_plain(), (hipStream_t)stream);
}
extern "C" int lds_ivf_retrieve_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, int metric,
                                       int weights, float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream) {
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, metric};
    return ivf_retrieve("lds_ivf_retrieve_metric", weights, X, N, P, h, M, D, k, ix, ratio, Y, idx, dist, ws, ws_bytes, kn_plain(), (hipStream_t)stream);
}

extern "C" int lds_ivf_retrieve_ragged(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                                       LDS_IVF_INDEX_PARAMS, float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream) {
    lds::KnLens lens;
    if (int rc = kn_ragged_lens("lds_ivf_retrieve_ragged", B, T, lengths, lens)) return rc;
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, LDS_METRIC_L2};
    return ivf_retrieve("lds_ivf_retrieve_ragged", LDS_WEIGHTS_INVERSE_SQUARE, X, (long long)B * T, P, h, M, D, k, ix, ratio, Y, idx, dist, ws, ws_bytes, lens,
                        (hipStream_t)stream);
}
extern "C" int lds_ivf_retrieve_ragged_metric(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                                              LDS_IVF_INDEX_PARAMS, int metric, int weights, float ratio, float* Y, int32_t* idx, float* dist, void* ws,
                                              size_t ws_bytes, void* stream) {
    lds::KnLens lens;
    if (int rc = kn_ragged_lens("lds_ivf_retrieve_ragged_metric", B, T, lengths, lens)) return rc;
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, metric};
    return ivf_retrieve("lds_ivf_retrieve_ragged_metric", weights, X, (long long)B * T, P, h, M, D, k, ix, ratio, Y, idx, dist, ws, ws_bytes, lens,
                        (hipStream_t)stream);
}

namespace {
int ivf_test_search(const char* fn, int metric, const float* X, int64_t N, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, int slab_rows, int32_t* idx, float* score,
                    void* ws, size_t ws_bytes, void* stream) {
    if (slab_rows < lds::kKnB || slab_rows % lds::kKnB || (D >= 8 && D <= 4096 && slab_rows > kn_slab_rows(D)))
        return set_error(LDS_EINVAL, "%s: slab_rows %d must be a multiple of 128 that one descriptor holds", fn, slab_rows);
    const IvfIndex ix = {C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, metric};
    return ivf_search(fn, X, N, M, D, k, ix, slab_rows, idx, score, ws, ws_bytes, (hipStream_t)stream);
}
}  // namespace

extern "C" int lds_test_ivf_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, int slab_rows,
                                   int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream) {
    (void)P; (void)h;
    return ivf_test_search("lds_test_ivf_search", LDS_METRIC_L2, X, N, M, D, k, C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, slab_rows, idx, score, ws,
                           ws_bytes, stream);
}
extern "C" int lds_test_ivf_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, LDS_IVF_INDEX_PARAMS, int metric,
                                          int slab_rows, int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream) {
    (void)P; (void)h;
    return ivf_test_search("lds_test_ivf_search_metric", metric, X, N, M, D, k, C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe, slab_rows, idx, score, ws,
                           ws_bytes, stream);
}
#undef LDS_IVF_INDEX_PARAMS
