// K-means semantic tokenizer (reference cluster/kmeans.py KMeansGPU + _kpp, cluster/__init__.py get_cluster_result): units -> tokens and
// the codebook fit, exact fp32, gfx950.
//   assign   label[n] = argmax_k (x_n . c_k - h_k), h_k = |c_k|^2 / 2 (= argmin of the squared distance = argmax of the reference's
//            euc_sim), lowest index among equal scores.  The dot products run on v_mfma_f32_32x32x2_f32 with both operand tiles moved
//            HBM/L2 -> LDS by LDS-DMA.  X [N][D] and C [K][D] are plain row-major: a lane's 16-byte LDS read is four consecutive d of
//            one row, used as the operands of four MFMAs, i.e. the d index inside a dot product is permuted -- the same way for both
//            operands and for every (n, k), so every score of a row is the same fmaf chain and duplicated centres tie exactly.  The
//            N x K matrix is never stored: the (value, index) maximum lives in registers across the centre blocks a workgroup walks.
//   update   one Lloyd step in the reference's form (kmeans.py:184-198): stable counting sort of the row indices by label (integer
//            atomics only for the per-row-block histograms), one workgroup per (cluster, 256 columns) summing its rows in index
//            order, error by a fixed-order reduction.  No floating-point atomics: every result is independent of scheduling.
//   cosine   (KMeansGPU mode='cosine', kmeans.py:96-105 cos_sim) the same tile with another epilogue: score = (x_n . c_k) r_k, r_k = 1 / max(|c_k|,
//            1e-12) in the per-centre array that holds h_k otherwise; `best` is multiplied by r(x_n) after the arg-max is decided.
//   seed     k-means++ (_kpp, kmeans.py:10-50) with a running minimum distance and a double-precision prefix; the picks stay on the device.
#include "../../include/lds.h"
#include "kernels.h"
#include "host.h"

#include <math.h>

namespace lds {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kKmB = 128;                  // rows of X / centres per tile
constexpr int kKmBK = 32;                  // d per K-step: one 128-byte line of every row
constexpr int kKmTile = kKmB * kKmBK;      // floats per operand tile
constexpr int kKmOob = 0x7fff0000;         // a buffer offset beyond every slab: the DMA stores zeros

struct KmLens { int n, T, pad; int v[64]; };      // ragged form: B = n clips of T rows, v[b] valid rows, `pad` written beyond; n = 0: plain

// the cosine row constant of a row whose fp32 sum of squares is s: 1 / max(sqrt(s), 1e-12), both operations correctly rounded
// (F.normalize's eps; s = 4, 16, 64 give exactly 1/2, 1/4, 1/8; a zero row gets 1e12 and scores 0 against everything)
static __device__ __forceinline__ float km_row_const(float s) { return __frcp_rn(fmaxf(__fsqrt_rn(s), 1e-12f)); }

// (value, index) maximum with the lowest index among equal values: associative and commutative, so any combination order agrees
static __device__ __forceinline__ void km_take(float v, int i, float& bv, int& bi) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// 256 threads = 2 x 2 waves; wave (wm, wn) owns centres wm*64 .. +64 (MFMA rows, spread over the accumulator registers) and points
// wn*64 .. +64 (MFMA columns, one per lane) of a 128 x 128 tile.  grid (row blocks, centre splits).
// LDS image of a tile: row r is 128 bytes = 8 chunks of 16; chunk q sits at position q ^ ((r >> 1) & 7), which makes the ds_read_b128 of
// 32 consecutive rows at one chunk conflict-free.  LDS-DMA stores lane-linearly, so the swizzle is applied to the SOURCE address: one
// wave instruction fetches 8 whole lines (8 rows x 128 bytes).  MET (LDS_METRIC_*) selects the epilogue only: acc - h_k, or acc * r_k.
template <int MET>
__global__ void __launch_bounds__(256) kmeans_assign_kernel(const float* __restrict__ X, long long N, const float* __restrict__ Cc, const float* __restrict__ hh, int K,
                                                            int D, int cb_per_split, long long* __restrict__ labels, float* __restrict__ best_out,
                                                            float* __restrict__ pval, int* __restrict__ pidx, const KmLens lens) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kKmTile];      // 2 stages x (X tile, C tile) = 64 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const long long n0 = (long long)blockIdx.x * kKmB;
    const int rows = (int)((N - n0) < kKmB ? (N - n0) : kKmB);
    const int nCB = (K + kKmB - 1) / kKmB;
    const int cb0 = blockIdx.y * cb_per_split;
    const int cb1 = cb0 + cb_per_split < nCB ? cb0 + cb_per_split : nCB;
    const int nk = (D + kKmBK - 1) / kKmBK;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X + n0 * D), 0, rows * D * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Cc), 0, K * D * 4, 0x00020000);
    int xoff[4], crow[4], kch[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        crow[i] = row;
        kch[i] = ch * 4;
        xoff[i] = (row < rows ? row : rows - 1) * D * 4 + ch * 16;      // rows beyond N read the last row (their labels are not stored)
    }
    auto issue = [&](int cb, int ks, float* st) {
        const int k0 = ks * kKmBK;
        const bool tail = k0 + kKmBK > D;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int kr = cb * kKmB + crow[i];
            kr = kr < K ? kr : K - 1;                                   // centres beyond K read the last one (masked in the epilogue)
            int vx = xoff[i], vc = kr * D * 4 + kch[i] * 4;
            if (tail && k0 + kch[i] >= D) vx = vc = kKmOob;             // d beyond D: zeros for both operands
            float* dst = st + (wave * 4 + i) * 256;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)dst, 16, vx, k0 * 4, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, (__attribute__((address_space(3))) void*)(dst + kKmTile), 16, vc, k0 * 4, 0, 0);
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
    float best[2] = {-INFINITY, -INFINITY};
    int bidx[2] = {0, 0};

    const int total = (cb1 - cb0) * nk;
    int cb = cb0, ks = 0;           // the tile being computed
    int icb = cb0, iks = 0;         // the tile being fetched
    issue(icb, iks, smem);
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();            // tile s has landed for everyone; everyone has finished reading tile s - 1
        if (s + 1 < total) {
            if (++iks == nk) { iks = 0; ++icb; }
            issue(icb, iks, smem + ((s + 1) & 1) * 2 * kKmTile);
        }
        const float* xs = smem + (s & 1) * 2 * kKmTile + (wn * 64 + c) * kKmBK;
        const float* cs = smem + (s & 1) * 2 * kKmTile + kKmTile + (wm * 64 + c) * kKmBK;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const f32x4*>(cs + i * 32 * kKmBK + pos[g]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f32x4*>(xs + j * 32 * kKmBK + pos[g]);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][jj], b[j][jj], acc[i][j], 0, 0, 0);
        }
        if (++ks == nk) {           // a centre block is complete: scores, running maximum in increasing centre order (strict >: lowest index)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kidx = cb * kKmB + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float hv = kidx < K ? hh[kidx] : (MET == LDS_METRIC_COSINE ? 0.f : INFINITY);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        float v;
                        if constexpr (MET == LDS_METRIC_COSINE) v = kidx < K ? acc[i][j][r] * hv : -INFINITY;
                        else v = acc[i][j][r] - hv;
                        if (v > best[j]) { best[j] = v; bidx[j] = kidx; }
                        acc[i][j][r] = 0.f;
                    }
                }
            ks = 0;
            ++cb;
        }
    }
    __syncthreads();
    float* rv = smem;
    int* ri = reinterpret_cast<int*>(smem + 4 * kKmB);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        rv[(wm * 2 + h) * kKmB + wn * 64 + j * 32 + c] = best[j];
        ri[(wm * 2 + h) * kKmB + wn * 64 + j * 32 + c] = bidx[j];
    }
    __syncthreads();
    if (tid < rows) {
        float bv = rv[tid];
        int bi = ri[tid];
#pragma unroll
        for (int q = 1; q < 4; ++q) km_take(rv[q * kKmB + tid], ri[q * kKmB + tid], bv, bi);
        const long long n = n0 + tid;
        if (pval) {
            pval[(long long)blockIdx.y * N + n] = bv;
            pidx[(long long)blockIdx.y * N + n] = bi;
        } else {
            const bool padded = lens.n > 0 && (int)(n % lens.T) >= lens.v[n / lens.T];
            labels[n] = padded ? (long long)lens.pad : (long long)bi;
            if (best_out) best_out[n] = padded ? 0.f : bv;
        }
    }
}

// joins the per-split partial maxima of a row in split order (any order gives the same answer)
__global__ void __launch_bounds__(256) kmeans_join_kernel(const float* __restrict__ pval, const int* __restrict__ pidx, int KS, long long N,
                                                          long long* __restrict__ labels, float* __restrict__ best_out, const KmLens lens) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float bv = pval[n];
    int bi = pidx[n];
    for (int q = 1; q < KS; ++q) km_take(pval[q * N + n], pidx[q * N + n], bv, bi);
    const bool padded = lens.n > 0 && (int)(n % lens.T) >= lens.v[n / lens.T];
    labels[n] = padded ? (long long)lens.pad : (long long)bi;
    if (best_out) best_out[n] = padded ? 0.f : bv;
}

// sum over the 256 threads of a workgroup in a fixed tree
template <typename T>
static __device__ __forceinline__ T km_block_sum(T v, T* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] = sh[tid] + sh[tid + o];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// cosine only: best[n] *= r(x_n), after the arg-max is decided.  One wave per row: the sum of squares in kmeans_prepare_kernel's order.
// Rows at and beyond a clip's length keep their 0.
__global__ void __launch_bounds__(256) kmeans_cos_best_kernel(const float* __restrict__ X, long long N, int D, float* __restrict__ best, const KmLens lens) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    if (lens.n > 0 && (int)(n % lens.T) >= lens.v[n / lens.T]) return;
    const float* r = X + n * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(r[d], r[d], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) best[n] = __fmul_rn(best[n], km_row_const(s));
}

// h[k] = |c_k|^2 / 2 (metric L2) or r_k = 1 / max(|c_k|, 1e-12) (cosine): one wave per centre, lanes stride the columns, fixed butterfly
__global__ void __launch_bounds__(256) kmeans_prepare_kernel(const float* __restrict__ Cc, int K, int D, float* __restrict__ hh, int metric) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const float* r = Cc + (long long)k * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(r[d], r[d], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) hh[k] = metric == LDS_METRIC_COSINE ? km_row_const(s) : 0.5f * s;
}

// ---- update: stable counting sort by label, then per-cluster sums in row order ----
// a label outside [0, K) belongs to no cluster: the row is ignored
__global__ void __launch_bounds__(256) kmeans_hist_kernel(const long long* __restrict__ labels, long long N, int K, long long per, int* __restrict__ hist) {
    const long long r0 = blockIdx.x * per, r1 = r0 + per < N ? r0 + per : N;
    int* hb = hist + (long long)blockIdx.x * K;
    for (long long r = r0 + threadIdx.x; r < r1; r += 256) {
        const long long l = labels[r];
        if (l >= 0 && l < K) atomicAdd(hb + l, 1);
    }
}
// hist[b][k] -> rows of cluster k in the row blocks before b; counts[k] = the cluster's size
__global__ void __launch_bounds__(256) kmeans_colscan_kernel(int* __restrict__ hist, int NB, int K, int* __restrict__ counts) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    int run = 0;
    for (int b = 0; b < NB; ++b) {
        const int v = hist[(long long)b * K + k];
        hist[(long long)b * K + k] = run;
        run += v;
    }
    counts[k] = run;
}
// offsets = exclusive prefix of counts (one workgroup)
__global__ void __launch_bounds__(256) kmeans_offsets_kernel(const int* __restrict__ counts, int K, int* __restrict__ offsets) {
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (K + 255) / 256;
    const int k0 = tid * per, k1 = k0 + per < K ? k0 + per : K;
    int s = 0;
    for (int k = k0; k < k1; ++k) s += counts[k];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    int run = part[tid];
    for (int k = k0; k < k1; ++k) { offsets[k] = run; run += counts[k]; }
}
// one workgroup per row block walks its rows 256 at a time; a row's slot = cluster offset + rows of the cluster in earlier blocks and
// chunks (the cursor in hist) + equal labels before it in the chunk: the sorted list of every cluster is in increasing row order
__global__ void __launch_bounds__(256) kmeans_scatter_kernel(const long long* __restrict__ labels, long long N, int K, long long per, int* __restrict__ hist,
                                                             const int* __restrict__ offsets, int* __restrict__ sorted) {
    __shared__ int lab[256];
    const int tid = threadIdx.x;
    const long long r0 = blockIdx.x * per, r1 = r0 + per < N ? r0 + per : N;
    int* hb = hist + (long long)blockIdx.x * K;
    for (long long base = r0; base < r1; base += 256) {
        const long long r = base + tid;
        int l = -1;
        if (r < r1) {
            const long long ll = labels[r];
            if (ll >= 0 && ll < K) l = (int)ll;
        }
        lab[tid] = l;
        __syncthreads();
        int rank = 0, cur = 0;
        bool last = true;
        if (l >= 0) {
            for (int t = 0; t < tid; ++t) rank += lab[t] == l;
            for (int t = tid + 1; t < 256; ++t) last = last && lab[t] != l;
            cur = atomicAdd(hb + l, 0);
            sorted[offsets[l] + cur + rank] = (int)r;
        }
        __syncthreads();
        if (l >= 0 && last) atomicExch(hb + l, cur + rank + 1);
        __syncthreads();
    }
}
// grid (K, ceil(D / 256)): thread = one column of one cluster.  c_grad = sum / count (empty cluster: a zero row, the reference's NaN
// removal), error partial = sum (c_grad - C)^2 over the block, lr = 1 / num_points * 0.9 + 0.1, C = C (1 - lr) + c_grad lr -- the
// reference's fp32 operations one by one (kmeans.py:188-198).  num_points is read only: kmeans_finish_kernel adds the counts.
__global__ void __launch_bounds__(256) kmeans_sum_kernel(const float* __restrict__ X, const int* __restrict__ sorted, const int* __restrict__ offsets,
                                                         const int* __restrict__ counts, float* __restrict__ Cc, const float* __restrict__ num_points, int D,
                                                         float* __restrict__ errpart) {
    __shared__ float sh[256];
    const int k = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    const int cnt = counts[k];
    const int* rows = sorted + offsets[k];
    const bool on = col < D;
    float s = 0.f;
    int i = 0;
    for (; i + 4 <= cnt; i += 4) {
        const long long a0 = rows[i], a1 = rows[i + 1], a2 = rows[i + 2], a3 = rows[i + 3];
        const float v0 = on ? X[a0 * D + col] : 0.f, v1 = on ? X[a1 * D + col] : 0.f, v2 = on ? X[a2 * D + col] : 0.f, v3 = on ? X[a3 * D + col] : 0.f;
        s = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(s, v0), v1), v2), v3);
    }
    for (; i < cnt; ++i) s = __fadd_rn(s, on ? X[(long long)rows[i] * D + col] : 0.f);
    float e = 0.f;
    if (on) {
        const float g = cnt > 0 ? __fdiv_rn(s, (float)cnt) : 0.f;
        const float cv = Cc[(long long)k * D + col];
        const float d = __fsub_rn(g, cv);
        e = __fmul_rn(d, d);
        const float lr = __fadd_rn(__fmul_rn(__fdiv_rn(1.0f, num_points[k]), 0.9f), 0.1f);
        Cc[(long long)k * D + col] = __fadd_rn(__fmul_rn(cv, __fsub_rn(1.0f, lr)), __fmul_rn(g, lr));
    }
    const float t = km_block_sum(e, sh);
    if (threadIdx.x == 0) errpart[(long long)k * gridDim.y + blockIdx.y] = t;
}
// one workgroup: error = the partials summed in a fixed order (thread t takes t, t + 256, ...; then the tree); num_points += counts
__global__ void __launch_bounds__(256) kmeans_finish_kernel(const float* __restrict__ errpart, long long n_part, const int* __restrict__ counts, int K,
                                                            float* __restrict__ num_points, float* __restrict__ error) {
    __shared__ float sh[256];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n_part; i += 256) s = __fadd_rn(s, errpart[i]);
    const float t = km_block_sum(s, sh);
    if (threadIdx.x == 0) *error = t;
    for (int k = threadIdx.x; k < K; k += 256) num_points[k] = __fadd_rn(num_points[k], (float)counts[k]);
}

// ---- k-means++ seeding ----
// dist[n] = |x_n - c_new| (the Euclidean distance, not its square: torch.cdist(p=2)), mind = min(mind, dist); one wave per row, a workgroup
// takes 256 rows and leaves their sum in double (fixed tree)
__global__ void __launch_bounds__(256) kmeans_seed_dist_kernel(const float* __restrict__ X, long long N, int D, const float* __restrict__ cnew, int first,
                                                               float* __restrict__ mind, double* __restrict__ blocksum) {
    __shared__ double sh[256];
    __shared__ float w[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 256;
    for (int q = 0; q < 64; ++q) {
        const long long r = r0 + wave * 64 + q;
        float m = 0.f;
        if (r < N) {
            const float* xr = X + r * D;
            float s = 0.f;
            for (int d = lane; d < D; d += 64) {
                const float t = xr[d] - cnew[d];
                s = fmaf(t, t, s);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const float dd = sqrtf(s);
            m = first ? dd : fminf(mind[r], dd);
            if (lane == 0) mind[r] = m;
        }
        if (lane == 0) w[wave * 64 + q] = m;
    }
    __syncthreads();
    const double t = km_block_sum((double)w[threadIdx.x], sh);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = t;
}
// one workgroup: pick = first j with prefix_j >= u * total, prefix in double in a fixed order (256 contiguous runs of block sums, the
// runs in order, the blocks of the run in order, the rows of the block in order), clamped to N - 1; forced >= 0: that index instead.
// The chosen row is copied to `cdst` and its index stored to `picked_i`.
__global__ void __launch_bounds__(256) kmeans_seed_pick_kernel(const float* __restrict__ X, long long N, int D, const float* __restrict__ mind,
                                                               const double* __restrict__ blocksum, long long nblk, const float* __restrict__ u, long long forced,
                                                               float* __restrict__ cdst, long long* __restrict__ picked_i) {
    __shared__ double part[256];
    __shared__ long long jsh;
    const int tid = threadIdx.x;
    if (forced < 0) {
        const long long per = (nblk + 255) / 256;
        const long long b0 = tid * per, b1 = b0 + per < nblk ? b0 + per : nblk;
        double s = 0.0;
        for (long long b = b0; b < b1; ++b) s += blocksum[b];
        part[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
            for (int t = 0; t < 256; ++t) total += part[t];
            const double target = (double)u[0] * total;
            long long j = N - 1;
            double run = 0.0;
            int t = 0;
            for (; t < 256; ++t) {
                if (run + part[t] >= target) break;
                run += part[t];
            }
            if (t < 256) {
                long long b = (long long)t * per;
                const long long be = b + per < nblk ? b + per : nblk;
                for (; b < be; ++b) {
                    if (run + blocksum[b] >= target) break;
                    run += blocksum[b];
                }
                // (the run's blocks added one by one may round differently from the run's sum, and a block's rows from the block's sum:
                // a search that comes up short by that rounding takes the last block of the run / the last row of the block)
                if (b == be) { b = be - 1; run -= blocksum[b]; }
                const long long re = (b + 1) * 256 < N ? (b + 1) * 256 : N;
                j = re - 1;
                for (long long r = b * 256; r < re; ++r) {
                    run += (double)mind[r];
                    if (run >= target) { j = r; break; }
                }
            }
            jsh = j;
        }
    } else if (tid == 0) {
        jsh = forced;
    }
    __syncthreads();
    const long long j = jsh;
    for (int d = tid; d < D; d += 256) cdst[d] = X[j * D + d];
    if (tid == 0) *picked_i = j;
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

using lds::set_error;

struct KmPlan {
    int KS, cbps;               // assign: centre splits, centre blocks per split
    int NB; long long per;      // update: row blocks of the counting sort, rows per block
    long long nblk;             // seeding: 256-row blocks
    size_t o_pval, o_pidx, o_hist, o_counts, o_offsets, o_sorted, o_err, o_mind, o_bsum, o_picked, bytes;
};

int km_check_dims(const char* fn, long long N, int K, int D) {
    if (D < 8 || D > 4096 || D % 8) return set_error(LDS_EINVAL, "%s: D %d must be a multiple of 8 in 8 .. 4096", fn, D);
    if (K < 1 || K > 65536) return set_error(LDS_EINVAL, "%s: K %d outside 1 .. 65536", fn, K);
    if (N < 1 || N > 2147483000LL) return set_error(LDS_EINVAL, "%s: N %lld outside 1 .. 2147483000", fn, N);
    return LDS_OK;
}

KmPlan km_plan(long long N, int K, int D) {
    KmPlan p;
    const long long rb = (N + lds::kKmB - 1) / lds::kKmB;
    const int nCB = (K + lds::kKmB - 1) / lds::kKmB;
    long long ks = rb >= 512 ? 1 : 512 / rb;      // enough workgroups for two per CU when the row blocks alone do not give them
    if (ks > nCB) ks = nCB;
    p.cbps = (int)((nCB + ks - 1) / ks);
    p.KS = (nCB + p.cbps - 1) / p.cbps;
    long long nb = (N + 255) / 256, cap = (16LL << 20) / K;      // at most 16 Mi histogram entries
    if (cap > 1024) cap = 1024;
    if (cap < 1) cap = 1;
    if (nb > cap) nb = cap;
    p.NB = (int)nb;
    p.per = (N + nb - 1) / nb;
    p.nblk = (N + 255) / 256;
    Slots S;
    p.o_pval = S.take(p.KS > 1 ? (size_t)p.KS * N * 4 : 0);
    p.o_pidx = S.take(p.KS > 1 ? (size_t)p.KS * N * 4 : 0);
    p.o_hist = S.take((size_t)p.NB * K * 4);
    p.o_counts = S.take((size_t)K * 4);
    p.o_offsets = S.take((size_t)K * 4);
    p.o_sorted = S.take((size_t)N * 4);
    p.o_err = S.take((size_t)K * ((D + 255) / 256) * 4);
    p.o_mind = S.take((size_t)N * 4);
    p.o_bsum = S.take((size_t)p.nblk * 8);
    p.o_picked = S.take((size_t)K * 8);
    p.bytes = S.o;
    return p;
}

int km_check_metric(const char* fn, int metric) {
    if (metric != LDS_METRIC_L2 && metric != LDS_METRIC_COSINE) return set_error(LDS_EINVAL, "%s: metric %d is neither LDS_METRIC_L2 nor LDS_METRIC_COSINE", fn, metric);
    return LDS_OK;
}

int km_assign(const char* fn, int metric, const float* X, long long N, const float* C, const float* h, int K, int D, int64_t* labels, float* best, void* ws,
              size_t ws_bytes, const lds::KmLens& lens, hipStream_t s) {
    if (int rc = km_check_metric(fn, metric)) return rc;
    if (!X || !C || !h || !labels || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const KmPlan p = km_plan(N, K, D);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    char* w = (char*)ws;
    float* pval = p.KS > 1 ? (float*)(w + p.o_pval) : nullptr;
    int* pidx = p.KS > 1 ? (int*)(w + p.o_pidx) : nullptr;
    {
        lds::ProfScope ps(s, "kmeans_assign", 2.0 * (double)N * K * D, 4.0 * ((double)N * D + (double)K * D * ((N + 127) / 128)));
        const dim3 grid((unsigned)((N + lds::kKmB - 1) / lds::kKmB), p.KS);
        if (metric == LDS_METRIC_COSINE)
            hipLaunchKernelGGL(lds::kmeans_assign_kernel<LDS_METRIC_COSINE>, grid, dim3(256), 0, s, X, N, C, h, K, D, p.cbps, (long long*)labels, best, pval, pidx, lens);
        else
            hipLaunchKernelGGL(lds::kmeans_assign_kernel<LDS_METRIC_L2>, grid, dim3(256), 0, s, X, N, C, h, K, D, p.cbps, (long long*)labels, best, pval, pidx, lens);
    }
    if (p.KS > 1)
        hipLaunchKernelGGL(lds::kmeans_join_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, pval, pidx, p.KS, N, (long long*)labels, best, lens);
    if (metric == LDS_METRIC_COSINE && best)
        hipLaunchKernelGGL(lds::kmeans_cos_best_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, X, N, D, best, lens);
    return launched(fn);
}

}  // namespace

extern "C" int lds_kmeans_workspace_bytes(int64_t N, int K, int D, size_t* out) {
    if (!out) return set_error(LDS_EINVAL, "lds_kmeans_workspace_bytes: null out");
    if (int rc = km_check_dims("lds_kmeans_workspace_bytes", N, K, D)) return rc;
    *out = km_plan(N, K, D).bytes;
    return LDS_OK;
}

namespace {
int km_prepare(const char* fn, int metric, const float* C, int K, int D, float* h, void* stream) {
    if (int rc = km_check_metric(fn, metric)) return rc;
    if (int rc = km_check_dims(fn, 1, K, D)) return rc;
    if (!C || !h) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipLaunchKernelGGL(lds::kmeans_prepare_kernel, dim3((K + 3) / 4), dim3(256), 0, (hipStream_t)stream, C, K, D, h, metric);
    return launched(fn);
}
}  // namespace

extern "C" int lds_kmeans_prepare(const float* C, int K, int D, float* h, void* stream) {
    return km_prepare("lds_kmeans_prepare", LDS_METRIC_L2, C, K, D, h, stream);
}
extern "C" int lds_kmeans_prepare_metric(const float* C, int K, int D, int metric, float* h, void* stream) {
    return km_prepare("lds_kmeans_prepare_metric", metric, C, K, D, h, stream);
}

namespace {
int km_assign_plain(const char* fn, int metric, const float* X, int64_t N, const float* C, const float* h, int K, int D, int64_t* labels, float* best, void* ws,
                    size_t ws_bytes, void* stream) {
    if (int rc = km_check_dims(fn, N, K, D)) return rc;
    lds::KmLens lens;
    lens.n = 0; lens.T = 1; lens.pad = 0;
    for (int i = 0; i < 64; ++i) lens.v[i] = 0;
    return km_assign(fn, metric, X, N, C, h, K, D, labels, best, ws, ws_bytes, lens, (hipStream_t)stream);
}
}  // namespace

extern "C" int lds_kmeans_assign(const float* X, int64_t N, const float* C, const float* h, int K, int D, int64_t* labels, float* best, void* ws,
                                 size_t ws_bytes, void* stream) {
    return km_assign_plain("lds_kmeans_assign", LDS_METRIC_L2, X, N, C, h, K, D, labels, best, ws, ws_bytes, stream);
}
extern "C" int lds_kmeans_assign_metric(const float* X, int64_t N, const float* C, const float* h, int K, int D, int metric, int64_t* labels, float* best,
                                        void* ws, size_t ws_bytes, void* stream) {
    return km_assign_plain("lds_kmeans_assign_metric", metric, X, N, C, h, K, D, labels, best, ws, ws_bytes, stream);
}

namespace {
int km_assign_ragged(const char* fn, int metric, const float* X, int B, int T, const int32_t* lengths, int64_t pad_id, const float* C, const float* h, int K, int D,
                     int64_t* labels, float* best, void* ws, size_t ws_bytes, void* stream) {
    if (B < 1 || B > 64 || T < 1) return set_error(LDS_EINVAL, "%s: B %d outside 1 .. 64 or T %d < 1", fn, B, T);
    if (!lengths) return set_error(LDS_EINVAL, "%s: null lengths", fn);
    if (pad_id < -2147483647LL || pad_id > 2147483647LL) return set_error(LDS_EINVAL, "%s: pad_id %lld does not fit 32 bits", fn, (long long)pad_id);
    if (int rc = km_check_dims(fn, (long long)B * T, K, D)) return rc;
    lds::KmLens lens;
    lens.n = B; lens.T = T; lens.pad = (int)pad_id;
    for (int i = 0; i < 64; ++i) lens.v[i] = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] < 0 || lengths[b] > T) return set_error(LDS_EINVAL, "%s: lengths[%d] = %d outside 0 .. %d", fn, b, lengths[b], T);
        lens.v[b] = lengths[b];
    }
    return km_assign(fn, metric, X, (long long)B * T, C, h, K, D, labels, best, ws, ws_bytes, lens, (hipStream_t)stream);
}
}  // namespace

extern "C" int lds_kmeans_assign_ragged(const float* X, int B, int T, const int32_t* lengths, int64_t pad_id, const float* C, const float* h, int K, int D,
                                        int64_t* labels, float* best, void* ws, size_t ws_bytes, void* stream) {
    return km_assign_ragged("lds_kmeans_assign_ragged", LDS_METRIC_L2, X, B, T, lengths, pad_id, C, h, K, D, labels, best, ws, ws_bytes, stream);
}
extern "C" int lds_kmeans_assign_ragged_metric(const float* X, int B, int T, const int32_t* lengths, int64_t pad_id, const float* C, const float* h, int K,
                                               int D, int metric, int64_t* labels, float* best, void* ws, size_t ws_bytes, void* stream) {
    return km_assign_ragged("lds_kmeans_assign_ragged_metric", metric, X, B, T, lengths, pad_id, C, h, K, D, labels, best, ws, ws_bytes, stream);
}

namespace {
int km_update(const char* fn, int metric, const float* X, const int64_t* labels, int64_t N, float* C, float* h, float* num_points, int K, int D, float* error,
              void* ws, size_t ws_bytes, void* stream) {
    if (int rc = km_check_metric(fn, metric)) return rc;
    if (int rc = km_check_dims(fn, N, K, D)) return rc;
    if (!X || !labels || !C || !h || !num_points || !error || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const KmPlan p = km_plan(N, K, D);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    int* hist = (int*)(w + p.o_hist);
    int* counts = (int*)(w + p.o_counts);
    int* offsets = (int*)(w + p.o_offsets);
    int* sorted = (int*)(w + p.o_sorted);
    float* errpart = (float*)(w + p.o_err);
    const int ncb = (D + 255) / 256;
    if (hipMemsetAsync(hist, 0, (size_t)p.NB * K * 4, s) != hipSuccess) return set_error(LDS_EHIP, "%s: hipMemsetAsync failed", fn);
    hipLaunchKernelGGL(lds::kmeans_hist_kernel, dim3(p.NB), dim3(256), 0, s, (const long long*)labels, (long long)N, K, p.per, hist);
    hipLaunchKernelGGL(lds::kmeans_colscan_kernel, dim3((K + 255) / 256), dim3(256), 0, s, hist, p.NB, K, counts);
    hipLaunchKernelGGL(lds::kmeans_offsets_kernel, dim3(1), dim3(256), 0, s, counts, K, offsets);
    hipLaunchKernelGGL(lds::kmeans_scatter_kernel, dim3(p.NB), dim3(256), 0, s, (const long long*)labels, (long long)N, K, p.per, hist, offsets, sorted);
    {
        lds::ProfScope ps(s, "kmeans_sum", (double)N * D, 4.0 * (double)N * D);
        hipLaunchKernelGGL(lds::kmeans_sum_kernel, dim3(K, ncb), dim3(256), 0, s, X, sorted, offsets, counts, C, num_points, D, errpart);
    }
    hipLaunchKernelGGL(lds::kmeans_finish_kernel, dim3(1), dim3(256), 0, s, errpart, (long long)K * ncb, counts, K, num_points, error);
    hipLaunchKernelGGL(lds::kmeans_prepare_kernel, dim3((K + 3) / 4), dim3(256), 0, s, C, K, D, h, metric);
    return launched(fn);
}
}  // namespace

extern "C" int lds_kmeans_update(const float* X, const int64_t* labels, int64_t N, float* C, float* h, float* num_points, int K, int D, float* error,
                                 void* ws, size_t ws_bytes, void* stream) {
    return km_update("lds_kmeans_update", LDS_METRIC_L2, X, labels, N, C, h, num_points, K, D, error, ws, ws_bytes, stream);
}
extern "C" int lds_kmeans_update_metric(const float* X, const int64_t* labels, int64_t N, float* C, float* h, float* num_points, int K, int D, int metric,
                                        float* error, void* ws, size_t ws_bytes, void* stream) {
    return km_update("lds_kmeans_update_metric", metric, X, labels, N, C, h, num_points, K, D, error, ws, ws_bytes, stream);
}

extern "C" int lds_kmeans_seed(const float* X, int64_t N, int D, int K, int64_t first_index, const float* uniforms, float* C, int64_t* picked, void* ws,
                               size_t ws_bytes, void* stream) {
    if (int rc = km_check_dims("lds_kmeans_seed", N, K, D)) return rc;
    if (K > N) return set_error(LDS_EINVAL, "lds_kmeans_seed: K %d > N %lld", K, (long long)N);
    if (first_index < 0 || first_index >= N) return set_error(LDS_EINVAL, "lds_kmeans_seed: first_index %lld outside 0 .. %lld", (long long)first_index, (long long)N - 1);
    if (!X || !C || !ws || (K > 1 && !uniforms)) return set_error(LDS_EINVAL, "lds_kmeans_seed: null pointer");
    const KmPlan p = km_plan(N, K, D);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "lds_kmeans_seed: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    float* mind = (float*)(w + p.o_mind);
    double* bsum = (double*)(w + p.o_bsum);
    long long* pk = picked ? (long long*)picked : (long long*)(w + p.o_picked);
    hipLaunchKernelGGL(lds::kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, s, X, (long long)N, D, mind, bsum, p.nblk, (const float*)nullptr, (long long)first_index, C, pk);
    for (int i = 1; i < K; ++i) {
        hipLaunchKernelGGL(lds::kmeans_seed_dist_kernel, dim3((unsigned)p.nblk), dim3(256), 0, s, X, (long long)N, D, C + (size_t)(i - 1) * D, i == 1 ? 1 : 0, mind, bsum);
        hipLaunchKernelGGL(lds::kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, s, X, (long long)N, D, mind, bsum, p.nblk, uniforms + (i - 1), -1LL, C + (size_t)i * D, pk + i);
    }
    return launched("lds_kmeans_seed");
}
