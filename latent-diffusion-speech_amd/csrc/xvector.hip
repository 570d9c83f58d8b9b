// The x-vector speaker head on the speech encoders (transformers' WavLMForXVector / Wav2Vec2ForXVector: projector, TDNN layers, statistics
// pooling, feature_extractor, classifier) and the cosine of two embeddings, exact fp32, gfx950.  include/lds.h states the semantics.
//   tdnn     y[t][o] = act(b[o] + sum_j sum_c x[t + j d][c] W[o][j Cin + c]) over a clip's own frames, on v_mfma_f32_32x32x2_f32 with
//            ctc.hip's (= kmeans.hip's assign) tiling: both operand tiles HBM/L2 -> LDS by LDS-DMA, the same swizzle, one fmaf chain per
//            (t, o) in k order.  W [Cout][ks Cin] is tap-major, so the weight tile is the assign's with D = ks Cin; the frame tile of a K-block
//            of tap j is the same tile with its row base moved by j d frames (Cin is a multiple of the K-step: no K-block spans two taps).
//            grid (row blocks of T, column blocks of Cout, B): a tile never spans two clips, and a clip's cut into tiles depends on its own
//            length only.  The buffer descriptor of the frame tile ends at the clip's last valid frame: nothing at or beyond it is read.
//   pool     POOL = true: the same kernel, but instead of storing y the tile goes through LDS once and every channel's valid frames of
//            each 64-frame half become (mean, M2 about that mean) in frame order; xv_pool_join_kernel combines a clip's partials in
//            order with Chan's update and writes mean and sqrt(M2 / (n - 1)).  No atomics; a constant channel has M2 = 0 exactly (the
//            first pass sums differences from the half's first frame, the update of equal means adds nothing).
//   cosine   one wave per pair.
// The two small linears behind the pooling are misc.hip's small_linear.
#include "../../include/lds.h"
#include "../../include/lds_test.h"
#include "kernels.h"
#include "host.h"

#include <math.h>

#include <string>
#include <vector>

namespace lds {

typedef float xf32x16 __attribute__((ext_vector_type(16)));
typedef float xf32x4 __attribute__((ext_vector_type(4)));

constexpr int kXvB = 128;                // frames / channels per tile
constexpr int kXvBK = 32;                // k per K-step: one 128-byte line of every row
constexpr int kXvTile = kXvB * kXvBK;    // floats per operand tile
constexpr int kXvHalf = 64;              // frames per pooling partial

struct XvLens { int B, T; int v[64]; };      // B clips of T rows, v[b] valid INPUT rows

// 256 threads = 2 x 2 waves; wave (wm, wn) owns channels wm*64 .. +64 (MFMA rows, spread over the accumulator registers) and frames
// wn*64 .. +64 (MFMA columns, one per lane) of a 128 x 128 tile.
// POOL false: Y [B][T][Cout] = act(.) in the clip's rows below T_out = v[b] - (ks - 1) d, zeros in the rows from T_out to T.
// POOL true:  part [B][2 ceil(T / 128)][Cout] float2 = (mean, M2) of the tile's two 64-frame halves (halves without a valid frame are not written).
template <bool POOL>
__global__ void __launch_bounds__(256) xv_tdnn_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias, int Cin, int Cout,
                                                      int ks, int dil, int relu, float* __restrict__ Y, float2* __restrict__ part, const XvLens lens) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kXvTile];      // 2 stages x (X tile, W tile) = 64 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int clip = blockIdx.z, T = lens.T;
    const int t0 = blockIdx.x * kXvB, cb = blockIdx.y;
    const int n_in = lens.v[clip];
    int rows = n_in - (ks - 1) * dil - t0;                                  // valid output rows of this tile
    rows = rows < kXvB ? rows : kXvB;
    const int trows = T - t0 < kXvB ? T - t0 : kXvB;                        // rows of the tile inside the tensor
    if (rows <= 0) {                                                        // (uniform: before any barrier)
        if constexpr (!POOL) {
            const int cw = Cout - cb * kXvB < kXvB ? Cout - cb * kXvB : kXvB;
            for (int e = tid; e < trows * (cw >> 2); e += 256) {
                const int r = e / (cw >> 2), q = e - r * (cw >> 2);
                *reinterpret_cast<xf32x4*>(Y + ((long long)clip * T + t0 + r) * Cout + cb * kXvB + q * 4) = xf32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        return;
    }
    const int K = ks * Cin, nk = K / kXvBK;
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X + ((long long)clip * T + t0) * Cin), 0, (n_in - t0) * Cin * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, Cout * K * 4, 0x00020000);
    int xoff[4], woff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        xoff[i] = (row < rows ? row : rows - 1) * Cin * 4 + ch * 16;        // rows beyond T_out read the last valid row (their results are not used)
        int kr = cb * kXvB + row;
        kr = kr < Cout ? kr : Cout - 1;                                     // channels beyond Cout read the last one (masked in the epilogue)
        woff[i] = kr * K * 4 + ch * 16;
    }
    auto issue = [&](int s, float* st) {
        const int k0 = s * kXvBK;
        const int tap = k0 / Cin;                                           // (Cin is a multiple of kXvBK: the whole K-block is tap `tap`)
        const int xs = (tap * dil * Cin + (k0 - tap * Cin)) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float* dst = st + (wave * 4 + i) * 256;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)dst, 16, xoff[i], xs, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, (__attribute__((address_space(3))) void*)(dst + kXvTile), 16, woff[i], k0 * 4, 0, 0);
        }
    };
    int pos[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) pos[g] = ((2 * g + h) ^ ((c >> 1) & 7)) * 4;
    xf32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    issue(0, smem);
    for (int s = 0; s < nk; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();            // tile s has landed for everyone; everyone has finished reading tile s - 1
        if (s + 1 < nk) issue(s + 1, smem + ((s + 1) & 1) * 2 * kXvTile);
        const float* xs = smem + (s & 1) * 2 * kXvTile + (wn * 64 + c) * kXvBK;
        const float* cs = smem + (s & 1) * 2 * kXvTile + kXvTile + (wm * 64 + c) * kXvBK;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            xf32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const xf32x4*>(cs + i * 32 * kXvBK + pos[g]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const xf32x4*>(xs + j * 32 * kXvBK + pos[g]);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][jj], b[j][jj], acc[i][j], 0, 0, 0);
        }
    }
    // y = act(dot + bias): register (i, j, r) holds channel wm*64 + i*32 + (r & 3) + 8 (r >> 2) + 4 h of frame wn*64 + j*32 + c
    if constexpr (!POOL) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kidx = cb * kXvB + wm * 64 + i * 32 + 8 * q + 4 * h;      // 4 consecutive channels (Cout is a multiple of 4)
                if (kidx < Cout) {
                    const xf32x4 bv = *reinterpret_cast<const xf32x4*>(bias + kidx);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int row = wn * 64 + j * 32 + c;
                        if (row < trows) {
                            xf32x4 v;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                float y = __fadd_rn(acc[i][j][4 * q + e], bv[e]);
                                if (relu) y = fmaxf(y, 0.f);
                                v[e] = row < rows ? y : 0.f;
                            }
                            *reinterpret_cast<xf32x4*>(Y + ((long long)clip * T + t0 + row) * Cout + kidx) = v;
                        }
                    }
                }
            }
    } else {
        __syncthreads();            // everyone has finished reading the last operand tiles: smem becomes the 128 x 128 tile of y
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kloc = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int kidx = cb * kXvB + kloc;
                const float bv = kidx < Cout ? bias[kidx] : 0.f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int row = wn * 64 + j * 32 + c;
                    float y = __fadd_rn(acc[i][j][r], bv);
                    if (relu) y = fmaxf(y, 0.f);
                    smem[kloc * kXvB + (row ^ (kloc & 31))] = y;      // (the xor spreads a channel's frames and a frame's channels over the banks)
                }
            }
        __syncthreads();
        const int kloc = tid & 127, half = tid >> 7, kidx = cb * kXvB + kloc;
        const int r0 = half * kXvHalf;
        const int n = rows - r0 < kXvHalf ? rows - r0 : kXvHalf;
        if (n > 0 && kidx < Cout) {
            const float* ys = smem + kloc * kXvB;
            const int sw = kloc & 31;
            const float pivot = ys[r0 ^ sw];
            // four interleaved chains (frame r into chain r % 4), joined as (0 + 1) + (2 + 3): a quarter of one chain's rounding, the same order always
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < n; r += 4)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (r + e < n) s[e] = __fadd_rn(s[e], __fsub_rn(ys[(r0 + r + e) ^ sw], pivot));
            const float sbar = __fdiv_rn(__fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3])), (float)n);      // the mean's distance from the pivot
            const float mean = __fadd_rn(pivot, sbar);
            float q[4] = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < n; r += 4)                                   // (y - pivot) - sbar: the deviations never see the rounding of pivot + sbar
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (r + e < n) {
                        const float d = __fsub_rn(__fsub_rn(ys[(r0 + r + e) ^ sw], pivot), sbar);
                        q[e] = fmaf(d, d, q[e]);
                    }
            const float m2 = __fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3]));
            const int nP = 2 * ((T + kXvB - 1) / kXvB);
            part[((long long)clip * nP + 2 * blockIdx.x + half) * Cout + kidx] = make_float2(mean, m2);
        }
    }
}

// stats [B][2 C]: a clip's partials combined in frame order (Chan, Golub, LeVeque: n = na + nb, delta = mb - ma, mean = ma + delta nb / n,
// M2 = M2a + M2b + delta^2 na nb / n), then mean and the unbiased standard deviation sqrt(M2 / (n - 1)) (torch.std).  One thread per
// (clip, channel); consecutive threads consecutive channels.  tout[b] >= 2 has been checked.
__global__ void __launch_bounds__(256) xv_pool_join_kernel(const float2* __restrict__ part, float* __restrict__ stats, int C, int span, const XvLens lens) {
    const int ch = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (ch >= C) return;
    const int tout = lens.v[b] - span;
    const int nP = 2 * ((lens.T + kXvB - 1) / kXvB);
    float na = 0.f, mean = 0.f, m2 = 0.f;
    for (int p = 0; p * kXvHalf < tout; ++p) {
        const float nb = (float)(tout - p * kXvHalf < kXvHalf ? tout - p * kXvHalf : kXvHalf);
        const float2 q = part[((long long)b * nP + p) * C + ch];
        if (p == 0) {
            na = nb; mean = q.x; m2 = q.y;
        } else {
            const float n = na + nb, delta = __fsub_rn(q.x, mean);
            mean = fmaf(delta, __fdiv_rn(nb, n), mean);
            m2 = __fadd_rn(__fadd_rn(m2, q.y), __fmul_rn(__fmul_rn(delta, delta), __fdiv_rn(__fmul_rn(na, nb), n)));
            na = n;
        }
    }
    stats[(long long)b * 2 * C + ch] = mean;
    stats[(long long)b * 2 * C + C + ch] = sqrtf(__fdiv_rn(m2, na - 1.f));
}

// out[i][j] = a_i . b_j / (max(|a_i|, 1e-8) max(|b_j|, 1e-8)) (torch.nn.functional.cosine_similarity).  grid (M, N), one wave per pair: a
// lane adds its elements in index order, the 64 partial sums meet in a fixed butterfly.
__global__ void __launch_bounds__(64) xv_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, int dim, int M, float* __restrict__ out) {
    const int j = blockIdx.x, i = blockIdx.y, lane = threadIdx.x;
    const float* ai = a + (long long)i * dim;
    const float* bj = b + (long long)j * dim;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int k = lane; k < dim; k += 64) {
        const float x = ai[k], y = bj[k];
        ab = fmaf(x, y, ab); aa = fmaf(x, x, aa); bb = fmaf(y, y, bb);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ab += __shfl_xor(ab, o, 64); aa += __shfl_xor(aa, o, 64); bb += __shfl_xor(bb, o, 64);
    }
    if (lane == 0) out[(long long)i * M + j] = __fdiv_rn(ab, __fmul_rn(fmaxf(sqrtf(aa), 1e-8f), fmaxf(sqrtf(bb), 1e-8f)));
}

}  // namespace lds

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/lds.h, include/lds_test.h)
// ---------------------------------------------------------------------------------------------------------------------------------
struct lds_xvector {
    lds_xvector_cfg cfg;
    int n_labels = 0;
    Owner own;
    float *proj_w = nullptr, *proj_b = nullptr, *fe_w = nullptr, *fe_b = nullptr, *cl_w = nullptr, *cl_b = nullptr;
    float *tdnn_w[8] = {}, *tdnn_b[8] = {};
};

namespace {

using lds::set_error;
constexpr int kXvMaxT = 32768;      // rows per clip: every byte offset of a clip's slab stays below 2^31 at the widest layer

int xv_check_layer(const char* fn, int Cin, int Cout, int ks, int dil) {
    if (Cin < lds::kXvBK || Cin > 4096 || Cin % lds::kXvBK)
        return set_error(LDS_EINVAL, "%s: Cin %d must be a multiple of the K-step %d in %d .. 4096 (a K-block may not span two taps)", fn, Cin, lds::kXvBK, lds::kXvBK);
    if (Cout < 4 || Cout > 4096 || Cout % 4) return set_error(LDS_EINVAL, "%s: Cout %d must be a multiple of 4 in 4 .. 4096", fn, Cout);
    if (ks < 1 || ks > 8) return set_error(LDS_EINVAL, "%s: kernel size %d outside 1 .. 8", fn, ks);
    if (dil < 1 || dil > 8) return set_error(LDS_EINVAL, "%s: dilation %d outside 1 .. 8", fn, dil);
    return LDS_OK;
}

int xv_check_bt(const char* fn, int B, int T) {
    LDS_TRY(range_check(fn, "B", B, 1, 64));
    return range_check(fn, "T", T, 1, kXvMaxT);
}

int xv_lens(const char* fn, int B, int T, const int32_t* n_frames, lds::XvLens& lens) {
    lens.B = B; lens.T = T;
    return clip_lens_fill(fn, "n_frames", B, T, n_frames, lens.v);
}

// one layer over the clips' own frames: into Y, or (part != NULL) into the pooling partials
void xv_layer(const float* X, const float* W, const float* bias, int Cin, int Cout, int ks, int dil, int relu, float* Y, float2* part, const lds::XvLens& lens,
              hipStream_t s) {
    const dim3 grid((lens.T + lds::kXvB - 1) / lds::kXvB, (Cout + lds::kXvB - 1) / lds::kXvB, lens.B);
    double frames = 0.0;
    for (int b = 0; b < lens.B; ++b) frames += lens.v[b];
    lds::ProfScope ps(s, part ? "xv_tdnn_pool" : "xv_tdnn", 2.0 * frames * Cout * ks * Cin, 4.0 * (frames * Cin * grid.y + (double)Cout * ks * Cin * grid.x * lens.B));
    if (part)
        hipLaunchKernelGGL(lds::xv_tdnn_kernel<true>, grid, dim3(256), 0, s, X, W, bias, Cin, Cout, ks, dil, relu, (float*)nullptr, part, lens);
    else
        hipLaunchKernelGGL(lds::xv_tdnn_kernel<false>, grid, dim3(256), 0, s, X, W, bias, Cin, Cout, ks, dil, relu, Y, (float2*)nullptr, lens);
}

void xv_join(const float2* part, float* stats, int C, int span, const lds::XvLens& lens, hipStream_t s) {
    lds::ProfScope ps(s, "xv_pool_join", 0.0, 8.0 * lens.B * (double)C * (2 * ((lens.T + 127) / 128)));
    hipLaunchKernelGGL(lds::xv_pool_join_kernel, dim3((C + 255) / 256, lens.B), dim3(256), 0, s, part, stats, C, span, lens);
}

size_t xv_part_bytes(int B, int T, int C) { return (size_t)B * 2 * ((T + lds::kXvB - 1) / lds::kXvB) * C * sizeof(float2); }

struct XvPlan { size_t o_a, o_b, o_part, o_stats, bytes; };

int xv_span(const lds_xvector_cfg& c) {
    int s = 0;
    for (int i = 0; i < c.n_tdnn; ++i) s += (c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i];
    return s;
}

XvPlan xv_plan(const lds_xvector* h, int B, int T) {
    const lds_xvector_cfg& c = h->cfg;
    int wide = c.tdnn_dim[0];
    for (int i = 0; i + 1 < c.n_tdnn; ++i) wide = wide > c.tdnn_dim[i] ? wide : c.tdnn_dim[i];
    XvPlan p;
    Slots S;
    p.o_a = S.take((size_t)B * T * wide * 4);
    p.o_b = S.take((size_t)B * T * wide * 4);
    p.o_part = S.take(xv_part_bytes(B, T, c.tdnn_dim[c.n_tdnn - 1]));
    p.o_stats = S.take((size_t)B * 2 * c.tdnn_dim[c.n_tdnn - 1] * 4);
    p.bytes = S.o;
    return p;
}

int xv_cfg_check(const lds_xvector_cfg* c) {
    const char* fn = "lds_xvector_create";
    if (c->n_tdnn < 1 || c->n_tdnn > 8) return set_error(LDS_EINVAL, "%s: n_tdnn %d outside 1 .. 8", fn, c->n_tdnn);
    if (int rc = xv_check_layer(fn, c->d_in, c->tdnn_dim[0], 1, 1)) return rc;
    for (int i = 0; i < c->n_tdnn; ++i)
        if (int rc = xv_check_layer(fn, i ? c->tdnn_dim[i - 1] : c->tdnn_dim[0], c->tdnn_dim[i], c->tdnn_kernel[i], c->tdnn_dilation[i])) return rc;
    if (c->xvector_dim < 4 || c->xvector_dim > 4096 || c->xvector_dim % 4)
        return set_error(LDS_EINVAL, "%s: xvector_dim %d must be a multiple of 4 in 4 .. 4096", fn, c->xvector_dim);
    return LDS_OK;
}

}  // namespace

extern "C" int lds_xvector_create(const lds_xvector_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_xvector** out) {
    const char* fn = "lds_xvector_create";
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "%s: null argument", fn);
    if (int rc = xv_cfg_check(cfg)) return rc;
    lds_xvector* h = new lds_xvector();
    h->cfg = *cfg;
    WeightLoader W(h->own, n, names, ptrs, numel);
    const int C0 = cfg->tdnn_dim[0], CL = cfg->tdnn_dim[cfg->n_tdnn - 1], E = cfg->xvector_dim;
    h->proj_w = W.vec("projector.weight", (int64_t)C0 * cfg->d_in);
    h->proj_b = W.vec("projector.bias", C0);
    bool ok = h->proj_w && h->proj_b;
    for (int i = 0; i < cfg->n_tdnn; ++i) {
        const int Cin = i ? cfg->tdnn_dim[i - 1] : C0;
        const std::string p = "tdnn." + std::to_string(i) + ".kernel.";
        h->tdnn_w[i] = W.vec(p + "weight", (int64_t)cfg->tdnn_dim[i] * cfg->tdnn_kernel[i] * Cin);
        h->tdnn_b[i] = W.vec(p + "bias", cfg->tdnn_dim[i]);
        ok = ok && h->tdnn_w[i] && h->tdnn_b[i];
    }
    h->fe_w = W.vec("feature_extractor.weight", (int64_t)E * 2 * CL);
    h->fe_b = W.vec("feature_extractor.bias", E);
    int64_t nl = 0;      // the classifier's width is the checkpoint's
    h->cl_b = W.vec("classifier.bias", -1, &nl);
    h->cl_w = W.vec("classifier.weight", nl * E);
    h->n_labels = (int)nl;
    ok = ok && h->fe_w && h->fe_b && h->cl_b && h->cl_w;
    if (!ok && W.T.missing.empty()) {
        delete h;
        return set_error(LDS_ENOMEM, "%s: device allocation or upload failed", fn);
    }
    return W.finish(ok, fn, h, out, "xvector weight tensor");
}

extern "C" void lds_xvector_destroy(lds_xvector* h) { delete h; }

extern "C" int lds_xvector_n_labels(const lds_xvector* h) { return h ? h->n_labels : 0; }

extern "C" int lds_xvector_workspace_bytes(const lds_xvector* h, int B, int T, size_t* out) {
    const char* fn = "lds_xvector_workspace_bytes";
    if (!h || !out) return set_error(LDS_EINVAL, "%s: null argument", fn);
    if (int rc = xv_check_bt(fn, B, T)) return rc;
    *out = xv_plan(h, B, T).bytes;
    return LDS_OK;
}

extern "C" int lds_xvector_embed(lds_xvector* h, const float* X, const int32_t* n_frames, float* emb, float* logits, void* ws, size_t ws_bytes, int B, int T,
                                 void* stream) {
    const char* fn = "lds_xvector_embed";
    if (!h) return set_error(LDS_EINVAL, "%s: null handle", fn);
    if (int rc = xv_check_bt(fn, B, T)) return rc;
    lds::XvLens lens;
    if (int rc = xv_lens(fn, B, T, n_frames, lens)) return rc;
    const lds_xvector_cfg& c = h->cfg;
    const int span = xv_span(c);
    for (int b = 0; b < B; ++b)
        if (lens.v[b] - span < 2)
            return set_error(LDS_EINVAL, "%s: n_frames[%d] = %d gives %d pooled frames; the unbiased standard deviation needs 2, i.e. at least %d frames", fn, b,
                             lens.v[b], lens.v[b] - span > 0 ? lens.v[b] - span : 0, span + 2);
    if (!X || !emb || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const XvPlan p = xv_plan(h, B, T);
    if (ws_bytes < p.bytes) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    float *cur = (float*)(w + p.o_a), *nxt = (float*)(w + p.o_b);
    float2* part = (float2*)(w + p.o_part);
    float* stats = (float*)(w + p.o_stats);
    const int CL = c.tdnn_dim[c.n_tdnn - 1];
    xv_layer(X, h->proj_w, h->proj_b, c.d_in, c.tdnn_dim[0], 1, 1, 0, cur, nullptr, lens, s);
    for (int i = 0; i < c.n_tdnn; ++i) {
        const int Cin = i ? c.tdnn_dim[i - 1] : c.tdnn_dim[0];
        const bool last = i == c.n_tdnn - 1;
        xv_layer(cur, h->tdnn_w[i], h->tdnn_b[i], Cin, c.tdnn_dim[i], c.tdnn_kernel[i], c.tdnn_dilation[i], 1, nxt, last ? part : nullptr, lens, s);
        if (!last) {
            for (int b = 0; b < B; ++b) lens.v[b] -= (c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i];
            float* t = cur; cur = nxt; nxt = t;
        }
    }
    xv_join(part, stats, CL, (c.tdnn_kernel[c.n_tdnn - 1] - 1) * c.tdnn_dilation[c.n_tdnn - 1], lens, s);
    if (lds::launch_small_linear(h->fe_w, h->fe_b, stats, 2 * CL, lds::IN_PLAIN, nullptr, emb, c.xvector_dim, 0, c.xvector_dim, 2 * CL, B, s) != hipSuccess)
        return set_error(LDS_EHIP, "%s: the feature_extractor launch failed", fn);
    if (logits && lds::launch_small_linear(h->cl_w, h->cl_b, emb, c.xvector_dim, lds::IN_PLAIN, nullptr, logits, h->n_labels, 0, h->n_labels, c.xvector_dim, B, s) !=
                      hipSuccess)
        return set_error(LDS_EHIP, "%s: the classifier launch failed", fn);
    return launched(fn);
}

extern "C" int lds_xvector_cosine(const float* a, int N, const float* b, int M, int dim, float* out, void* stream) {
    const char* fn = "lds_xvector_cosine";
    if (N < 1 || N > 65535 || M < 1 || M > 65535) return set_error(LDS_EINVAL, "%s: N %d / M %d outside 1 .. 65535", fn, N, M);
    if (dim < 1 || dim > 65536) return set_error(LDS_EINVAL, "%s: dim %d outside 1 .. 65536", fn, dim);
    if (!a || !b || !out) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    hipLaunchKernelGGL(lds::xv_cosine_kernel, dim3(M, N), dim3(64), 0, (hipStream_t)stream, a, b, dim, M, out);
    return launched(fn);
}

extern "C" int lds_test_xvector_tdnn(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int Cin, int Cout, int ks, int dil,
                                     int relu, float* Y, void* stream) {
    const char* fn = "lds_test_xvector_tdnn";
    if (int rc = xv_check_bt(fn, B, T)) return rc;
    if (int rc = xv_check_layer(fn, Cin, Cout, ks, dil)) return rc;
    lds::XvLens lens;
    if (int rc = xv_lens(fn, B, T, n_frames, lens)) return rc;
    if (!X || !W || !bias || !Y) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    xv_layer(X, W, bias, Cin, Cout, ks, dil, relu ? 1 : 0, Y, nullptr, lens, (hipStream_t)stream);
    return launched(fn);
}

extern "C" int lds_test_xvector_pool_workspace_bytes(int B, int T, int Cout, size_t* out) {
    const char* fn = "lds_test_xvector_pool_workspace_bytes";
    if (!out) return set_error(LDS_EINVAL, "%s: null out", fn);
    if (int rc = xv_check_bt(fn, B, T)) return rc;
    if (Cout < 4 || Cout > 4096 || Cout % 4) return set_error(LDS_EINVAL, "%s: Cout %d must be a multiple of 4 in 4 .. 4096", fn, Cout);
    *out = Slots::round(xv_part_bytes(B, T, Cout));
    return LDS_OK;
}

extern "C" int lds_test_xvector_pool(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int Cin, int Cout, int ks, int dil,
                                     float* stats, float* Y, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "lds_test_xvector_pool";
    if (int rc = xv_check_bt(fn, B, T)) return rc;
    if (int rc = xv_check_layer(fn, Cin, Cout, ks, dil)) return rc;
    lds::XvLens lens;
    if (int rc = xv_lens(fn, B, T, n_frames, lens)) return rc;
    for (int b = 0; b < B; ++b)
        if (lens.v[b] - (ks - 1) * dil < 2)
            return set_error(LDS_EINVAL, "%s: n_frames[%d] = %d gives %d pooled frames; the unbiased standard deviation needs 2", fn, b, lens.v[b],
                             lens.v[b] - (ks - 1) * dil > 0 ? lens.v[b] - (ks - 1) * dil : 0);
    if (!X || !W || !bias || !stats || !ws) return set_error(LDS_EINVAL, "%s: null pointer", fn);
    const size_t need = Slots::round(xv_part_bytes(B, T, Cout));
    if (ws_bytes < need) return set_error(LDS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    xv_layer(X, W, bias, Cin, Cout, ks, dil, 1, nullptr, (float2*)ws, lens, s);
    xv_join((const float2*)ws, stats, Cout, (ks - 1) * dil, lens, s);
    if (Y) xv_layer(X, W, bias, Cin, Cout, ks, dil, 1, Y, nullptr, lens, s);
    return launched(fn);
}
