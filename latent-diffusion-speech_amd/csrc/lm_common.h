// What the two language models share (lm.hip: RoFormer, llama.hip: Llama): the wave64 / workgroup reductions of their kernels and the
// launchers of the token-choice kernels, which live in lm.hip and serve both decodes.
#pragma once
#include "../../include/lds.h"
#include "kernels.h"

namespace lds {

// Wave64 reductions on the DPP path (row shifts + row broadcasts: VALU speed, no LDS crossbar), result in every lane.  A butterfly of
// __shfl_xor is six dependent ds_bpermute round trips (~0.3 us); the decode step runs ~40 of these reductions back to back.
template <int CTRL, int ROW_MASK, bool BOUND>
static __device__ __forceinline__ int dpp_i(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, BOUND); }
template <int CTRL, int ROW_MASK, bool BOUND>
static __device__ __forceinline__ float dpp_f(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
static __device__ __forceinline__ float wave_sum(float v) {      // fixed order; the total forms in lane 63
    v += dpp_f<0x111, 0xf, true>(0.f, v);      // row_shr:1
    v += dpp_f<0x112, 0xf, true>(0.f, v);      // row_shr:2
    v += dpp_f<0x114, 0xf, true>(0.f, v);      // row_shr:4
    v += dpp_f<0x118, 0xf, true>(0.f, v);      // row_shr:8: lane 15 of every 16-lane row = the row's sum
    v += dpp_f<0x142, 0xa, false>(0.f, v);     // row_bcast:15 into rows 1 and 3
    v += dpp_f<0x143, 0xc, false>(0.f, v);     // row_bcast:31 into rows 2 and 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
static __device__ __forceinline__ float wave_max(float v) {      // lanes without a source keep their own value (old = v)
    v = fmaxf(v, dpp_f<0x111, 0xf, false>(v, v));
    v = fmaxf(v, dpp_f<0x112, 0xf, false>(v, v));
    v = fmaxf(v, dpp_f<0x114, 0xf, false>(v, v));
    v = fmaxf(v, dpp_f<0x118, 0xf, false>(v, v));
    v = fmaxf(v, dpp_f<0x142, 0xa, false>(v, v));
    v = fmaxf(v, dpp_f<0x143, 0xc, false>(v, v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
static __device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, dpp_i<0x111, 0xf, false>(v, v));
    v = min(v, dpp_i<0x112, 0xf, false>(v, v));
    v = min(v, dpp_i<0x114, 0xf, false>(v, v));
    v = min(v, dpp_i<0x118, 0xf, false>(v, v));
    v = min(v, dpp_i<0x142, 0xa, false>(v, v));
    v = min(v, dpp_i<0x143, 0xc, false>(v, v));
    return __builtin_amdgcn_readlane(v, 63);
}
// sum over the NT threads of a workgroup (fixed order), result in every thread; red has NT / 64 <= 16 slots
template <int NT>
static __device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}
static __device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// ---- lm.hip's token choice (greedy, top-k 1..64 with ties, no filter, top-p, repetition penalty, n-gram ban) with per-row positions: row b
//      continues a history of plen[b] tokens in tokens [B][cap] and writes slot plen[b] + step (lm_sample_body's PROW form).  word .. eb / xnext:
//      the RoFormer's next input row, null to skip it. ----
hipError_t lm_launch_choice_rows(const lds_lm_decode_opts& o, int B, int V, const float* lg, float inv_temp, const float* u, int64_t* tokens, int cap, int step,
                                 int* unfinished, int eos, int pad, int* any_unf, const float* word, const float* type, const float* eg, const float* eb, float eps,
                                 int H, float* xnext, const int32_t* plen, int* rowlen, hipStream_t st);
// ---- lm.hip's teacher-forced row statistics (lds_lm_score's definitions; lds_llama_score counts over its whole vocabulary with them).
//      lm_launch_score_rows: `rows` logits rows [rows][V], the first being row n0 = b * T + t of the batch -> lp / rank [B][T-1] at the counted
//      positions (t + 1 < len[b], labels[b][t + 1] in [0, V)), 0 / -1 elsewhere.  lm_launch_score_loss: the fixed-order double sum over the
//      counted positions -> loss [1] = -sum / n, n_counted [1]; psum [B] doubles and pcnt [B] ints are scratch. ----
hipError_t lm_launch_score_rows(const float* logits, long long n0, int rows, int V, int T, const int64_t* labels, const int32_t* len, float* lp, int32_t* rank,
                                hipStream_t st);
hipError_t lm_launch_score_loss(const float* lp, const int32_t* rank, int B, int T1, double* psum, int32_t* pcnt, float* loss, int32_t* n_counted, hipStream_t st);
// ---- lm.hip's beam-search step (lm_beam_step_kernel: one step of HF's _beam_search per batch item), its state, and its per-row form for a decode
//      whose items continue prompts of their own lengths (the Llama's: lm_beam_step_kernel<NW, true>) ----
constexpr int kMaxBeams = 8, kMaxBeamVocab = 64 * 68;
struct LmBeamState {
    const int64_t* rseq_in; int64_t* rseq_out;      // running sequences [B * K][cap]
    const float* rscore_in; float* rscore_out;      // running scores [B * K]
    const int* tab_in; int* tab_out;                // [B * K][cap]: cache row of key p of each running beam (null: not tracked)
    const int64_t* fseq_in; int64_t* fseq_out;      // finished hypotheses [B * K][cap]
    const float* fscore_in; float* fscore_out;      // [B * K]
    const int* ffin_in; int* ffin_out;              // is_sent_finished [B * K]
    const int* flen_in; int* flen_out;              // generated tokens of each hypothesis (the prompt / BOS not counted) [B * K]
    const int* unsat_in; int* unsat_out;            // is_early_stop_heuristic_unsatisfied [B]
    int* parent;                                    // [B * K] parent beam of each new running beam, or null
    const int* prev_flag; int* flag_out;
};
// The per-row form.  plen [B]: every item's decoder_prompt_len; the item is at cur_len = plen[b] + step.  first_free: ids below it are banned
// (-inf) after the n-gram ban.  ended_in / ended_out [B] (may alias): 1 once the item's own loop condition has turned false; such an item's
// state goes through unchanged and it adds nothing to the flag bits, whose bit 16 says that some item still runs after the step.  The step that
// finds 1 copies the state into the other buffers and writes 2; one that finds 2 touches nothing of the item's (both buffers already agree).  The
// ancestry table is [B * K][tcap] over generated positions only: entry e is the cache row of the key at position plen[b] + e.
struct LmBeamRows { const int32_t* plen; int first_free; const int* ended_in; int* ended_out; int tcap; };
hipError_t lm_launch_beam_rows(int B, int K, int V, const float* lg, int step, int cap, int max_length, int eos, float pen, int ngram, int es,
                               const LmBeamState& bs, const LmBeamRows& rw, hipStream_t st);
// the option checks that need no model (no device call); LDS_OK or LDS_EINVAL with a message
int lm_check_opts(const lds_lm_decode_opts& o, const float* logits_out);
constexpr int kLmMaxTopK = 64;            // survivors of the top-k filter
constexpr int kLmMaxChoiceVocab = 8192;   // columns the token-choice kernels take (32 per thread; the n-gram ban's bit set)

}  // namespace lds
