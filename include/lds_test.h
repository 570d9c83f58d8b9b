/*
 * liblds.so -- single-op test and micro-benchmark entry points.  NOT part of the drop-in boundary (include/lds.h): they exist so
 * that tests/ can check each kernel alone against the oracle and tools/ can time one launch.  Every call here allocates its own
 * temporaries and synchronises the stream before returning.
 */
#ifndef LDS_TEST_H
#define LDS_TEST_H

#include "lds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- single-op entry points (used by the parity tests to check each kernel alone) ----------- */
typedef struct {                        /* the generic convolution (vocoder / front end path, conv_gemm)   */
    const float* x1; const float* x2;   /* dev inputs [B,C1,Tsrc], [B,C2,Tsrc] (x2 may be NULL)  */
    int C1, C2, Tsrc;
    const float* w;                     /* host, reference layout [Co, C1+C2, K]                  */
    const float* bias;                  /* host [Co] or NULL                                      */
    int Co, K, pad, dil;
    int act_in;                         /* 0 none, 2 LeakyReLU(slope) on the input                */
    float slope;
    const float* res;                   /* dev [B,Co,To] or NULL                                  */
    int epilogue;                       /* 0 none, 2 tanh                                         */
    int tile;                           /* 0 auto, else BM*1000+BN                                */
} lds_conv_test;
int lds_test_conv(const lds_conv_test* a, float* out, int B, void* stream);
/* ---- the UNet's K4P path, one op at a time (plain tensors in/out; layout conversion happens on the device) ---- */
typedef struct {
    const float* x1; const float* x2;   /* dev inputs [B,C1,T], [B,C2,T] (x2 may be NULL)                 */
    int C1, C2, T;
    const float* w; const float* bias;  /* host, reference layout [Co, C1+C2, K] / [Co]                   */
    int Co, K, stride, pad, ups;
    const float* res;                   /* dev [B,Cout,To] or NULL                                        */
    int epilogue;                       /* 0 none, 1 GEGLU                                                */
    int plain_out;                      /* 1: the kernel writes frame-major output directly               */
    int v_split;                        /* QKV: last third of the channels frame-major (1) or in attention's VT layout with head dim v_split (> 1) */
    int cfg;                            /* 0 auto, else BM*1000000 + BN*1000 + BK*10 + NST                */
} lds_dconv_test;
int lds_test_dconv(const lds_dconv_test* a, float* out, float* lnpart, int B, void* stream);
int lds_bench_dconv(const lds_dconv_test* a, float* out, int B, int iters, float* ms_out, char* cfg_out, size_t cfg_cap,
                    void* stream);
int lds_test_gn_apply(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                      const float* beta, const float* scale_shift, int silu, float* out, int B, void* stream);
/* average time of one streaming-GroupNorm launch on zero-filled tensors (tools/bench_gn.py) */
int lds_bench_gn_stream(int C1, int C2, int T, int B, int iters, float* ms_out, void* stream);
/* conv 1x1 (C -> Cm, GroupNorm partials from its epilogue) -> proj(GroupNorm(mid)) (Cm -> Co) as ONE launch with the normalisation folded into the
 * projection (csrc/kernels.h DmaConvArgs::gnf_part); tile_batch > 0: the latency mode's tile / cluster-split choices at that batch */
int lds_test_gn_fold_k4p(const float* x, const float* w1, const float* bias1, const float* gamma, const float* beta, float eps, int groups,
                         const float* w2, const float* bias2, float* mid, float* out, int B, int C, int Cm, int Co, int T, int cfg, int tile_batch,
                         void* stream);
/* the same through either kernel family (fmt -1 = exact fp32 K4P, 0 = three bf16 planes, 1 = two fp16 planes); the folded launch runs `reps` times
 * on the same inputs into out[rep][B][Co][T]: every repetition must equal the first bit for bit, also when workgroups share a CU */
int lds_test_gn_fold_split(const float* x, const float* w1, const float* bias1, const float* gamma, const float* beta, float eps, int groups,
                           const float* w2, const float* bias2, float* mid, float* out, int B, int C, int Cm, int Co, int T, int cfg, int tile_batch,
                           int fmt, int reps, void* stream);
/* the latency mode's cluster split-K hand-off (csrc/conv_dma.hip cluster_join): a K-tap (1 / 3) convolution Ci -> Co with the tile and cluster choices at
 * tile_batch = B, launched `reps` times back to back alternating between the inputs xa / xb (a stale partial is then the other input's) into
 * out[rep][B][Co][T]; ref_a / ref_b = the same tile shapes with one workgroup per tile; fmt -1 exact fp32, 0 / 1 split planes; cfg_out = the cluster
 * launch's configuration ("... KS<S> ...": S workgroups per tile) */
int lds_test_cluster_join(const float* xa, const float* xb, const float* w, const float* bias, int Ci, int Co, int K, int T, int B, int fmt, int reps,
                          float* out, float* ref_a, float* ref_b, char* cfg_out, size_t cfg_cap, void* stream);
/* mid = conv1x1(x) (+bias) written together with the epilogue's GroupNorm partial statistics; out = GroupNorm(mid)(+SiLU) by the
 * streaming pass that combines those partials -- the statistics path of the UNet (cfg: conv_dma tile code, 0 = auto) */
int lds_test_gn_chain_k4p(const float* x, const float* w1, const float* bias1, const float* gamma, const float* beta, float eps,
                          int groups, int silu, float* mid, float* out, int B, int C, int Co, int T, int cfg, void* stream);
int lds_test_ln_chain_k4p(const float* x, const float* w1, const float* w2, const float* gamma, const float* beta,
                          float eps, float* mid, float* out, int B, int C, int Co, int T, void* stream);
/* one residual step of a vocoder ResBlock1 on the K4P / LDS-DMA path: out = c2(lrelu(c1(lrelu(x)))) + x (reference models.py:186-192);
 * mode 0 plain output, 1 raw + LeakyReLU'd K4P outputs (returned plain in out / out_act), 2 running sum out = (acc + y) / div */
int lds_test_voc_step(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int C, int T, int K, int dil, int mode,
                      const float* acc, float div, float* out, float* out_act, int B, void* stream);
/* qkv dev [B,3C,T] -> out dev [B,C,T]; softmax(QK^T/sqrt(C/heads))V per head */
int lds_test_attention_k4p(const float* qkv, float* out, int B, int C, int T, int heads, void* stream);
/* the same with both products on the fp16 matrix pipe, operands split in registers into two fp16 terms (the split-fp16 GEMM mode's attention) */
int lds_test_attention_f16math(const float* qkv, float* out, int B, int C, int T, int heads, void* stream);
/* the latency mode's configuration choice (judged at the actual batch: 32-query workgroups whose four waves share the keys); f16math 0 / 1 */
int lds_test_attention_latency(const float* qkv, float* out, int B, int C, int T, int heads, int f16math, void* stream);
/* the same three on a ragged batch: lens = HOST int32 [B], 1 <= lens[b] <= T.  q and k reach the kernel as given (the caller may fill the frames
 * beyond a clip's length with NaN); v is zeroed there, as the QKV convolution writes it; the K4P output buffer starts as NaN.  out [B,C,T]:
 * frames at and beyond lens[b] are zeros.  f16math 0 / 1; latency 1 = the latency mode's configuration choice */
int lds_test_attention_ragged(const float* qkv, const int* lens, float* out, int B, int C, int T, int heads, int f16math, int latency, void* stream);
int lds_test_conv_transpose(const float* x, const float* w /*host [Ci,Co,K]*/, const float* bias,
                            float* out, int B, int Ci, int Co, int T, int K, int stride, int pad,
                            float in_slope, void* stream);

/* the same single-op entry as lds_test_dconv / lds_bench_dconv through the split-bf16 kernel (conv_bf3.hip): plain tensors are
 * converted to K8B3 on the device; nprod = bf16 products per fp32 product (6 = the product path; 3 and 9 exist for the error study
 * of tools/split_bf16_probe.py on the 128 x 128 x BK32 1x1 tile only) */
int lds_test_dconv_bf3(const lds_dconv_test* a, float* out, float* lnpart, int B, int nprod, void* stream);
int lds_bench_dconv_bf3(const lds_dconv_test* a, float* out, int B, int iters, int nprod, float* ms_out, char* cfg_out, size_t cfg_cap,
                        void* stream);
/* lds_bench_dconv with consecutive launches rotating through the tile configurations cfgs[0 .. n): the cost of running code the previous
 * launch did not run (tools/bench_icache.py) */
int lds_bench_dconv_alt(const lds_dconv_test* a, float* out, int B, int iters, const int* cfgs, int n, float* ms_out, void* stream);
/* the same through either split-plane format: fmt 0 = three bf16 planes, 1 = two fp16 planes (csrc/k8b3.h); nprod 0 = the format's default */
int lds_test_dconv_split(const lds_dconv_test* a, float* out, float* lnpart, int B, int nprod, int fmt, void* stream);
int lds_bench_dconv_split(const lds_dconv_test* a, float* out, int B, int iters, int nprod, int fmt, float* ms_out, char* cfg_out, size_t cfg_cap,
                          void* stream);
int lds_test_split_roundtrip(const float* x, float* out, int B, int C, int T, int fmt, void* stream);
int lds_test_gn_apply_split(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                            const float* beta, const float* scale_shift, int silu, float* out, int B, int fmt, void* stream);
/* tuning only (tools/tune_split_rules.py): bit mask of alternative tile rules of the split-GEMM launcher, 0 = the shipped rules */
/* 0: the transformer blocks' GroupNorm runs as its own pass instead of folded into proj_in (A/B measurements and tests); default 1 */
int lds_debug_set_gn_fold(int on);
/* the narrow vocoder stages' residual steps: 1 (default) = one fused launch per step (csrc/voc_pair.hip), 0 = two convolution launches */
int lds_debug_set_voc_pair(int on);
/* experiment: 1 = a convolution's weights are read (one dword per 64-byte line) by a small launch immediately before the convolution's own:
 * the upper bound of what a weight prefetcher could give (tools/touch_weights_probe.py) */
int lds_debug_set_touch_weights(int on);
/* one residual step of ResBlock1 at 16 / 32 channels through the fused kernel: out = (acc ? acc : 0) + c2(lrelu(c1(lrelu(x)))) + x, / div
 * (reference models.py:186-192, 250-259); x, acc, out dev [B][C][T], weights host [C][C][K]; lengths host int32 [B] or null */
int lds_test_voc_pair(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int C, int T, int K, int dil,
                      const float* acc, float div, const int32_t* lengths, float* out, int B, void* stream);
/* the VAE encoder's convolution alone (csrc/conv_down.hip; reference models.py:24-29,39-54 Conv1d with stride): x dev [B][Ci][T], w host
 * [Co][Ci][K], b host [Co] or NULL, out dev [B][Co][To]; pad = (K - stride + 1) / 2, To = (T + 2 pad - K) / stride + 1; LeakyReLU(slope) on
 * the input (slope 1 = none); T a multiple of stride.  tile: 0 = the product path's choice (workgroups against the device's CU count), else
 * BM*1000+BN in {64064, 64128, 128128}; cfg_out (or NULL) receives the configuration that ran ("BM128 BN128 grid ...").  Synchronises. */
int lds_test_conv_down(const float* x, const float* w, const float* b, int Ci, int Co, int K, int stride, int T, int B, float slope,
                       int tile, float* out, char* cfg_out, size_t cfg_cap, void* stream);
/* ... in a ragged batch: lengths_in / lengths_out host int32 [B] (B <= 64) = every element's valid input frames (0 .. T; x reads as zeros
 * from there on, whatever it holds) and output frames (0 .. To; out is stored as zeros from there on) */
int lds_test_conv_down_ragged(const float* x, const float* w, const float* b, int Ci, int Co, int K, int stride, int T, int B, float slope,
                              const int32_t* lengths_in, const int32_t* lengths_out, int tile, float* out, char* cfg_out, size_t cfg_cap,
                              void* stream);
int lds_debug_set_split_rule(int rule);
/* host only (no device is touched): conv_dma's block-index decomposition without a division (csrc/kernels.h dma_magic).
 * lds_test_dma_magic_div: out[n] = n / d for n in [0, n_count) through the launchers' multiplier / shift pair.
 * lds_test_dma_tile_order: out[id][4] = (M-block, frame block, batch element, cluster share) of every workgroup id of a grid of
 * nMb * nN * B * S workgroups, with the constants the launchers pass and the arithmetic the kernel runs. */
int lds_test_dma_magic_div(uint32_t d, uint32_t n_count, uint32_t* out);
int lds_test_dma_tile_order(int nMb, int nN, int B, int S, int32_t* out);
/* Arm a tap on the calling thread: the next call of lds_test_dconv (fp32, K4P output), lds_test_dconv_ex / lds_test_dconv_pair (fmt -1),
 * lds_test_ln_chain_k4p (its `out` tensor) or lds_test_attention_k4p / _f16math / _latency fills the K4P buffer its kernel writes with NaN
 * before the launch and copies it to dst afterwards, as the kernel left it: dev [B][C/8][2][T + 2][4] (csrc/k4p.h), entry 0 and entry T + 1
 * of every row being the pad frames.  floats must be B * C * (T + 2) of that output (an error otherwise); the tap is then disarmed.
 * dst NULL, floats 0: disarm. */
int lds_test_tap_k4p(float* dst, size_t floats);

/* ---- conv_dma / conv_bf3 modes that the product reaches through whole models only (tests/test_gpu_conv_modes.py) ----
 * Common to the three entries: fmt -1 = exact fp32 (K4P, conv_dma), 0 = three bf16 planes, 1 = two fp16 planes (conv_bf3), as lds_test_gn_fold_split;
 * tile_batch as there (0 = the tile rules at the nominal batch, > 0 = the latency mode's choices at that batch, cluster split-K included); cfg_out
 * (or NULL) receives the configuration string of the launch under test.  lengths (host int32 [B], B <= 64, or NULL = dense) are the per-utterance
 * lengths of a ragged batch (csrc/k4p.h ragged_len): the INPUT tensors must hold zeros at and beyond an utterance's frames at their level, as every
 * tensor of a ragged batch does; the entry does not mask them.  Output buffers are filled with NaN patterns before the launch. */
/* the fused resnet tail (csrc/kernels.h launch_conv_dma_pair / launch_conv_bf3_pair): out [B][Co][T] = conv_k3(h [B][Cm][T]; w3 [Co][Cm][3], pad 1)
 * + conv_1x1([x1 ; x2] [B][C1 + C2][T]; w1 [Co][C1 + C2][1]) + b3 + b1 (x2 NULL when C2 = 0; weights and biases host), gnpart [B][Co/16][ceil(T/32)][2]
 * = the epilogue's GroupNorm partials (mean, M2) over each block's valid frames; lvl = the level of all tensors.  Shapes without a fused variant are an
 * error: the two-launch fallback of the resnet driver is never run here. */
int lds_test_dconv_pair(const float* h, const float* x1, const float* x2, const float* w3, const float* b3, const float* w1, const float* b1, int B,
                        int Cm, int C1, int C2, int Co, int T, const int32_t* lengths, int lvl, int tile_batch, int fmt, float* out, float* gnpart,
                        char* cfg_out, size_t cfg_cap, void* stream);
typedef struct {                        /* lds_dconv_test with the encoders' epilogue and geometries and the ragged drivers' lengths */
    const float* x1; const float* x2;   /* dev inputs [B,C1,T], [B,C2,T] (x2 NULL when C2 = 0)                                      */
    int C1, C2, T;
    const float* w; const float* bias;  /* host, reference layout [Co, C1+C2, K] / [Co] (or NULL)                                   */
    int Co, K, stride, pad;             /* To = (T + 2 pad - K) / stride + 1                                                        */
    const float* res;                   /* dev [B,Co,To] or NULL                                                                    */
    int epilogue;                       /* 0 none, 3 exact-form GELU of the biased / normalised value, before the residual          */
    const int32_t* lengths;             /* host [B] or NULL; the input is at level lvl_in of them, the output at lvl_out            */
    int lvl_in, lvl_out;
    const float* ln_gamma; const float* ln_beta;      /* host [C1], both or neither: LayerNorm over the channels of x1 folded into the (1x1) convolution;   */
    float ln_eps;                       /* its per-frame partials come from the epilogue of an identity convolution the entry runs  */
    int tile_batch, fmt;
    int v_split;                        /* 0, or > 1 (fp32, 1x1): the QKV projection -- the last third of the rows in attention's VT layout, head dim v_split */
    int cfg;                            /* 0 auto, else BM*1000000 + BN*1000 + BK*10 + NST                                           */
} lds_dconv_ex_test;
/* epilogue 1 (GEGLU; fp32 with the LayerNorm fold only): the transformer's FF1, Co = 2 x the output channels, out dev [B][Co/2][To].
 * out dev [B][Co][To] (v_split: [B][2 Co/3][To] followed by the raw VT buffer [B][Co/3/D][ceil4(To)/4][D][4]); gnpart dev [B][Co/16][ceil(To/32)][2] or NULL */
int lds_test_dconv_ex(const lds_dconv_ex_test* a, float* out, float* gnpart, int B, char* cfg_out, size_t cfg_cap, void* stream);
/* one vocoder upsampler on conv_dma as the generator runs it: x dev [B][Ci][T] -> LeakyReLU(0.1) K4P copy with its pad frames zeroed -> polyphase
 * ConvTranspose1d(K = 2 stride, stride, padding (K - stride + 1) / 2; w host [Ci][Co][K], bias host [Co] or NULL) -> out (raw) and out_act
 * (LeakyReLU(0.1) of it), both dev [B][Co][(T - 1) stride - 2 padding + K].  lengths_in / lengths_out (host int32 [B], both or neither): x is not read at
 * and beyond lengths_in[b] frames (it counts as zeros there, whatever it holds) and both outputs are zeros at and beyond lengths_out[b]. */
int lds_test_voc_ups(const float* x, const float* w, const float* bias, int B, int Ci, int Co, int T, int K, int stride, const int32_t* lengths_in,
                     const int32_t* lengths_out, float* out, float* out_act, char* cfg_out, size_t cfg_cap, void* stream);
/* plain [B,C,T] -> K8B3 -> plain: must return the input bit for bit (the three-term split is lossless) */
int lds_test_k8b3_roundtrip(const float* x, float* out, int B, int C, int T, void* stream);
/* GroupNorm(+scale/shift)(+SiLU) through the K8B3 streaming pass (statistics from gn_partials_bf3) */
int lds_test_gn_apply_bf3(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                          const float* beta, const float* scale_shift, int silu, float* out, int B, void* stream);

/* ONE token choice per row of logits [B][V] (dev) with the kernels of lds_lm_generate, after a history hist [B][n_hist] int64 (dev; what the repetition
 * penalty looks at); uniforms [B] (dev); out [B] int64 (dev).  top_k 0 = no top-k filter (HF: None / 0), else 1 .. 64 with ties of the k-th kept. */
int lds_test_lm_sample(const float* logits, int B, int V, int do_sample, int top_k, float top_p, float temperature, float repetition_penalty,
                       const float* uniforms, const int64_t* hist, int n_hist, int64_t* out, void* stream);
/* ONE step of lds_lm_generate_opts' beam search on logits [B * K][V] (dev) and the state of HF's _beam_search (all dev): running sequences
 * [B * K][max_length] int64 (the first cur_len ids are the history) and scores [B * K]; finished hypotheses [B * K][max_length], scores,
 * is_sent_finished flags and generated lengths [B * K]; is_early_stop_heuristic_unsatisfied [B].  Writes the same state after the step,
 * parent_out [B * K] (parent beam 0 .. K - 1 of every new running beam) and flag_out [1] (1: some item may improve, 2: some item has an
 * unfinished hypothesis slot, 4: some candidate did not hit the stopping criteria).  2 K <= V <= 4352, 1 <= cur_len < max_length. */
int lds_test_lm_beam_step(const float* logits, int B, int K, int V, int cur_len, int max_length, int eos, float repetition_penalty,
                          int no_repeat_ngram_size, int early_stopping, const int64_t* run_seq, const float* run_score, const int64_t* fin_seq,
                          const float* fin_score, const int32_t* fin_flag, const int32_t* fin_len, const int32_t* unsat, int64_t* run_seq_out,
                          float* run_score_out, int32_t* parent_out, int64_t* fin_seq_out, float* fin_score_out, int32_t* fin_flag_out,
                          int32_t* fin_len_out, int32_t* unsat_out, int32_t* flag_out, void* stream);
/* ONE step of lds_llama_generate_beam's beam search: lds_test_lm_beam_step with per-item prompts.  Item b continues a prompt of prompt_len[b]
 * ids (HOST int32 [B]) and is at cur_len = prompt_len[b] + step: its histories are the first cur_len ids of its running sequences, and fin_len
 * counts generated tokens.  Ids below first_free_id are banned after the n-gram ban.  ended (HOST int32 [B]): an item whose own loop has ended
 * comes back unchanged (parent_out = 0 .. K - 1) and adds nothing to flag_out; ended_out dev int32 [B] = 2 for it (its state now stands in both
 * buffers; an item handed in with 2 is not touched at all) and 1 for every item whose loop ends with this step.  flag_out [1]: the bits of lds_test_lm_beam_step over the items that ran, plus 16 = some item still runs.
 * vocab <= 4352, V - first_free_id >= 2 K, prompt_len[b] + step < max_length for every item that runs. */
int lds_test_llama_beam_step(const float* logits, int B, int K, int V, int step, int max_length, int eos, float repetition_penalty,
                             int no_repeat_ngram_size, int early_stopping, int first_free_id, const int32_t* prompt_len, const int32_t* ended,
                             const int64_t* run_seq, const float* run_score, const int64_t* fin_seq, const float* fin_score, const int32_t* fin_flag,
                             const int32_t* fin_len, const int32_t* unsat, int64_t* run_seq_out, float* run_score_out, int32_t* parent_out,
                             int64_t* fin_seq_out, float* fin_score_out, int32_t* fin_flag_out, int32_t* fin_len_out, int32_t* unsat_out,
                             int32_t* ended_out, int32_t* flag_out, void* stream);
/* ONE attention call of the Llama decode at step `step`: q, out dev [R][heads * d]; kc, vc dev [R][kv_heads][cap][d]; row n of item n / K is at
 * position prompt_len[n / K] - 1 + step (prompt_len HOST int32 [R / K]).  tab dev int32 [R][tcap]: the beam attention -- key p of row n comes
 * from cache row (n / K) * K for p < prompt_len, from row n for the last key, from tab[n][p - prompt_len] otherwise.  tab NULL (K = 1): the
 * plain attention of lds_llama_generate, every row on its own cache row. */
int lds_test_llama_beam_attn(const float* q, const float* kc, const float* vc, const int32_t* tab, const int32_t* prompt_len, int R, int K, int heads,
                             int kv_heads, int d, int cap, int tcap, int step, float* out, void* stream);
/* lds_llama_generate_beam with `poll` steps (>= 1) between two polls of the flag bits in place of its own 8: the result must not depend on it. */
int lds_test_llama_generate_beam_poll(lds_llama* h, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length,
                                      const lds_lm_decode_opts* opts, int64_t* tokens, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream, int poll);

/* The wav2vec 2.0 encoder's own kernels alone (csrc/w2v.hip); every pointer but the lengths is a device pointer.
 * w2v_conv0: audio [B][L] -> out [B][C][N0], N0 = (L - 10) / 5 + 1: GELU(LayerNorm over the C channels of each frame(bias + conv0(clip)));
 * w [C][10]; lengths (host int32 [B] or NULL): the clips' sample counts (10 .. L), frames at and beyond (lengths[b] - 10) / 5 + 1 are zeros.
 * w2v_ln_act: x [B][C][T] -> out [B][C][T] = GELU(LayerNorm over the channels); n_frames (host int32 [B] or NULL): zeros at and beyond;
 * part (or NULL) [B][C / 32][T][2] = (mean, M2) of every 32 channels of out.  C a multiple of 64 up to 1024, B <= 64. */
int lds_test_w2v_conv0(const float* audio, const int32_t* lengths, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                       float* out, int B, int C, int64_t L, void* stream);
int lds_test_w2v_ln_act(const float* x, const int32_t* n_frames, const float* gamma, const float* beta, float eps, float* out, float* part, int B, int C,
                        int T, void* stream);

/* The w2v-BERT 2.0 encoder's own kernels alone (csrc/w2vbert.hip, csrc/attention_k4p.hip); every pointer but the row / sample counts is a
 * device pointer, B <= 64.
 * w2vbert_fbank: audio [B][L] -> out [B][R][160] = SeamlessM4TFeatureExtractor's input_features (80 mel bins, stride 2), R = the rows of L samples;
 *   lengths (host int32 [B] or NULL): the clips' sample counts (560 .. L), zeros beyond a clip's rows.
 * w2vbert_attention: qkv [B][3C][T] (q, k, v; heads of 64), E [left + right + 1][64] -> out [B][C][T] = softmax((q.k + q.E[clamp(j - i, -left, right)
 *   + left]) / 8) v; q_rows / k_rows (host int32 [B], both or neither): the clip's queries (zeros beyond) and keys, 1 <= k_rows[b] <= q_rows[b] <= T.
 *   q and k may hold anything at and beyond q_rows[b]; v must be finite there (in the encoder its producer writes zeros).
 * w2vbert_dwconv: x [B][C][T], w [C][K] -> out [B][C][T] = swish(LayerNorm over the channels(sum_k w[c][k] x[c][t - (K - 1) + k])); in_rows / out_rows
 *   (host int32 [B], both or neither): input frames at and beyond in_rows[b] read as zeros, output frames at and beyond out_rows[b] are zeros,
 *   1 <= in_rows[b] <= out_rows[b] <= T.  C a multiple of 64 up to 1024, K <= 31. */
int lds_test_w2vbert_fbank(const float* audio, const int32_t* lengths, float* out, int B, int64_t L, void* stream);
int lds_test_w2vbert_attention(const float* qkv, const float* E, const int32_t* q_rows, const int32_t* k_rows, float* out, int B, int C, int T, int heads,
                               int left, int right, void* stream);
int lds_test_w2vbert_dwconv(const float* x, const float* w, const float* gamma, const float* beta, float eps, const int32_t* in_rows, const int32_t* out_rows,
                            float* out, int B, int C, int T, int K, void* stream);

/* The WavLM encoder's gated-bias attention alone (csrc/attention_k4p.hip attention_k4p_bias); every pointer but `lengths` is a device
 * pointer, B <= 64, T <= n_ctx <= 1500.  qkv [B][3C][T] (q, k, v; heads of 64), gate [B][heads][T], toep [heads][2 n_ctx - 1] (the bias of distance
 * d = key - query at index d + n_ctx - 1) -> out [B][C][T] = softmax(q.k / 8 + gate[i] toep[j - i]) v; lengths (host int32 [B] or NULL): the
 * clip's queries (zeros beyond) and keys, 1 <= lengths[b] <= T.  q, k, v and gate may hold anything at and beyond lengths[b] (the entry zeroes
 * the value rows there, as the encoder's q | k | v convolution writes them).  Synchronises.
 * wavlm_buckets (host only, no device): out host int32 [2 n - 1] = WavLMAttention._relative_positions_bucket of the distances -(n - 1) .. n - 1,
 * the table lds_wavlm_create builds its bias from. */
int lds_test_wavlm_attention(const float* qkv, const float* gate, const float* toep, const int32_t* lengths, float* out, int B, int C, int T, int heads,
                             int n_ctx, void* stream);
int lds_test_wavlm_buckets(int num_buckets, int max_distance, int n, int32_t* out);

/* csrc/stftmel.hip's framed DFT alone: the frames of audio [B][L] as they are (no padding; F = 1 + (L - n_fft_new) / hop_new rows) times
 * basis [n_fft_new][n_fft_new / 2 + 1][2] -> dft dev double [B][F][n_fft_new / 2 + 1][2], the raw sums before the magnitude (an integer-valued
 * asymmetric basis makes them exact: a swapped row / column of the f64 MFMA's C/D map shows); out dev [B][F][n_mels] as lds_stft_mel.  Synchronises. */
int lds_test_stft_dft(const float* audio, const double* basis, const float* mel_basisT, int n_fft_new, int hop_new, int n_mels, int F, float* out,
                      double* dft, int B, int64_t L, void* stream);

/* lds_knn_search (include/lds.h, csrc/knn.hip) with the pool's cut forced by the caller, so that the slab and split paths run at toy sizes:
 * slab_rows (a multiple of 128 that one buffer descriptor holds) pool rows per descriptor, `splits` (1 .. 64) ranges of 128-row pool blocks,
 * each walked by its own workgroups.  The workspace holds min(splits, pool blocks) * N * (k rounded up to 1, 2, 4, 8) * 8 bytes or more
 * (each of the two halves rounded up to 256); LDS_ENOMEM below that. */
int lds_test_knn_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int slab_rows, int splits, int32_t* idx,
                        float* score, void* ws, size_t ws_bytes, void* stream);
/* the same probe of lds_knn_search_metric (replaces nothing in the reference: a test entry) */
int lds_test_knn_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int metric, int slab_rows, int splits,
                               int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream);

/* lds_ivf_search (include/lds.h) with the list-ordered copy cut into slabs of slab_rows rows (a multiple of 128 that one buffer descriptor
 * holds), so that lists in different slabs are walked at toy sizes.  The workspace is lds_ivf_workspace_bytes'. */
int lds_test_ivf_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, const float* C, const float* hc, int nlist,
                        const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe, int slab_rows,
                        int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream);
/* the same probe of lds_ivf_search_metric */
int lds_test_ivf_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, const float* C, const float* hc, int nlist,
                               const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe, int metric,
                               int slab_rows, int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream);

/* The two CTC recursions of csrc/ctc.hip on ready emissions E dev [B][T][Lmax + 1] (column 0 the blank's log-prob, column j that of label
 * j - 1 of the clip), so that they are tested apart from the head: lds_ctc_score's nll and lds_ctc_align's four outputs (include/lds.h).
 * labels dev int64 [B][Lmax] are read for their repeats only.  The Viterbi workspace holds B * T * 256 bytes of back-pointers or more. */
int lds_test_ctc_forward(const float* E, int B, int T, const int32_t* n_frames, const int64_t* labels, const int32_t* label_len, int Lmax, float* nll,
                         void* stream);
int lds_test_ctc_viterbi(const float* E, int B, int T, const int32_t* n_frames, const int64_t* labels, const int32_t* label_len, int Lmax, float* path_score,
                         int32_t* frame_label, int32_t* segments, float* label_logprob, void* ws, size_t ws_bytes, void* stream);

/* ---- the resnets' k 3 convolution in the Winograd form F(2,3) (csrc/conv_wino.hip) ----------------------------------------------
 * lds_test_wino_pack (host only): g [Co][Ci][3] -> U [4][Co][Ci], U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2, computed in
 * double and rounded once.
 * lds_test_wino_conv: out = conv_k3(act(GroupNorm([x1 ; x2]) (* (1 + scale) + shift))) + bias (+ res) as the UNet's routed resnet convolutions
 * run it: GroupNorm partials of the sources, the transform pass (gn_wino_kernel), conv_wino.  Planes, K4P output and partial buffers start as
 * NaN.  out dev [B,Co,T]; vplanes (or NULL) dev [B][Ci/8][2][4][ceil(T/2)][4], the raw planes; gnpart (or NULL) dev [B][Co/16][ceil(T/32)][2],
 * the epilogue's (mean, M2) of every (16 channels x 32 frames) block inside a length.  lengths: frames at and beyond lengths[b] are outside
 * utterance b (zeros in x and res as the kernels see them, zeros in out).  poison 1: the sources' pad frames and their frames beyond the
 * lengths hold NaN / Inf when the transform pass reads them.  An armed lds_test_tap_k4p receives the raw K4P output.
 * lds_bench_wino: the direct pair (gn_stream + conv_dma) against the Winograd pair on the same inputs, alternating in blocks of `iters`
 * passes, `reps` times; ms_direct / ms_wino [reps] = a block's device time per pass (events on the stream around each block). */
int lds_test_wino_pack(const float* g, int Co, int Ci, float* U);
/* x1 / x2 dev [B,C1,T] / [B,C2,T] (x2 may be NULL); gamma / beta host [C1+C2]; scale_shift dev [B, 2 (C1+C2)] (scales, then shifts) or NULL;
 * w / bias host, reference layout [Co, C1+C2, 3] / [Co] or NULL; res dev [B,Co,T] or NULL; lengths HOST int32 [B], 1 <= lengths[b] <= T, or
 * NULL; cfg 0 = the launcher's choice, else BK * 10 + NST in {322, 162} */
int lds_test_wino_conv(const float* x1, const float* x2, int C1, int C2, int T, const float* gamma, const float* beta, const float* scale_shift,
                       int groups, int silu, const float* w, const float* bias, int Co, const float* res, const int32_t* lengths, int poison, int cfg,
                       float* out, float* vplanes, float* gnpart, int B, void* stream);
int lds_bench_wino(const float* x1, const float* x2, int C1, int C2, int T, const float* gamma, const float* beta, const float* scale_shift,
                   int groups, int silu, const float* w, const float* bias, int Co, const float* res, int cfg, int B, int iters, int reps,
                   float* ms_direct, float* ms_wino, char* cfg_out, size_t cfg_cap, void* stream);
/* lds_test_wino_conv at level lvl of a ragged batch, as the UNet's resnets run below the first level: lengths are the LEVEL-0 lengths, T is the
 * tensors' length at level lvl, and every length reduced lvl times by (n - 1) / 2 + 1 lies in 1 .. T.  The sources, the residual, the poison
 * and the sources' partials are staged with the reduced lengths; both kernels receive the level-0 lengths and lvl and reduce them themselves.
 * lvl 0 is lds_test_wino_conv. */
int lds_test_wino_conv_lvl(const float* x1, const float* x2, int C1, int C2, int T, const float* gamma, const float* beta, const float* scale_shift,
                           int groups, int silu, const float* w, const float* bias, int Co, const float* res, const int32_t* lengths, int poison, int cfg,
                           int lvl, float* out, float* vplanes, float* gnpart, int B, void* stream);
/* the routing table of the UNet's resnets (csrc/model.hip wino_min_T): the shortest T at which a k 3 convolution Ci -> Co runs on conv_wino in
 * exact-fp32 mode, 0 = never.  Host only; returns the value, not a status. */
int lds_test_wino_min_T(int Ci, int Co);

/* ---- conv2 + the 1x1 shortcut of a resnet as one conv_wino launch over Cm + Cin / 2 channels (csrc/model.hip run_wconv_pair) ----------------
 * lds_test_wino_pair_pack (host only): g [Co][Cm][3], S [Co][Cin] -> U [4][Co][Cm + Cin/2]: lds_test_wino_pack's taps of g, then per tap the
 * Cin / 2 extension columns S_A, S_B / 2, S_B / 2, -S_A (S_A / S_B: the first / second half of S's columns), computed in double, rounded once.
 * lds_test_wino_pair: out = conv_k3(SiLU(GroupNorm2(h) (* (1 + scale) + shift)); w2) + conv_1x1([x1 ; x2]; ws) + b2 + bs as run_resnet runs a
 * routed pair: conv1's GroupNorm pass over [x1 ; x2] (gamma1 / beta1, SiLU) with the side output, conv2's pass over h (gn_wpair), the launch.
 * h dev [B,Cm,T]; x1 / x2 dev [B,C1,T] / [B,C2,T] (x2 may be NULL); gamma / beta host; scale_shift dev [B, 2 Cm] or NULL; w2 [Cm,Cm,3], ws
 * [Cm,C1+C2], b2 / bs [Cm] host.  lengths (LEVEL-0, host, or NULL), lvl, poison, cfg as lds_test_wino_conv_lvl.  out dev [B,Cm,T]; vplanes (or
 * NULL) dev [B][Cin/8][2][4][P][4]: conv1's planes, bit for bit lds_test_wino_conv's; pplanes (or NULL) dev [B][(Cm + Cin/2)/8][2][4][P][4]: the
 * launch's planes (conv2's blocks, then the shortcut's); gnpart (or NULL) as lds_test_wino_conv.  Every buffer starts as NaN.
 * lds_bench_wino_pair: the direct tail (conv1's pass, gn_stream, conv_dma_pair) against the new one (conv1's pass with the side output,
 * gn_wpair, conv_wino_pair), alternating as lds_bench_wino.
 * lds_test_wino_pair_min_T: the routing table (csrc/model.hip wino_pair_min_T), 0 = never; a pair is routed only where conv1 is as well. */
int lds_test_wino_pair_pack(const float* g, const float* S, int Co, int Cm, int Cin, float* U);
int lds_test_wino_pair(const float* h, const float* x1, const float* x2, int Cm, int C1, int C2, int T, const float* gamma1, const float* beta1,
                       const float* gamma2, const float* beta2, const float* scale_shift, int groups, const float* w2, const float* b2, const float* ws,
                       const float* bs, const int32_t* lengths, int poison, int cfg, int lvl, float* out, float* vplanes, float* pplanes, float* gnpart, int B,
                       void* stream);
int lds_bench_wino_pair(const float* h, const float* x1, const float* x2, int Cm, int C1, int C2, int T, const float* gamma1, const float* beta1,
                        const float* gamma2, const float* beta2, const float* scale_shift, int groups, const float* w2, const float* b2, const float* ws,
                        const float* bs, int cfg, int B, int iters, int reps, float* ms_direct, float* ms_wino, char* cfg_out, size_t cfg_cap, void* stream);
int lds_test_wino_pair_min_T(int Cin, int Cm);

/* ---- x-vector head, one layer at a time (csrc/xvector.hip; limits as lds_xvector_*) -----------------------------------------------------------
 * lds_test_xvector_tdnn: X dev [B][T][Cin], n_frames host [B] (0 .. T), W dev [Cout][ks Cin], bias dev [Cout] -> Y dev [B][T][Cout]: rows below
 * T_out = n_frames[b] - (ks - 1) d hold the layer (relu 0 / 1), the rows from there to T zeros.  ks 1 without relu is the projector.
 * lds_test_xvector_pool: the layer with ReLU and the pooling in its epilogue -> stats dev [B][2 Cout] (means, then unbiased standard deviations);
 * every clip needs T_out >= 2.  Y (dev [B][T][Cout] or NULL): the unfused layer's output as well, bit for bit what was pooled. */
int lds_test_xvector_tdnn(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int Cin, int Cout, int ks, int dil, int relu,
                          float* Y, void* stream);
int lds_test_xvector_pool_workspace_bytes(int B, int T, int Cout, size_t* out);
int lds_test_xvector_pool(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int Cin, int Cout, int ks, int dil,
                          float* stats, float* Y, void* ws, size_t ws_bytes, void* stream);

/* ---- debugging aids (tests/test_gpu_poison.py, tools/diag_trace.py)----------------------------------------------------------
 * lds_debug_fill_u32: every 32-bit word of a device buffer = pattern.  Tests fill a caller workspace with NaN patterns (0x7fc07fc0 is a NaN
 * as fp32 and as two fp16 / bf16 halves) before a call: a kernel that reads a slot no kernel of THAT call wrote turns it into a NaN (or, behind
 * a select, into a result that differs from the zero-filled run's).
 * lds_debug_trace(1): clear the records and, while on, make every lds_unet_forward synchronise after each stage and keep a host copy of the
 * stage's output tensor (names "down0.res1.conv1", "mid.tfm.att2", ...; activation tensors in the handle's layout: K4P fp32, or split planes
 * [B][C/8][planes][T+2][8] 16-bit); lds_debug_trace(0) stops recording and keeps the records for lds_debug_trace_get.  Process-global. */
int lds_debug_fill_u32(void* dev, size_t n_words, uint32_t pattern, void* stream);
/* the workspace plan of lds_unet_forward(B, T) as text, one slot per line: "name offset bytes" */
int lds_debug_unet_plan(const lds_unet* u, int B, int T, char* buf, size_t cap);
int lds_debug_trace(int on);
int lds_debug_trace_count(void);
int lds_debug_trace_get(int i, char* name, size_t name_cap, const void** data, size_t* bytes);

/* The Whisper decoder's vocabulary head alone (csrc/whisper_dec.hip: the linear's head epilogue + wd_choose_kernel).  x dev [N][K] (N <= 64,
 * 32 <= K <= 8192), ln_g / ln_b dev [K] (the final LayerNorm), et dev [K][V] (the token embedding transposed), suppress dev int32
 * [n_suppress] or NULL -> token dev int64 [N] (arg-max over the unsuppressed columns, ties to the lowest id), logprob dev [N] (its
 * log-softmax over them), lse dev [N], logits dev [N][V] or NULL (raw).  Synchronises. */
int lds_test_whisper_head(const float* x, const float* ln_g, const float* ln_b, const float* et, int N, int K, int V, const int32_t* suppress,
                          int n_suppress, int64_t* token, float* logprob, float* lse, float* logits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDS_TEST_H */
