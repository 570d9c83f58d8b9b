/*
 * liblds.so -- C ABI of the MI355X-native latent-diffusion speech sampler.
 *
 * The reference (bfloat16/latent-diffusion-speech) is pure Python on PyTorch and has no
 * FFI layer of its own; its drop-in boundary is the module API
 *   diffusion.unit2mel.Unit2Mel / load_model_vocoder   (reference diffusion/unit2mel.py:18-88)
 *   diffusion.diffusion.GaussianDiffusion.forward      (reference diffusion/diffusion.py:189-343)
 *   diffusion.vocoder.Vocoder.infer                    (reference diffusion/vocoder.py:32-33)
 *   diffusion.vocoder.Vocoder.extract                  (reference diffusion/vocoder.py:20-31, hifi_vaegan.py:32-50)
 * which the modules under latent-diffusion-speech_amd/diffusion/ re-expose unchanged.  Those modules keep
 * tensors, streams and checkpoints in PyTorch and call the entry points below through ctypes
 * (latent-diffusion-speech_amd/lds/native.py); INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer marked "dev" is device memory owned by the caller (a torch tensor);
 *     "host" pointers are read during the call only.
 *   - activations are fp32, channel-major [B, C, T] with the frame axis contiguous.
 *   - `stream` is a hipStream_t passed as void*; the forward / run calls only enqueue work on it and
 *     never synchronise the device (host arrays they are handed -- the sampler's table -- are copied into
 *     the launches' kernel arguments during the call).  Exceptions, documented at the function:
 *     lds_lm_generate polls for EOS, *_create upload weights, lds_prof_summary reads events.
 *     Handles are immutable after create EXCEPT for the two mode switches of the denoiser (lds_unet_set_gemm_mode,
 *     lds_unet_set_latency_mode): calls on different streams / threads are safe as long as each has its own
 *     workspace and nobody switches a mode meanwhile -- a switch while another thread is inside a forward or
 *     sampler call of the same handle is refused with LDS_EBUSY (the handle counts the calls in progress).
 *   - return value 0 = ok, negative LDS_E* on error; lds_last_error() gives the message
 *     (thread-local).  Nothing throws or aborts.
 */
#ifndef LDS_H
#define LDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDS_OK 0
#define LDS_EINVAL (-1)    /* bad argument / unsupported shape */
#define LDS_ENOMEM (-2)    /* workspace too small or device allocation failed */
#define LDS_EHIP (-3)      /* a HIP runtime call failed */
#define LDS_EMISSING (-4)  /* a required weight tensor was not supplied */
#define LDS_EBUSY (-5)     /* a mode switch while another thread is inside a forward / sampler call of the same handle */

typedef struct lds_unet lds_unet;
typedef struct lds_embed lds_embed;
typedef struct lds_vocoder lds_vocoder;

const char* lds_last_error(void);
int lds_version(void);

/* ---- denoiser: UNet1DConditionModel (reference diffusion/unet1d/unet_1d_condition.py:61-1036,
 *      configured as in reference diffusion/unit2mel.py:62-71) ------------------------------ */
typedef struct {
    int out_dims;              /* mel channels M (x / eps channels)                       */
    int n_hidden;              /* condition channels H; UNet in_channels = M + H          */
    int n_layers;              /* layers_per_block                                        */
    int n_heads;               /* attention heads (reference attention_head_dim)          */
    int norm_groups;           /* GroupNorm groups (8)                                    */
    int n_blocks;              /* len(block_out_channels), <= 8                           */
    int block_out_channels[8];
} lds_unet_cfg;

/* names[i] are the reference's state_dict keys of UNet1DConditionModel (e.g.
 * "down_blocks.0.resnets.0.conv1.weight"), host_ptrs[i] fp32 host arrays in the reference's
 * own layouts, numel[i] their element counts.  Weights are re-laid-out and uploaded once. */
int lds_unet_create(const lds_unet_cfg* cfg, int n_tensors, const char* const* names,
                    const float* const* host_ptrs, const int64_t* numel, lds_unet** out);
void lds_unet_destroy(lds_unet* u);
int lds_unet_workspace_bytes(const lds_unet* u, int B, int T, size_t* out);

/* One denoiser evaluation = `self.denoise_fn(cat([x, cond], dim=-2), t).sample`
 * (reference diffusion/diffusion.py:105-106,223-226).
 * x dev [B,M,T], cond dev [B,H,T], t dev [B] (fp32, may be fractional), eps dev [B,M,T]. */
int lds_unet_forward(lds_unet* u, const float* x, const float* cond, const float* t, float* eps,
                     void* ws, size_t ws_bytes, int B, int T, void* stream);

/* ---- sampler: GaussianDiffusion.forward(infer=True) loops (reference diffusion/diffusion.py:
 *      214-341; DPM-Solver++ dpm_solver_pytorch.py:1171-1213; UniPC uni_pc.py:590-658) -------- */
#define LDS_METHOD_DPM_SOLVER_PP 1
#define LDS_METHOD_UNIPC 2
#define LDS_METHOD_DDPM 3
#define LDS_METHOD_DDIM 4
#define LDS_METHOD_PLMS 5
#define LDS_TABLE_STRIDE 16

/* `table` (host, n_rows x LDS_TABLE_STRIDE floats) holds the per-step scalar coefficients,
 * computed by the caller from the noise schedule in fp32 (layout per method: see
 * latent-diffusion-speech_amd/diffusion/diffusion.py and lds_sampler_run in csrc/model.hip).  The table is read on the
 * host during the call (it may be freed afterwards); no device synchronisation is performed.
 * x dev [B,M,T] is x_T on entry and the sample on return; cond dev [B,H,T];
 * noise dev [n_rows,B,M,T] for DDPM (one draw per step), else NULL. */
int lds_sampler_run(lds_unet* u, int method, int n_rows, const float* table, const float* cond,
                    float* x, const float* noise, void* ws, size_t ws_bytes, int B, int T,
                    void* stream);
int lds_sampler_workspace_bytes(const lds_unet* u, int B, int T, size_t* out);

/* Ragged batches (the reference's 22_infer_tts.py:76-114 synthesises sentences of different lengths; a padded torch batch would change
 * every GroupNorm statistic and attention row): `lengths` (host int32 [B], 1 <= lengths[b] <= T, B <= 64) are the utterances' own frame
 * counts inside buffers of T frames.  Every kernel stops an utterance's statistics and attention keys at its length and writes zeros
 * beyond it (the convolutions' zero padding, as when the utterance runs alone), and the decoder resamples every utterance to its own skip
 * lengths.  Frames [0, lengths[b]) of utterance b equal the utterance run alone at its own length within the stated tolerances (not bit
 * for bit: tile shapes follow the buffer length); frames beyond are unspecified in x / zero in eps.  Every GEMM mode. */
int lds_unet_forward_ragged(lds_unet* u, const float* x, const float* cond, const float* t, const int32_t* lengths, float* eps, void* ws,
                            size_t ws_bytes, int B, int T, void* stream);
int lds_sampler_run_ragged(lds_unet* u, int method, int n_rows, const float* table, const float* cond, float* x, const float* noise,
                           const int32_t* lengths, void* ws, size_t ws_bytes, int B, int T, void* stream);

/* ---- front end: Unit2Mel.forward's condition (reference diffusion/unit2mel.py:79-82) ---------
 * cond[b,:,t] = unit_embed(units[b,t,:]) + spk_embed[spk_id[b]-1]                               */
int lds_embed_create(int input_channel, int n_hidden, int n_spk, const float* unit_w,
                     const float* unit_b, const float* spk_w, lds_embed** out);
void lds_embed_destroy(lds_embed* e);
int lds_embed_workspace_bytes(const lds_embed* e, int B, int T, size_t* out);
/* units dev [B,T,input_channel], spk_id dev [B] int64 (1-based, may be NULL when n_spk<=1),
 * cond dev [B,n_hidden,T]. */
int lds_embed_forward(lds_embed* e, const float* units, const int64_t* spk_id, float* cond,
                      void* ws, size_t ws_bytes, int B, int T, void* stream);

/* out[b,c,r] = in[b,r,c] / div  (the [B,T,M] <-> [B,M,T] layout changes at the module
 * boundary: reference diffusion/diffusion.py:190,342-343, hifi_vaegan.py:54). */
int lds_transpose(const float* in, float* out, int B, int R, int C, float div, void* stream);
/* ---- token -> unit-embedding step in front of the path (reference 22_infer_tts.py:43-52,100-110) -------------
 * out[i,:] = table[idx[i],:]: the k-means codebook lookup `semantic_embedding(semantic_token)` (nn.Embedding over
 * cluster_centers_ [n_rows, C]); an index outside [0, n_rows) yields a NaN row (nn.Embedding raises). */
int lds_gather_rows(const float* table, const int64_t* idx, float* out, int n_idx, int C, int n_rows, void* stream);
/* out[b,i,:] = in[b, min((int)floorf(i*step), Tin-1), :]: F.interpolate(mode='nearest') of units_forced_alignment
 * (reference tools/tools.py:193-223) on frame-major units [B,Tin,C] -> [B,Tout,C]; step = 1/scale_factor (fp32). */
int lds_resample_frames(const float* in, float* out, int B, int Tin, int Tout, int C, float step, void* stream);
/* out = c0*a + c1*b over n elements (q_sample of shallow diffusion, reference diffusion.py:169-171) */
int lds_axpby(float* out, const float* a, const float* b, float c0, float c1, int64_t n, void* stream);

/* ---- the diffusion loss of the validation pass (reference diffusion.py:169-187: q_sample with one timestep per item, the denoiser, the mean
 *      residual; evaluated without gradients, reference solver.py:56-62) ------------------------------------------------------------------
 * lds_q_sample_rows: out[b][i] = sqrt_ac[t[b]] * x0[b][i] + sqrt_1m_ac[t[b]] * noise[b][i] over rows of n elements; the two products are
 * rounded separately and then added, so the result has the reference's bits.  t dev int64 [B], read on the device and clamped into
 * [0, n_steps); the tables dev fp32 [n_steps]; t_f32 (dev [B] or NULL) receives t as fp32, the time input of lds_unet_forward.
 * lds_loss_reduce: out[0] (dev) = mean((a - b)^2) (loss_type 2, F.mse_loss) or mean(|a - b|) (loss_type 1) over n elements.  Deterministic:
 * fixed slices of 4096 elements per workgroup, each summed in a fixed tree in double, and one fixed-order second stage over the partial sums
 * in ws (lds_loss_reduce_workspace_bytes(n), 8-byte aligned); no atomics. */
int lds_q_sample_rows(float* out, const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac, const float* sqrt_1m_ac,
                      int n_steps, float* t_f32, int B, int64_t n, void* stream);
int lds_loss_reduce_workspace_bytes(int64_t n, size_t* out);
int lds_loss_reduce(const float* a, const float* b, int64_t n, int loss_type, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- the vocoder's log-mel analysis (reference encoder/hifi_vaegan/modules/nvSTFT.py:69-118, STFT.get_mel with center = False) --------
 * audio dev [B][L] -> out dev [B][F][n_mels] = log(max(mel_basis @ |STFT(pad(audio))|, clip_val)), frame-major, as one launch.
 * Geometry, resolved by the caller from (keyshift, speed): n_fft_new = round(n_fft * 2^(keyshift/12)), win_new likewise from win, hop_new =
 * round(hop * speed).  The library pads each clip as the reference does -- (win_new - hop_new) / 2 samples on the left, max((win_new - hop_new
 * + 1) / 2, win_new - len - left) on the right, reflected when the right pad is shorter than the clip and zeros otherwise -- and takes
 * 1 + (len + left + right - n_fft_new) / hop_new frames; nothing at or beyond a clip's length is read.
 * basis: dev double [n_fft_new][bins][2], bins = min(n_fft_new / 2 + 1, n_fft / 2 + 1): (cos, -sin)(2 pi n k / n_fft_new) times the window
 * (centred in n_fft_new).  mel_basisT: dev fp32 [n_fft / 2 + 1][n_mels], the transposed filter bank.  When win_new != win the magnitudes are
 * scaled by win / win_new, and bins at and beyond `bins` count as zeros (nvSTFT.py:110-115).  The DFT sums run in double on the f64 matrix
 * pipe, the rest in fp32.
 * lengths: host int32 [B] (B <= 64; 1 .. L) or NULL = every clip has L samples.  Each clip's padding mode and frame count follow its own
 * length; its rows [0, F_b) equal the clip run alone bit for bit, rows [F_b, F) are zeros.  F: the rows of out, at least the longest clip's
 * frames.  n_mels <= 128; 15 hop_new + n_fft_new samples must fit the workgroup's LDS (LDS_EINVAL otherwise).
 * The launch keeps the spectrum inside the workgroup, so lds_stft_mel_workspace_bytes answers 0 today and ws may be NULL. */
int lds_stft_mel_workspace_bytes(int n_fft_new, int hop_new, int n_mels, int B, int64_t L, size_t* out);
int lds_stft_mel(const float* audio, const int32_t* lengths, const double* basis, const float* mel_basisT, int n_fft_new, int win_new,
                 int hop_new, int n_fft, int win, int n_mels, float clip_val, int F, float* out, void* ws, size_t ws_bytes, int B, int64_t L,
                 void* stream);

/* ---- vocoder: HiFi-VAEGAN Generator (reference encoder/hifi_vaegan/modules/models.py:224-272,
 *      hifi_vaegan.py:52-65) ------------------------------------------------------------------- */
typedef struct {
    int inter_channels;             /* latent / mel channels                                */
    int upsample_initial_channel;
    int n_ups;                      /* <= 8 */
    int upsample_rates[8];
    int upsample_kernel_sizes[8];
    int resblock;                   /* 1 or 2 */
    int n_kernels;                  /* <= 4 */
    int resblock_kernel_sizes[4];
    int n_dil;                      /* dilations per resblock, <= 4 */
    int resblock_dilation_sizes[4][4];
} lds_vocoder_cfg;

/* names: the reference Generator's state_dict keys; weight-norm pairs (`*.weight_g`,
 * `*.weight_v`) are folded here like remove_weight_norm() (reference hifi_vaegan.py:61);
 * already-folded `*.weight` tensors are accepted too. */
int lds_vocoder_create(const lds_vocoder_cfg* cfg, int n_tensors, const char* const* names,
                       const float* const* host_ptrs, const int64_t* numel, lds_vocoder** out);
void lds_vocoder_destroy(lds_vocoder* v);
int lds_vocoder_workspace_bytes(const lds_vocoder* v, int B, int T, size_t* out);
/* z dev [B,C,T] -> wav dev [B,1,T*prod(upsample_rates)] */
int lds_vocoder_forward(lds_vocoder* v, const float* z, float* wav, void* ws, size_t ws_bytes,
                        int B, int T, void* stream);
/* Ragged batch (see lds_sampler_run_ragged): lengths host int32 [B] (B <= 64) = the utterances' own frame counts inside z [B,C,T].  Every
 * stage of the generator writes zeros beyond an utterance's (up-sampled) length -- the zero padding its convolutions see when it runs
 * alone -- and z itself is read as zeros there; samples [0, lengths[b] * prod(rates)) of wav[b] equal the utterance decoded alone within the
 * stated tolerance, the samples beyond are zeros. */
int lds_vocoder_forward_ragged(lds_vocoder* v, const float* z, const int32_t* lengths, float* wav, void* ws, size_t ws_bytes,
                               int B, int T, void* stream);

/* ---- VAE encoder: HiFi-VAEGAN Encoder, audio -> latent (reference encoder/hifi_vaegan/modules/models.py:14-67,
 *      hifi_vaegan.py:32-50; called from diffusion/vocoder.py:24-31 and batch_proccessor/acoustic_extract.py:46) ----------------
 * The same lds_vocoder_cfg as the generator (upsample_rates / kernel sizes are read in reverse, as the reference does); each
 * downsampler must have kernel = 2 * stride with the stride a power of two in 2 .. 16 (LDS_EINVAL otherwise).  names: the reference
 * Encoder's state_dict keys; weight-norm pairs are folded like remove_weight_norm() (the `ups.i` weights are Conv1d [Cout][Cin][k], so
 * the norm runs over all dims but Cout); a missing key gives LDS_EMISSING naming it.  L (samples per utterance) must be a positive
 * multiple of the hop prod(upsample_rates); T = L / hop frames. */
typedef struct lds_vae_encoder lds_vae_encoder;
int  lds_vae_encoder_create(const lds_vocoder_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs,
                            const int64_t* numel, lds_vae_encoder** out);
void lds_vae_encoder_destroy(lds_vae_encoder* e);
int  lds_vae_encoder_workspace_bytes(const lds_vae_encoder* e, int B, int64_t L, size_t* out);
/* audio dev [B][L]; noise dev [B][C][T] or NULL; out dev [B][T][2C] = cat(m, logs) frame-major (logs written as zeros when only_mean);
 * z dev [B][T][C] = m + noise * exp(logs) (the real logs, whatever only_mean) or NULL (needs noise) */
int  lds_vae_encoder_forward(lds_vae_encoder* e, const float* audio, const float* noise, float* out, float* z,
                             int only_mean, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);
/* Ragged batch (see lds_vocoder_forward_ragged): lengths host int32 [B] (B <= 64) = every clip's own sample count inside audio [B][L],
 * 1 <= lengths[b] <= L.  Clip b is encoded as if alone (zero-padded to ceil(lengths[b] / hop) * hop samples, T_b frames): every stage of
 * the encoder stores zeros beyond the clip's length at that stage, which is the zero padding its convolutions see when it runs alone.
 * Rows [T_b, T) of out and z are zeros; samples of audio beyond lengths[b] are never read as anything but zero (NaN / Inf included), nor
 * is noise beyond T_b.  Rows [0, T_b) equal the clip encoded alone within the stated tolerance; with every length equal to L the result
 * is lds_vae_encoder_forward's, bit for bit.  Uses lds_vae_encoder_workspace_bytes; a bad length, a null lengths or B > 64 give
 * LDS_EINVAL naming the value, before anything is enqueued. */
int  lds_vae_encoder_forward_ragged(lds_vae_encoder* e, const float* audio, const int32_t* lengths, const float* noise, float* out,
                                    float* z, int only_mean, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);

/* ---- units encoder: Whisper log-mel front end + AudioEncoder, audio -> units (reference tools/tools.py:43-126 Units_Encoder /
 *      WhisperLargeV3, encoder/whisper/audio.py:62-82, encoder/whisper/model.py:112-131) -------------------------------------------
 * names: the reference Whisper.state_dict() keys ("encoder.conv1.weight", "encoder.blocks.N.attn.query.weight", ...,
 * "encoder.ln_post.bias"; `key` has no bias), fp32 host arrays in the reference's layouts.  mel_filters: host [n_mels][201] (the filter
 * bank of audio.py:55-60).  Limits (LDS_EINVAL): n_mels 80 or 128, n_state a multiple of 64 with n_state / n_head == 64, 1 <= n_layer <= 64.
 * The sinusoid table of n_ctx rows is built at create with the reference's fp32 operation order.
 *
 * A call takes B clips in audio dev [B][L] (16 kHz samples, L >= 400).  lengths host int32 [B] (B <= 64), 400 <= lengths[b] <= L, or NULL
 * (every clip has L samples).  Clip b is audio[b, :lengths[b]] ENCODED ALONE: reflect padding at its own end, F_b = lengths[b] / 160 mel
 * frames, the dynamic-range floor from its own maximum, T_b = (F_b - 1) / 2 + 1 encoder frames, attention keys stop at T_b.  Nothing at or
 * beyond lengths[b] is read.  F = L / 160, T = (F - 1) / 2 + 1 <= n_ctx (LDS_EINVAL otherwise).  A clip's result does not depend on the
 * other clips of the call.  Nothing synchronises; a bad argument returns before anything is enqueued; a small workspace gives LDS_ENOMEM. */
typedef struct lds_whisper lds_whisper;
typedef struct { int n_mels, n_state, n_head, n_layer, n_ctx; } lds_whisper_cfg;
int  lds_whisper_create(const lds_whisper_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel,
                        const float* mel_filters, lds_whisper** out);
void lds_whisper_destroy(lds_whisper* w);
/* one size for all three calls below (lds_whisper_encode_mel: L = 160 * F) */
int  lds_whisper_workspace_bytes(const lds_whisper* w, int B, int64_t L, size_t* out);
/* mel dev [B][n_mels][F] plain = log_mel_spectrogram of every clip; frames at and beyond F_b are zeros */
int  lds_whisper_logmel(lds_whisper* w, const float* audio, const int32_t* lengths, float* mel, void* ws, size_t ws_bytes, int B, int64_t L,
                        void* stream);
/* AudioEncoder.forward: mel dev [B][n_mels][F] plain, n_frames host int32 [B] (1 <= n_frames[b] <= F; mel beyond is read as zeros) or NULL
 * -> units dev [B][T][n_state] frame-major; rows at and beyond T_b are zeros */
int  lds_whisper_encode_mel(lds_whisper* w, const float* mel, const int32_t* n_frames, float* units, void* ws, size_t ws_bytes, int B, int F,
                            void* stream);
/* both in one call (WhisperLargeV3.__call__): the log-mel goes straight into the first convolution's input layout */
int  lds_whisper_encode(lds_whisper* w, const float* audio, const int32_t* lengths, float* units, void* ws, size_t ws_bytes, int B, int64_t L,
                        void* stream);

/* ---- units encoder: HuBERT-base / HuBERT-Soft / ContentVec, audio -> units (reference encoder/hubert/model.py:19-148: Hubert.encode,
 *      HubertSoft.units) -------------------------------------------------------------------------------------------------------------------
 * A 7-layer waveform convolution stack (conv0 k 10 stride 5 + GroupNorm per channel; conv1..4 k 3, conv5..6 k 2, all stride 2, no bias, no
 * padding, GELU), LayerNorm + Linear (conv_dim -> n_state), a grouped positional convolution (pos_kernel taps, pos_groups groups, weight norm
 * folded at create in double) added to its input and normalised, n_layer post-LayerNorm blocks (nn.TransformerEncoderLayer, GELU,
 * norm_first False, eps 1e-5) and proj (n_state -> n_proj).  names: the reference Hubert.state_dict() keys ("feature_extractor.conv0.weight",
 * "positional_embedding.conv.parametrizations.weight.original0" = g [1][1][K], "...original1" = v, "encoder.layers.N.self_attn.in_proj_weight",
 * ..., "proj.bias"; masked_spec_embed and label_embedding.weight are not read), fp32 host arrays in the reference's layouts.
 * HuBERT-base: {512, 768, 12, 12, 3072, 256, 128, 16, 1500}.  Limits (LDS_EINVAL): conv_dim and n_state multiples of 64 up to 1024,
 * n_state / n_head == 64, n_ffn and n_proj multiples of 64, n_state / pos_groups in {16, 32, 48, 64}, pos_kernel even in 2 .. 128,
 * 1 <= n_layer <= 64, 1 <= n_ctx <= 1500 (the range the attention kernel is tested in).
 *
 * A call takes B clips in audio dev [B][L] (16 kHz samples).  `pad` zeros are added on each side of every clip: 40 is HubertSoft.units
 * (F.pad(wav, (40, 40)), T = L / 320 frames), 0 is Hubert.encode on a waveform as given; 0 <= pad <= 40, L + 2 pad >= 400.  The frame counts:
 * n0 = (L + 2 pad - 10) / 5 + 1, four times n <- (n - 3) / 2 + 1, twice n <- (n - 2) / 2 + 1 = T <= n_ctx.  lengths host int32 [B] (B <= 64),
 * 400 - 2 pad <= lengths[b] <= L, or NULL (every clip has L samples).  Clip b is audio[b, :lengths[b]] ENCODED ALONE: its own zero pad, its
 * own GroupNorm statistics over its own n0 frames, its own zero padding in the positional convolution, attention keys that stop at its T_b.
 * Nothing at or beyond lengths[b] is read; rows at and beyond T_b of a result are zeros.  A clip's result does not depend on the other clips
 * of the call.  Exact fp32, no floating-point atomics: a repeat gives the same bits.  Nothing synchronises; a bad argument returns before
 * anything is enqueued; a small workspace gives LDS_ENOMEM. */
typedef struct lds_hubert lds_hubert;
typedef struct lds_hubert_cfg { int conv_dim, n_state, n_head, n_layer, n_ffn, n_proj, pos_kernel, pos_groups, n_ctx; } lds_hubert_cfg;
int  lds_hubert_create(const lds_hubert_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel,
                       lds_hubert** out);
void lds_hubert_destroy(lds_hubert* h);
/* one size for both calls below */
int  lds_hubert_workspace_bytes(const lds_hubert* h, int B, int64_t L, int pad, size_t* out);
/* out dev [B][T][conv_dim] frame-major = the feature extractor's output (FeatureExtractor.forward, transposed) */
int  lds_hubert_features(lds_hubert* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, int pad,
                         void* stream);
/* Hubert.encode(., layer = n_layers_run)[0] -> out dev [B][T][n_state]; 0 <= n_layers_run <= n_layer (0 = the output of `norm`).  want_proj
 * (only with n_layers_run == n_layer): proj applied, out dev [B][T][n_proj] (HubertSoft.units with pad 40). */
int  lds_hubert_encode(lds_hubert* h, const float* audio, const int32_t* lengths, float* out, int n_layers_run, int want_proj, void* ws,
                       size_t ws_bytes, int B, int64_t L, int pad, void* stream);

/* ---- units encoder: wav2vec 2.0 in its layer-norm flavour (XLSR-53; reference tools/tools.py Audio2xlsr_53_56k = fairseq's
 *      extract_features(source, padding_mask = all False)["x"]), audio -> units ----------------------------------------------------------
 * Seven waveform convolutions with HuBERT's kernels and strides (conv0 k 10 stride 5; conv1..4 k 3, conv5..6 k 2, all stride 2, no
 * padding), each with a bias, a LayerNorm over the conv_dim channels of every frame and an erf GELU; LayerNorm + Linear (conv_dim -> n_state);
 * x + GELU(grouped positional convolution: pos_kernel taps, pos_groups groups, weight norm over the taps, padding pos_kernel / 2, last
 * frame dropped); n_layer pre-LayerNorm transformer blocks (n_head heads of 64, feed-forward n_ffn, biases on q, k, v, out); a final
 * LayerNorm.  The waveform is taken as it is (no normalisation, no padding).  A clip of n samples gives T = the frame rule of lds_hubert with
 * pad 0 (400 samples -> 1 frame, 30 s -> 1499).
 * Tensor names are fairseq's (what the reference's pretrain/xlsr_53_56k.pt holds): feature_extractor.conv_layers.{i}.0.{weight,bias},
 * feature_extractor.conv_layers.{i}.2.1.{weight,bias} (the LayerNorm), layer_norm.*, post_extract_proj.*,
 * encoder.pos_conv.0.{bias,weight_g,weight_v}, encoder.layers.{l}.self_attn.{q,k,v,out}_proj.*, .self_attn_layer_norm.*, .fc1.*, .fc2.*,
 * .final_layer_norm.*, encoder.layer_norm.*; other names are ignored.  LDS_EMISSING names a missing tensor.
 * Limits: conv_dim and n_state multiples of 64 up to 1024, n_state = 64 n_head, n_ffn a multiple of 64, pos_kernel even in 2 .. 128,
 * n_state / pos_groups in {16, 32, 48, 64}, 1 <= n_layer <= 64, T <= n_ctx <= 1500, 400 <= L <= 2^30.
 * audio: dev [B][L] fp32.  lengths: host int32 [B] (B <= 64, 400 <= lengths[b] <= L) or NULL: clip b is audio[b, :lengths[b]] encoded alone.
 * Nothing at or beyond lengths[b] is read; rows at and beyond T_b of a result are zeros.  A clip's result does not depend on the other clips
 * of the call.  Exact fp32, no floating-point atomics: a repeat gives the same bits.  Nothing synchronises; a bad argument returns before
 * anything is enqueued; a small workspace gives LDS_ENOMEM. */
typedef struct lds_w2v lds_w2v;
typedef struct lds_w2v_cfg { int conv_dim, n_state, n_head, n_layer, n_ffn, pos_kernel, pos_groups, n_ctx; } lds_w2v_cfg;
int  lds_w2v_create(const lds_w2v_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel, lds_w2v** out);
void lds_w2v_destroy(lds_w2v* h);
/* one size for both calls below */
int  lds_w2v_workspace_bytes(const lds_w2v* h, int B, int64_t L, size_t* out);
/* out dev [B][T][conv_dim] frame-major = the feature extractor's output (after the last LayerNorm + GELU) */
int  lds_w2v_features(lds_w2v* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);
/* out dev [B][T][n_state] = the output of encoder.layer_norm */
int  lds_w2v_encode(lds_w2v* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);

/* ---- units encoder: WavLM (transformers' WavLMModel: so-vits-svc's wavlmbase+, kNN-VC's WavLM-Large), audio -> units ----------------
 * Two flavours of one network, chosen by stable_layer_norm:
 *   0 (Base / Base+; feat_extract_norm "group", do_stable_layer_norm False): lds_hubert's skeleton -- seven bias-free waveform convolutions, a
 *     GroupNorm per channel behind conv0, LayerNorm + Linear (conv_dim -> n_state), x + GELU(grouped positional convolution), encoder.layer_norm,
 *     post-LayerNorm blocks.  WavLM-Base+: {512, 768, 12, 12, 3072, 128, 16, 320, 800, 0, 1500}.
 *   1 (Large; feat_extract_norm "layer", do_stable_layer_norm True): lds_w2v's skeleton with zero convolution biases -- a LayerNorm + GELU behind
 *     every convolution, pre-LayerNorm blocks, a final encoder.layer_norm.  WavLM-Large: {512, 1024, 16, 24, 4096, 128, 16, 320, 800, 1, 1500}.
 * conv_bias is False in both; eps 1e-5.  The self-attention of every block (n_head heads of 64), x its input [T][n_state]:
 *   p = gru_rel_pos_linear(x viewed as [n_head][T][64]) -> [n_head][T][8]; (a, b) = sigmoid of the sums of p[..., 0:4] and p[..., 4:8];
 *   gate[h][i] = a (b gru_rel_pos_const[h] - 1) + 2;   score(i, j) = q_i . k_j / 8 + gate[h][i] bias[h][j - i], soft-max over the clip's own keys;
 *   bias[h][d] = layer 0's rel_attn_embed.weight[bucket(d)][h] for every layer, bucket = WavLMAttention._relative_positions_bucket with
 *   nb = num_buckets / 2, me = nb / 2: (d > 0) nb + (|d| < me ? |d| : min(me + trunc(log(|d| / me) / log(max_distance / me) (nb - me)), nb - 1)),
 *   the logarithm branch in float32 as torch runs it.  The bias is kept as a table [n_head][2 n_ctx - 1] built at create; nothing of size
 *   T x T is stored.
 * Tensor names are the keys of WavLMModel.state_dict(): feature_extractor.conv_layers.{i}.conv.weight, .{i}.layer_norm.* (i = 0; every i in
 * the stable flavour), feature_projection.{layer_norm,projection}.*, encoder.pos_conv_embed.conv.{bias,parametrizations.weight.original0,
 * parametrizations.weight.original1} (weight norm folded at create in double), encoder.layer_norm.*, encoder.layers.{l}.attention.{q,k,v,out}_proj.*,
 * .attention.gru_rel_pos_linear.*, .attention.gru_rel_pos_const, encoder.layers.0.attention.rel_attn_embed.weight, .layer_norm.*,
 * .feed_forward.{intermediate_dense,output_dense}.*, .final_layer_norm.*; masked_spec_embed and other names are not read.  LDS_EMISSING names a
 * missing tensor.
 * Limits (LDS_EINVAL otherwise): conv_dim and n_state multiples of 64 up to 1024, n_state = 64 n_head, n_ffn a multiple of 64, pos_kernel even
 * in 2 .. 128, n_state / pos_groups in {16, 32, 48, 64}, 1 <= n_layer <= 64, num_buckets a multiple of 4 in 4 .. 4096,
 * num_buckets / 4 < max_distance <= 2^20, stable_layer_norm 0 or 1, T <= n_ctx <= 1500, 1 <= B <= 64, 400 <= L <= 2^30.
 * audio: dev [B][L] fp32 at 16 kHz.  A clip of n samples gives T = the frame rule of lds_hubert with pad 0 (400 samples -> 1 frame, 16,000 -> 49,
 * 30 s -> 1499).  lengths: host int32 [B] (400 <= lengths[b] <= L) or NULL: clip b is audio[b, :lengths[b]] encoded alone.  normalize (0 or 1):
 * with 1 every clip becomes (x - mean) / sqrt(var + 1e-7) over its own samples first (what Wav2Vec2FeatureExtractor(do_normalize=True) does in
 * front of WavLM-Large), statistics in double.
 * Nothing at or beyond lengths[b] is read; rows at and beyond T_b of a result are zeros.  A clip's result does not depend on the other clips
 * of the call.  Exact fp32, no floating-point atomics: a repeat gives the same bits.  Nothing synchronises; a bad argument returns before
 * anything is enqueued; a small workspace gives LDS_ENOMEM naming the size. */
typedef struct lds_wavlm lds_wavlm;
typedef struct lds_wavlm_cfg { int conv_dim, n_state, n_head, n_layer, n_ffn, pos_kernel, pos_groups, num_buckets, max_distance, stable_layer_norm, n_ctx; } lds_wavlm_cfg;
int  lds_wavlm_create(const lds_wavlm_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel, lds_wavlm** out);
void lds_wavlm_destroy(lds_wavlm* h);
/* one size for both calls below, with or without normalize */
int  lds_wavlm_workspace_bytes(const lds_wavlm* h, int B, int64_t L, size_t* out);
/* out dev [B][T][conv_dim] frame-major = feature_extractor(audio) transposed (before the projection's LayerNorm) */
int  lds_wavlm_features(lds_wavlm* h, const float* audio, const int32_t* lengths, float* out, int normalize, void* ws, size_t ws_bytes, int B, int64_t L,
                        void* stream);
/* out dev [B][T][n_state] = WavLMModel(audio, output_hidden_states=True).hidden_states[n_layers_run], 0 <= n_layers_run <= n_layer;
 * n_layers_run == n_layer gives last_hidden_state */
int  lds_wavlm_encode(lds_wavlm* h, const float* audio, const int32_t* lengths, float* out, int n_layers_run, int normalize, void* ws, size_t ws_bytes,
                      int B, int64_t L, void* stream);
/* out dev [B][T][n_state] = sum_l layer_w[l] hidden_states[l] over all n_layer + 1 hidden states, hidden_states[0] included: the weighted layer
 * sum of WavLMForXVector.forward under config.use_weighted_layer_sum (transformers 5.15 modeling_wavlm.py 1591-1596, "hidden_states = torch.stack(...);
 * norm_weights = softmax(self.layer_weights); hidden_states = (hidden_states * norm_weights.view(-1, 1, 1)).sum(dim=1)").  layer_w: HOST
 * float[n_layer + 1], finite, already soft-maxed.  One encode: each hidden state is added where it exists, out = (l == 0 ? 0 : out) + layer_w[l] h_l
 * (one fmaf) with l ascending, so the sum's order is fixed; no hidden state is stored.  Same workspace, limits and guarantees as lds_wavlm_encode. */
int  lds_wavlm_encode_layersum(lds_wavlm* h, const float* audio, const int32_t* lengths, const float* layer_w, float* out, int normalize, void* ws,
                               size_t ws_bytes, int B, int64_t L, void* stream);

/* ---- units encoder: w2v-BERT 2.0 (reference tools/tools.py Wav2Vec2Bert: transformers' Wav2Vec2BertModel(**SeamlessM4TFeatureExtractor(audio,
 *      sampling_rate = 16000)).last_hidden_state), audio -> units ------------------------------------------------------------------------
 * Front end (SeamlessM4TFeatureExtractor.__call__ on one clip): the waveform times 2^15; n = 1 + (len - 400) / 160 frames of 400 samples, not
 * centred; per frame mean removal, pre-emphasis 0.97, Povey window, 512-point power spectrum, n_mels Kaldi-scale mel triangles (20 Hz .. 8 kHz),
 * floor 1.192092955078125e-07, natural log; per mel bin (x - mean) / sqrt(var(ddof = 1) + 1e-7) over the clip's own n frames; `stride` frames side by
 * side per row: rows = ceil(n / stride) rows of n_mels * stride values of which valid = n / stride are unmasked.  With n odd (stride 2) the last
 * row is the MASKED ROW: its second half is the extractor's padding (0) and its attention-mask entry is 0.
 * Model (Wav2Vec2BertModel without adapter): LayerNorm + Linear (n_mels * stride -> n_state), masked rows set to 0; n_layer Conformer blocks:
 * x += 0.5 ffn1(LN(x)) (Linear n_state -> n_ffn, swish, Linear back); x += attention(LN(x)) with n_head heads of 64, biases on q, k, v, out, scores
 * (q.k + q.E[clamp(j - i, -left_max, right_max) + left_max]) / 8 with the layer's distance_embedding E, keys at and beyond `valid` excluded;
 * x += conv_module(x): LayerNorm, masked rows -> 0, pointwise 1x1 to 2 n_state without bias, GLU, causal depthwise convolution of dw_kernel taps
 * without bias, LayerNorm over the channels of each frame, swish, pointwise 1x1 without bias; x += 0.5 ffn2(LN(x)); x = final_layer_norm(x).
 * The result has `rows` rows per clip, the masked row INCLUDED, as last_hidden_state has it; a caller who does not want it drops row `valid`
 * when n is odd.  The masked row's padding never reaches another row.
 * Tensor names are transformers': feature_projection.{layer_norm,projection}.*, encoder.layers.{l}.{ffn1_layer_norm,ffn1.intermediate_dense,
 * ffn1.output_dense,self_attn_layer_norm,self_attn.linear_{q,k,v,out},conv_module.layer_norm,conv_module.depthwise_layer_norm,ffn2_layer_norm,
 * ffn2.intermediate_dense,ffn2.output_dense,final_layer_norm}.{weight,bias}, .self_attn.distance_embedding.weight,
 * .conv_module.{pointwise_conv1,depthwise_conv,pointwise_conv2}.weight; other names are ignored.  LDS_EMISSING names a missing tensor.
 * Limits (LDS_EINVAL otherwise): n_mels 8 .. 128 and stride 1 .. 8 with n_mels * stride a multiple of 32 up to 1024; n_state a multiple of 64 in
 * 64 .. 1024 = 64 n_head; n_ffn a multiple of 64; 1 <= n_layer <= 64; left_max + right_max + 1 <= 80; dw_kernel odd in 1 .. 31; rows <= n_ctx <= 1500;
 * 0 < eps < 1; at most 64 clips per call; 560 <= L <= 2^30 (560 samples = two frames: one frame makes the reference's variance 0 / 0).
 * audio: dev [B][L] fp32 at 16 kHz.  lengths: host int32 [B] (560 <= lengths[b] <= L) or NULL: clip b is audio[b, :lengths[b]] encoded alone.
 * Nothing at or beyond lengths[b] is read; rows at and beyond rows_b of a result are zeros.  A clip's result does not depend on the other clips
 * of the call.  The matrix products are exact fp32, the filter bank's DFT runs in double; no floating-point atomics: a repeat gives the same
 * bits.  Nothing synchronises; a bad argument returns before anything is enqueued; a small workspace gives LDS_ENOMEM. */
typedef struct lds_w2vbert lds_w2vbert;
typedef struct lds_w2vbert_cfg { int n_mels, stride, n_state, n_head, n_ffn, n_layer, left_max, right_max, dw_kernel, n_ctx; float eps; } lds_w2vbert_cfg;
int  lds_w2vbert_create(const lds_w2vbert_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel, lds_w2vbert** out);
void lds_w2vbert_destroy(lds_w2vbert* h);
/* one size for the three calls below; for encode_features with R rows pass L = 400 + 160 (stride R - 1) */
int  lds_w2vbert_workspace_bytes(const lds_w2vbert* h, int B, int64_t L, size_t* out);
/* out dev [B][Rmax][n_mels * stride] = SeamlessM4TFeatureExtractor's input_features (Rmax = the rows of L samples), zeros beyond rows_b */
int  lds_w2vbert_fbank(lds_w2vbert* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);
/* feats dev [B][R][n_mels * stride] (input_features), n_frames host int32 [B] (the clips' frame counts n, max(2, stride) .. stride R) or NULL
 * (= stride R) -> out dev [B][R][n_state] = Wav2Vec2BertModel(input_features, attention_mask).last_hidden_state; feats rows at and beyond n / stride
 * are not read */
int  lds_w2vbert_encode_features(lds_w2vbert* h, const float* feats, const int32_t* n_frames, float* out, void* ws, size_t ws_bytes, int B, int R, void* stream);
/* out dev [B][Rmax][n_state]: the two calls above in one */
int  lds_w2vbert_encode(lds_w2vbert* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);

/* ---- text2semantic: RoFormer encoder prefill + cached autoregressive decode (reference text2semantic/roformer/roformer.py:59-255
 *      over HF transformers RoFormerModel / RoFormerForCausalLM + GenerationMixin; called from 22_infer_tts.py:76-98) ------------- */
typedef struct lds_lm lds_lm;
typedef struct {
    int hidden, heads, inter;          /* 256, 8, 512 (reference configs/config.yaml:60-83)                          */
    int enc_layers, dec_layers;        /* 4, 1                                                                        */
    int text_vocab, type_vocab;        /* phone symbols + 3, tones + 1                                                */
    int sem_vocab;                     /* semantic_kmeans_num + 3                                                     */
    int n_spk_rows;                    /* rows of spk_emb (n_spk + 1), 0 = no speaker embedding                       */
    int max_pos;                       /* rows of the sinusoid tables                                                 */
    float eps;                         /* layer_norm_eps                                                              */
    int sem_bos, sem_eos, sem_pad;
} lds_lm_cfg;
/* names = the reference Roformer.state_dict() keys (text_encoder.*, semantic_decoder.*, spk_emb.weight), fp32 host arrays */
int lds_lm_create(const lds_lm_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel,
                  lds_lm** out);
void lds_lm_destroy(lds_lm* lm);
int lds_lm_workspace_bytes(const lds_lm* lm, int B, int L, int max_length, size_t* out);
/* phone, tone, spk_id: dev int64 [B,L] (spk_id may be NULL) -> enc dev [B,L,hidden] = encoder_hidden_states (roformer.py:196-204).
 * enc_len: dev int32 [B] or NULL -- the padding mask of a right-padded batch (reference roformer.py:182,209-214: attention_mask), given as
 * the number of real positions per row: keys at positions >= enc_len[b] get probability 0 in every encoder self-attention. */
int lds_lm_encode(lds_lm* lm, const int64_t* phone, const int64_t* tone, const int64_t* spk_id, const int32_t* enc_len, float* enc, void* ws,
                  size_t ws_bytes, int B, int L, void* stream);
/* Roformer.generate (roformer.py:179-240): greedy (do_sample 0) or RepetitionPenalty -> Temperature -> TopK -> TopP -> one draw per
 * step.  enc_len as above (roformer.py:229-236: encoder_attention_mask on the decoder's cross-attention) or NULL.  top_k as HF's
 * TopKLogitsWarper: 1 .. 64 keeps the k largest scores AND every score tied with the k-th (up to 64 survivors in all); 0 (HF: None / 0) applies
 * no top-k filter -- softmax, the nucleus cut and the draw then run over the whole vocabulary (a slower, optional path).
 * uniforms dev [max_length-1][B]: the draw is the inverse-CDF rule over the vocabulary order with these numbers (torch's own
 * multinomial stream cannot be reproduced outside torch).  tokens dev int64 [B][max_length] (BOS first; finished sequences padded);
 * logits_out optional dev [max_length-1][B][sem_vocab]; *n_tokens_host = length of the returned sequences incl. BOS.  The call
 * synchronises the stream every 8 steps to poll for EOS. */
int lds_lm_generate(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, int max_length, int do_sample, int top_k, float top_p,
                    float temperature, float repetition_penalty, const float* uniforms, int64_t* tokens, float* logits_out, int* n_tokens_host,
                    void* ws, size_t ws_bytes, void* stream);

/* Decode options of lds_lm_generate_opts (HF GenerationConfig fields of reference roformer.py:216-227).
 *   num_beams 1: greedy (do_sample 0) or sampling as lds_lm_generate.  no_repeat_ngram_size n >= 1 adds HF's NoRepeatNGramLogitsProcessor
 *     between the repetition penalty and the temperature: a token that would complete an n-gram already in the sequence (BOS included)
 *     gets -inf; nothing is banned while the sequence is shorter than n.  0 = off (lds_lm_generate's kernels, bit for bit).
 *   num_beams 2 .. 8 with do_sample 0: HF's greedy beam search (_beam_search, length_penalty 1): log_softmax -> repetition penalty (on the
 *     log-probabilities) -> n-gram ban (each beam's own history) -> + running score -> top 2K of K * vocab (ties: the lower index beam * vocab
 *     + token) -> running beams and finished hypotheses with HF's -1e9 masks as fp32 additions -> early-stop heuristic.  early_stopping:
 *     1 = True (the reference's default), 0 = False, 2 = "never".  The result is each item's best finished hypothesis, cropped to the longest
 *     of them: BOS first, EOS kept, PAD after it.  Not built (LDS_EINVAL): beam sampling (num_beams > 1 with do_sample), logits_out with
 *     num_beams > 1.  Beam search limits: vocabularies of at most 4352 entries, max_length <= 8000.  top_k, top_p, temperature are read
 *     only when do_sample is set. */
typedef struct {
    int do_sample, top_k;
    float top_p, temperature, repetition_penalty;
    int no_repeat_ngram_size, num_beams, early_stopping;
} lds_lm_decode_opts;
/* workspace of lds_lm_generate_opts: num_beams * B decode rows (the cross-attention keys / values stay one set per item) plus the beam state */
int lds_lm_workspace_bytes_opts(const lds_lm* lm, int B, int L, int max_length, int num_beams, size_t* out);
/* lds_lm_generate with lds_lm_decode_opts (arguments as there; enc, enc_len one row per batch item, also with beams).  A bad option gives
 * LDS_EINVAL before anything is enqueued (the option checks come first and need no handle).  Beam search keeps the decode loop on the
 * stream as well: the synchronisation every 8 steps reads the search's per-step flags instead of the EOS flags. */
int lds_lm_generate_opts(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, int max_length, const lds_lm_decode_opts* opts,
                         const float* uniforms, int64_t* tokens, float* logits_out, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream);

/* Prompted decode: every row continues from semantic tokens it is given (reference roformer.py:235-242 calls semantic_decoder.generate, whose
 * HF GenerationMixin.generate takes the decoder prompt as input_ids=; the reference wrapper's **kwargs drop it).  Arguments as
 * lds_lm_generate_opts, plus:
 *   prompt dev int64 [B][P]: row b = BOS, s_1 .. s_{prompt_len[b]-1}, right-padded to P.  Ids are clamped to [0, sem_vocab) on the way in
 *     (callers validate the ids inside the lengths; lds.native's caller does); ids at and beyond prompt_len[b] are never looked at.
 *   prompt_len HOST int32 [B] (like `lengths` of the ragged sampler entries: the driver sizes the prefill and the step count from it) or
 *     NULL = P everywhere.  1 <= prompt_len[b] <= P and prompt_len[b] < max_length: max_length is the TOTAL length, prompt included, as in HF.
 *   tokens dev int64 [B][max_length]: the prompt, then the generated ids; EOS kept, PAD after it.  *n_tokens_host = the longest row's length.
 *   Row b's s-th generated token is drawn with uniforms[s][b] and chosen from logits_out[s][b] (both laid out [max_length-1][B] as there; the first
 *     max_length - min prompt_len steps are used); rows of logits_out at steps past a row's end are unspecified.  The repetition penalty and
 *     the n-gram ban see the whole history, prompt included (HF hands the full input_ids to the processors).
 * Each row equals that row run alone (B = 1, its own phones and prompt), tokens and logits bit for bit: a row's position, cache slot, key
 * count and history are its own.  The prompt's positions but the last go through ONE causal pass that fills the decode's key/value caches
 * (the arithmetic of the cached steps, as in lds_lm_score), then the decode continues step by step.  With prompt_len 1 everywhere the call
 * IS lds_lm_generate_opts (same launches; slot 0 gets the model's BOS id).  The contents of the workspace on entry do not matter.
 * Limits (LDS_EINVAL before anything is enqueued): B <= 64; num_beams 1 (beam search from a prompt is not built here: the ancestry tables
 * would need the prefix replicated per beam, or lds_llama_generate_beam's shared-prefix scheme); P <= 16000 and B * P <= 524280; max_length <= 16000.  A workspace smaller than
 * lds_lm_workspace_bytes_prompt(B, L, max_length, P) gives LDS_ENOMEM; with P = 1 that size is lds_lm_workspace_bytes_opts(.., 1, ..)'s. */
int lds_lm_workspace_bytes_prompt(const lds_lm* lm, int B, int L, int max_length, int P, size_t* out);
int lds_lm_generate_prompt(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, int max_length, const lds_lm_decode_opts* opts,
                           const int64_t* prompt, const int32_t* prompt_len, int P, const float* uniforms, int64_t* tokens, float* logits_out,
                           int* n_tokens_host, void* ws, size_t ws_bytes, void* stream);

/* Teacher-forced scoring: the log-probability, under the LM, of given semantic tokens at every position, in one causal pass over all
 * B * T decoder rows instead of T cached decode steps.  The logits at position t are those of the prefix semantic[:, :t + 1] -- what
 * lds_lm_generate computes at step t, bit for bit (the rows go through the decode's own linear kernels, and the causal self-attention
 * restates the cached step's arithmetic per row and head).
 *   enc dev [B][L][hidden] from lds_lm_encode, enc_len dev int32 [B] or NULL as there (the cross-attention's padding mask).
 *   semantic dev int64 [B][T], BOS first; sem_len dev int32 [B] (real tokens per right-padded row) or NULL = T everywhere;
 *   labels dev int64 [B][T] or NULL = semantic.  Position t of row b (0 <= t <= T - 2) is counted when t + 1 < sem_len[b] and
 *   y = labels[b][t + 1] != -100 (HF's shift and ignore index, ForCausalLMLoss); a label outside [0, sem_vocab) is ignored like -100.
 *   logprobs dev [B][T-1]:  logit_y - logsumexp_v logit_v  (max and sum of exp in a fixed order, the log in double, rounded once); 0 where not counted
 *   ranks dev int32 [B][T-1]:  #{v : logit_v > logit_y} + #{v < y : logit_v == logit_y}  (ties to the lowest index); -1 where not counted
 *   loss dev [1] = -(sum of the counted logprobs) / n_counted (HF's mean reduction; NaN when nothing is counted), n_counted dev int32 [1]:
 *     a fixed-order two-stage sum in double, no atomics -- every output is bit-identical on repeat.
 *   logits_out dev [B][T][sem_vocab] or NULL.  Without it the head runs over chunks of 256 rows through one reused buffer, so the
 *     workspace does not grow with B * T * sem_vocab.
 * Token ids are clamped to [0, sem_vocab) on the way into the embedding (callers validate the ids inside the lengths; lds.native's
 * wrapper does).  Ids, labels and logits rows at and beyond sem_len[b] have no effect on any counted output.  The contents of the
 * workspace on entry do not matter.  Nothing synchronises and nothing is copied from the host.  Limits (LDS_EINVAL before anything is
 * enqueued): 2 <= T <= min(max_position_embeddings, 16000), L as for lds_lm_generate_opts, B * T and B * L <= 524280.  A workspace
 * smaller than lds_lm_score_workspace_bytes(B, L, T) gives LDS_ENOMEM with the size needed in the message. */
int lds_lm_score_workspace_bytes(const lds_lm* lm, int B, int L, int T, size_t* out);
int lds_lm_score(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, const int64_t* semantic, const int32_t* sem_len,
                 const int64_t* labels, int T, float* logprobs, int32_t* ranks, float* loss, int32_t* n_counted, float* logits_out, void* ws,
                 size_t ws_bytes, void* stream);

/* ---- text2semantic, the second LM: a decoder-only Llama over one token stream (reference text2semantic/llama/llama.py:23-184 over HF transformers
 *      LlamaForCausalLM + GenerationMixin): [phone BOS, phones, phone EOS, semantic BOS, semantic tokens ...].  RMSNorm, bias-free projections with
 *      grouped-query attention (query head h reads kv head h / (heads / kv_heads)), rotary embedding in the half-split convention (element i pairs
 *      with i + head_dim / 2; default rope, the angle an fp32 product of position and inv_freq), SwiGLU MLP, untied head.  Everything fp32. ------- */
typedef struct lds_llama lds_llama;
/* llama.py:23-65: hidden .. max_pos, eps (rms_norm_eps), rope_theta are LlamaConfig's; vocab = len(symbols) + semantic_kmeans_num + 3;
 * first_free_id = semantic_token_shift (108): llama.py:170 bans every id below it (bad_words_ids), so the head computes the columns
 * first_free_id .. vocab only; bos / eos / pad = the config's ids (llama.py:56-58), inside those columns. */
typedef struct lds_llama_cfg { int hidden, heads, kv_heads, head_dim, inter, layers, vocab, max_pos; float eps, rope_theta; int first_free_id, bos, eos, pad; } lds_llama_cfg;
/* names = the reference Llama.state_dict() keys (llama.py:65: llama.model.embed_tokens.weight, llama.model.layers.N.{self_attn.{q,k,v,o}_proj,
 * mlp.{gate,up,down}_proj,input_layernorm,post_attention_layernorm}.weight, llama.model.norm.weight, llama.lm_head.weight), fp32 host arrays; a
 * missing one gives LDS_EMISSING naming it.  Optional: llama.model.rotary_emb.inv_freq [head_dim / 2], HF's own inverse frequencies (absent: powf).
 * Limits (LDS_EINVAL): head_dim a multiple of 16 in 16 .. 256; kv_heads divides heads; hidden <= 2048; inter and heads * head_dim <= 3840;
 * vocab - first_free_id <= 8192 (the token-choice kernels' columns). */
int  lds_llama_create(const lds_llama_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel, lds_llama** out);
void lds_llama_destroy(lds_llama* h);
int  lds_llama_workspace_bytes(const lds_llama* h, int B, int P, int max_length, size_t* out);
/* Llama.generate (llama.py:121-184; the reference can only do B = 1, llama.py:148) for num_beams 1: greedy, or HF's order per step on the raw logits of
 * the last position -- repetition penalty, n-gram ban (both over the WHOLE input_ids, phones included), the bad-word ban of the ids below
 * first_free_id (llama.py:170), temperature, top-k, top-p, one draw -- through the token-choice kernels of lds_lm_generate_prompt.
 *   input_ids dev int64 [B][P]: row b = its in_len[b] prompt ids (llama.py:148-152: [BOS, phones, EOS, semantic BOS]; any prefix of generated ids may
 *     follow), right-padded to P.  Ids are clamped to [0, vocab) on the way in; ids at and beyond in_len[b] are never looked at.
 *   in_len HOST int32 [B] or NULL = P everywhere; 1 <= in_len[b] <= P and in_len[b] < max_length (the TOTAL length, prompt included, as in HF).
 *   opts: lds_lm_decode_opts with num_beams 1.  uniforms dev [max_length-1][B] (sampling): row b's s-th generated token uses uniforms[s][b].
 *   tokens dev int64 [B][max_length]: the prompt, then the generated ids of the model's vocabulary (not shifted; llama.py:182 subtracts the shift), EOS
 *     kept, PAD after it.  logits_out optional dev [max_length-1][B][vocab - first_free_id]: HF's raw logits (before any processor) of the columns
 *     first_free_id .. vocab that chose row b's s-th generated token.  *n_tokens_host = the longest row's length.
 * One causal pass over the prompts' positions but the last fills the key/value caches (kv_heads of them per row), then the decode continues step by
 * step; prefill rows and decode steps run the same kernels, so a row equals that row run alone and a call continued from a longer prefix, tokens and
 * logits bit for bit.  The workspace's contents on entry do not matter.  The call synchronises the stream every 8 steps to poll for EOS.
 * Limits (LDS_EINVAL with a message before anything is enqueued): num_beams 1 (beam search is lds_llama_generate_beam: HF's log_softmax runs
 * over the whole vocabulary, banned columns included, which this entry's head does not form); B <= 64; P and max_length <= 15000; max_length <=
 * max_pos; the lds_lm_decode_opts checks of lds_lm_generate_opts.  A workspace smaller than lds_llama_workspace_bytes(B, P, max_length) gives
 * LDS_ENOMEM with the size needed. */
int  lds_llama_generate(lds_llama* h, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length, const lds_lm_decode_opts* opts,
                        const float* uniforms, int64_t* tokens, float* logits_out, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream);
/* Llama.generate with num_beams 2 .. 8 and do_sample 0: HF's greedy beam search (_beam_search, length_penalty 1) as lds_lm_decode_opts states it,
 * from a decoder prompt.  Row b's decoder_prompt_len is in_len[b] -- [BOS, phones, EOS, semantic BOS] plus any semantic prompt -- so a finished
 * hypothesis scores  sum / (length - in_len[b]),  the early-stop heuristic divides by the generated length (early_stopping 2, "never": by
 * max_length - in_len[b]) and max_length is the total length.  Per step and beam: log_softmax over the WHOLE vocabulary (the head's low
 * columns included, as in lds_llama_score) -> repetition penalty -> n-gram ban (both over the whole ids, phones included) -> -inf for every id
 * below first_free_id -> + the running score; ties go to the lower index beam * vocab + token.  early_stopping is the caller's (1 / 0 / 2).
 *   input_ids, in_len, B, P, max_length: as lds_llama_generate, one row per ITEM (not per beam).
 *   tokens dev int64 [B][max_length]: the prompt, then the item's best finished hypothesis, EOS kept, PAD after it.  *n_tokens_host = the longest row.
 * The prefill runs the B prompts once: all num_beams beams of an item read the positions below in_len[b] from the item's one prefilled cache row,
 * and an ancestry table over the generated positions tells the attention which beam row holds each later key.  Every item equals that item run
 * alone (B = 1), token for token: items reach max_length and the end of HF's loop at steps of their own, and an item whose loop has ended is
 * frozen.  The loop stays on the stream; every 8 steps the step's flag bits are polled, and the result does not depend on that interval.  The
 * workspace's contents on entry do not matter.
 * Limits (LDS_EINVAL with a message before anything is enqueued): the lds_lm_decode_opts checks; num_beams 2 .. 8; do_sample 0; B <= 64 and
 * B * num_beams <= 256; P <= 15000; max_length <= 7488 and <= max_pos; in_len as for lds_llama_generate; vocab <= 4352 and vocab - first_free_id
 * >= 2 * num_beams.  A workspace smaller than lds_llama_beam_workspace_bytes(B, P, max_length, num_beams) gives LDS_ENOMEM with the size needed. */
int  lds_llama_beam_workspace_bytes(const lds_llama* h, int B, int P, int max_length, int num_beams, size_t* out);
int  lds_llama_generate_beam(lds_llama* h, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length, const lds_lm_decode_opts* opts,
                             int64_t* tokens, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream);

/* Teacher-forced scoring under the Llama: what the reference's forward (llama.py:73-117) hands to LlamaForCausalLM with labels -- the logits of
 * every position of given streams in ONE causal pass, and HF's shifted cross entropy over the WHOLE vocabulary (ids below first_free_id
 * included: only generate bans them, llama.py:170) -- with lds_lm_score's outputs and definitions.  The rows go through the kernels of
 * lds_llama_generate (a row's position is all that tells a scoring row from a prefill row or a decode step), so the columns first_free_id ..
 * of the logits at position t equal what the decode computes there, bit for bit.
 *   input_ids dev int64 [B][S]: the streams (llama.py:98-101: [phone BOS, phones, phone EOS, semantic BOS, semantic ids + shift, semantic EOS]),
 *     right-padded; ids_len dev int32 [B] (real ids per row) or NULL = S everywhere.  Ids are clamped to [0, vocab) on the way into the
 *     embedding (callers validate the ids inside the lengths; lds.native's callers do).
 *   labels dev int64 [B][S] or NULL = input_ids (the loader's choice, text2semantic/llama/dataloader.py:182-183).  Position t of row b
 *     (0 <= t <= S - 2) is counted when t + 1 < ids_len[b] and y = labels[b][t + 1] lies in [0, vocab); -100 (HF's ignore index) and every
 *     other id outside are ignored.
 *   logprobs dev [B][S-1]:  logit_y - logsumexp_v logit_v over v in [0, vocab)  (max and sum of exp in a fixed order, the log in double,
 *     rounded once); 0 where not counted.   ranks dev int32 [B][S-1]:  #{v : logit_v > logit_y} + #{v < y : logit_v == logit_y}; -1 where not counted.
 *   loss dev [1] = -(sum of the counted logprobs) / n_counted (llama.py:103-117's outputs.loss, HF's mean reduction; NaN when nothing is
 *     counted), n_counted dev int32 [1]: a fixed-order two-stage sum in double, no atomics -- every output is bit-identical on repeat.
 *   logits_out dev [B][S][vocab] or NULL.  Without it the head runs over chunks of 256 rows through one reused buffer, so the workspace does
 *     not grow with B * S * vocab.
 * Slots at and beyond ids_len[b] are filled from PAD, as in the prefill; ids, labels and logits rows there have no effect on any counted
 * output.  The contents of the workspace on entry do not matter.  Nothing synchronises and nothing is copied from the host.  Limits
 * (LDS_EINVAL with a message before anything is enqueued): B >= 1, 2 <= S <= min(max_position_embeddings, 15000), B * S <= 524280.  A workspace
 * smaller than lds_llama_score_workspace_bytes(B, S) gives LDS_ENOMEM with the size needed in the message. */
int  lds_llama_score_workspace_bytes(const lds_llama* h, int B, int S, size_t* out);
int  lds_llama_score(lds_llama* h, const int64_t* input_ids, const int32_t* ids_len, const int64_t* labels, int B, int S, float* logprobs, int32_t* ranks,
                     float* loss, int32_t* n_counted, float* logits_out, void* ws, size_t ws_bytes, void* stream);

/* ---- speech to text: Whisper's text decoder on the native audio encoder (OpenAI whisper/model.py TextDecoder; the reference's
 *      encoder/whisper/model.py:85-110 ResidualAttentionBlock(cross_attention=True) and :150-154 Whisper.logits / Whisper.forward, which
 *      end in a `self.decoder` that it never builds; csrc/whisper_dec.hip; tests/whisper_decoder_numpy.py is the float64 restatement) ---------
 * cfg: large-v3 is {51866, 448, 1280, 20, 32, 1500}.  Limits (LDS_EINVAL): n_state a multiple of 64 (<= 8192) with n_state / n_head == 64,
 * 1 <= n_layer <= 64, 2 <= n_text_ctx <= 448, 1 <= n_audio_ctx <= 1500, 2 <= n_vocab <= 2^20.
 * names: OpenAI Whisper's own checkpoint keys, fp32 host arrays in that layout: "decoder.token_embedding.weight" [n_vocab][n_state],
 * "decoder.positional_embedding" [n_text_ctx][n_state], "decoder.blocks.N.{attn,cross_attn}.{query,value,out}.{weight,bias}",
 * "decoder.blocks.N.{attn,cross_attn}.key.weight" (no bias), "decoder.blocks.N.{attn_ln,cross_attn_ln,mlp_ln}.{weight,bias}",
 * "decoder.blocks.N.mlp.{0,2}.{weight,bias}", "decoder.ln.{weight,bias}"; a missing tensor gives LDS_EMISSING naming it.  The head is the
 * token embedding transposed (tied): the handle keeps the embedding twice, [n_vocab][n_state] for the look-up and [n_state][n_vocab] for
 * the head's column walk, n_vocab * n_state * 4 bytes each (266 MB each at large-v3 and 3.89 GB for the whole handle, both in units of 10^6 / 10^9 bytes).
 *
 * One workspace serves the three calls; lds_whisper_decoder_workspace_bytes(h, B, T, S) sizes it for B rows, T encoder frames and S text
 * positions (a scoring pass's S, a decode's cap).  Its first part depends on B and T alone and holds what lds_whisper_decoder_cross leaves
 * for the other two: the clips' frame counts and every layer's cross-attention keys and values, 2 * n_layer * B * T * n_state * 4 bytes
 * (491 MB per 30 s clip at large-v3).  So: cross once per batch of clips, then any number of logits / generate calls with the SAME
 * workspace, B and T.  The rest of the workspace's contents on entry do not matter to any call.  A small workspace gives LDS_ENOMEM with
 * the size needed in the message; a bad argument returns before anything is enqueued.
 *
 * Exact fp32; one fixed-order accumulation per output that does not depend on the batch size; no floating-point atomics, so a repeat gives
 * the same bits; a row of a batch equals that row run alone (B = 1, its own n_frames and prompt), tokens and log-probs bit for bit; a
 * prefill row and a decode step go through the same kernels, so generate's logits_out equals logits on the produced sequence bit for bit.
 * Whisper's d^-0.25 scaling of q and of k is applied once to their product (0.125 at d = 64, exact).
 * Not built (LDS_EINVAL): sampling and temperature fallback, beam search, timestamp rules (ApplyTimestampRules), word alignment from
 * alignment_heads, long-form windows, fp16, and a no-repeat n-gram ban (lm.hip's bit set spans 8192 columns, not this vocabulary). */
typedef struct lds_whisper_decoder lds_whisper_decoder;
typedef struct lds_whisper_decoder_cfg { int n_vocab, n_text_ctx, n_state, n_head, n_layer, n_audio_ctx; } lds_whisper_decoder_cfg;
int  lds_whisper_decoder_create(const lds_whisper_decoder_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs,
                                const int64_t* numel, lds_whisper_decoder** out);
void lds_whisper_decoder_destroy(lds_whisper_decoder* h);
/* B 1 .. 64, T 1 .. n_audio_ctx, S 2 .. n_text_ctx */
int  lds_whisper_decoder_workspace_bytes(const lds_whisper_decoder* h, int B, int T, int S, size_t* out);
/* units dev [B][T][n_state], the encoder's output (lds_whisper_encode's layout); n_frames host int32 [B] (1 <= n_frames[b] <= T) or NULL
 * (T everywhere).  Every layer's cross key and value rows, once per call, into the workspace.  Nothing at or beyond n_frames[b] is read
 * (NaN included), and keys stop at n_frames[b] in every later step.  Takes any workspace of lds_whisper_decoder_workspace_bytes(h, B, T, S >= 2).
 * n_frames is read during the call only; nothing synchronises. */
int  lds_whisper_decoder_cross(lds_whisper_decoder* h, const float* units, const int32_t* n_frames, int B, int T, void* ws, size_t ws_bytes,
                               void* stream);
/* Whisper.logits: tokens dev int64 [B][S] (ids clamped to the vocabulary), tok_len dev int32 [B] or NULL (S everywhere; rows at and beyond
 * tok_len[b] are computed from id 0 and mean nothing) -> logits dev [B][S][n_vocab] or NULL, from ONE causal pass over all B * S rows.
 * Optionally logprobs / ranks dev [B][S-1], loss / n_counted dev [1] (all four or none) with exactly lds_lm_score's definitions over the
 * whole vocabulary, labels dev int64 [B][S] or NULL (= tokens): position t predicts labels[b][t + 1], counted when t + 1 < tok_len[b] and
 * the label lies in [0, n_vocab).  With logits NULL the rows go through a buffer of 64 rows and B * S * n_vocab floats are never stored.
 * 2 <= S <= n_text_ctx.  Nothing synchronises. */
int  lds_whisper_decoder_logits(lds_whisper_decoder* h, const int64_t* tokens, const int32_t* tok_len, const int64_t* labels, int B, int S, int T,
                                float* logits, float* logprobs, int32_t* ranks, float* loss, int32_t* n_counted, void* ws, size_t ws_bytes,
                                void* stream);
/* Greedy decode.  suppress / begin_suppress: dev int32 lists; a listed id gets -inf at every step / at each row's first generated step only
 * (HF's SuppressTokensLogitsProcessor / SuppressTokensAtBeginLogitsProcessor); ids outside the vocabulary are ignored.  num_beams must be
 * 1, temperature 0 and no_repeat_ngram_size 0 (above). */
typedef struct lds_whisper_decode_opts {
    int max_new_tokens, eos, pad, no_repeat_ngram_size;
    const int32_t* suppress;
    const int32_t* begin_suppress;
    int n_suppress, n_begin_suppress;
    int num_beams;
    float temperature;
} lds_whisper_decode_opts;
/* prompt dev int64 [B][P] with host int32 prompt_len[B] (1 .. P): <|startoftranscript|><|lang|><|transcribe|><|notimestamps|>, behind an
 * optional <|startofprev|> prefix.  The prompt's positions but the last go through one causal prefill into the self-attention caches, then
 * come cached steps.  cap (P < cap <= n_text_ctx): the sequences' capacity; row b stops at EOS, after max_new_tokens ids or at position
 * cap, whichever comes first.
 * -> tokens dev int64 [B][cap]: the prompt, then the generated ids, EOS kept, PAD after it;  token_logprob dev [B][max_new_tokens]: the
 * chosen id's log-softmax over the unsuppressed columns (max and sum in a fixed order), 0 behind a row's end;  sum_logprob dev [B] or NULL;
 * logits_out dev [max_new_tokens][B][n_vocab] or NULL: the raw logits of every step run (before the suppress lists; a finished row's are
 * computed and mean nothing);  *n_tokens_host: the longest row's length, prompt included.
 * Synchronises: before the first launch (prompt_len), at the EOS poll every 8 steps and at the end. */
int  lds_whisper_decoder_generate(lds_whisper_decoder* h, const int64_t* prompt, const int32_t* prompt_len, int B, int P, int T, int cap,
                                  const lds_whisper_decode_opts* opts, int64_t* tokens, float* token_logprob, float* sum_logprob, float* logits_out,
                                  int* n_tokens_host, void* ws, size_t ws_bytes, void* stream);

/* ---- k-means semantic tokenizer: units -> tokens and the codebook fit (reference cluster/__init__.py:13-23 get_cluster_result /
 *      get_cluster_center_result, cluster/kmeans.py:10-50 _kpp, :108-131 euc_sim / max_sim, :184-198 the Lloyd step; called from
 *      17_preprocess_train_cluster.py and 19_preprocess_token.py) -------------------------------------------------------------------
 * Stateless helpers.  X dev [N][D] and C dev [K][D] are plain row-major fp32 (units as they are at the module boundary and on disk).
 * Limits, checked before anything is enqueued (LDS_EINVAL with a message): D a multiple of 8 in 8 .. 4096, 1 <= K <= 65,536,
 * 1 <= N <= 2,147,483,000 (all row addressing is 64-bit), K <= N for seeding, no NULL pointer except where noted; a workspace smaller
 * than lds_kmeans_workspace_bytes(N, K, D) gives LDS_ENOMEM.  One workspace size serves all calls of the same (N, K, D); its contents
 * on entry do not matter.  Nothing synchronises.  No floating-point atomics: every call is bit-identical on repeat. */
int lds_kmeans_workspace_bytes(int64_t N, int K, int D, size_t* out);
/* The metric of the lds_kmeans_*_metric, lds_knn_*_metric and lds_ivf_*_metric entries (any other value: LDS_EINVAL).  Each of those entries is its
 * namesake with `int metric` added (and `int weights` where a blend follows); with LDS_METRIC_L2 (and LDS_WEIGHTS_INVERSE_SQUARE) it IS its
 * namesake, bit for bit -- the namesakes forward.  LDS_METRIC_COSINE, all fp32:
 *   row constant  r(v) = 1 / max(sqrt(s), 1e-12), s = the fp32 sum of squares of the row in one fixed order (lanes of a wave stride the columns,
 *                 one fmaf chain per lane, a fixed butterfly), square root and reciprocal correctly rounded: F.normalize's eps.  s = 4, 16, 64
 *                 give exactly 1/2, 1/4, 1/8.  A zero row has r = 1e12 and scores 0 against everything; nothing gives NaN for finite rows.
 *                 LIMIT: a row whose s overflows fp32 (|v| beyond about 1.8e19) is outside the contract (r = 0: it scores 0 or NaN).
 *   score         (x_n . p_m) r_m: the dot product is the L2 score's fmaf chain, the per-row array `h` holds r_m where it holds |p_m|^2 / 2
 *                 for L2.  Order: descending score, the lower index among exactly equal scores (rows that are scaled copies by powers of
 *                 two tie exactly).  The value REPORTED (search's score, assign's best) is that score times r(x_n), multiplied after the
 *                 order is decided: the cosine similarity.
 *   distance      of a chosen neighbour, recomputed directly: d_j = 1/2 sum_c (x_c r_x - p_jc r_j)^2 (= 1 - cos) in one fixed order,
 *                 floored at 1e-12.
 * No second copy of any pool is made; no floating-point atomics; every call is bit-identical on repeat whatever the workspace held. */
#define LDS_METRIC_L2 0
#define LDS_METRIC_COSINE 1
/* the weights of a blend: (1 / d_j)^2 normalised for j ascending (the RVC / Diffusion-SVC tool chains), or w_j = 1 / found over the
 * neighbours actually present (kNN-VC's plain mean of the matched rows) */
#define LDS_WEIGHTS_INVERSE_SQUARE 0
#define LDS_WEIGHTS_UNIFORM 1
/* h dev [K] = |c_k|^2 / 2 (once per codebook; lds_kmeans_update refreshes it) */
int lds_kmeans_prepare(const float* C, int K, int D, float* h, void* stream);
/* cosine: h dev [K] = r(c_k).  Replaces the b side of the reference's cos_sim (kmeans.py:96-105 normalize(b, dim=-1)) without a normalised copy */
int lds_kmeans_prepare_metric(const float* C, int K, int D, int metric, float* h, void* stream);
/* labels dev int64 [N]: label[n] = argmax_k (x_n . c_k - h_k) = the nearest centre (scikit-learn's predict; the arg-max of the reference's
 * euc_sim), the LOWEST index among exactly equal scores; best dev [N] or NULL = the winning score (|x_n|^2 - 2 best = squared distance).
 * Exact fp32 on the MFMA; the N x K matrix is never stored.  A row's label depends on that row and the codebook only: not on N, the row's
 * position or the other rows (NaN / Inf there included). */
int lds_kmeans_assign(const float* X, int64_t N, const float* C, const float* h, int K, int D, int64_t* labels, float* best, void* ws, size_t ws_bytes,
                      void* stream);
/* cosine: label[n] = argmax_k (x_n . c_k) r_k, best = the cosine similarity.  Replaces KMeansGPU(mode='cosine').max_sim (kmeans.py:117-131 over
 * cos_sim :96-105) */
int lds_kmeans_assign_metric(const float* X, int64_t N, const float* C, const float* h, int K, int D, int metric, int64_t* labels, float* best, void* ws,
                             size_t ws_bytes, void* stream);
/* the same over a ragged batch X dev [B][T][D]: lengths host int32 [B] (B <= 64, 0 <= lengths[b] <= T); rows t >= lengths[b] get pad_id (a
 * 32-bit value; best = 0 there) whatever they hold.  Workspace of N = B * T. */
int lds_kmeans_assign_ragged(const float* X, int B, int T, const int32_t* lengths, int64_t pad_id, const float* C, const float* h, int K, int D,
                             int64_t* labels, float* best, void* ws, size_t ws_bytes, void* stream);
/* the ragged form of lds_kmeans_assign_metric (max_sim per clip; padded rows: pad_id, best = 0, whatever they hold) */
int lds_kmeans_assign_ragged_metric(const float* X, int B, int T, const int32_t* lengths, int64_t pad_id, const float* C, const float* h, int K, int D,
                                    int metric, int64_t* labels, float* best, void* ws, size_t ws_bytes, void* stream);
/* One Lloyd step given labels (kmeans.py:185-198): c_grad = per-cluster mean (an empty cluster: a zero row), *error (dev float) =
 * sum (c_grad - C)^2, lr = 1 / num_points * 0.9 + 0.1, C = C (1 - lr) + c_grad lr in place, then num_points (dev [K]) += the counts and h
 * refreshed.  The sums run in row order per cluster (a stable counting sort of the rows by label), the error in a fixed order.  Rows whose
 * label is outside [0, K) are ignored. */
int lds_kmeans_update(const float* X, const int64_t* labels, int64_t N, float* C, float* h, float* num_points, int K, int D, float* error, void* ws,
                      size_t ws_bytes, void* stream);
/* the same step -- the reference's Lloyd step (kmeans.py:185-198) is the plain mean and the same lr in both modes -- refreshing h as
 * lds_kmeans_prepare_metric(metric) of the new centres, bit for bit */
int lds_kmeans_update_metric(const float* X, const int64_t* labels, int64_t N, float* C, float* h, float* num_points, int K, int D, int metric,
                             float* error, void* ws, size_t ws_bytes, void* stream);
/* k-means++ seeding (kmeans.py:42-49): C[0] = X[first_index]; for i >= 1 the weight of a point is its Euclidean DISTANCE (not squared, as
 * the reference's cdist) to the nearest centre picked so far (a running minimum, fp32), and C[i] = X[j], j = the first index whose
 * prefix sum reaches uniforms[i - 1] * total -- the prefix in double in a fixed order -- clamped to N - 1 (the reference raises there).
 * uniforms dev [K - 1] (may be NULL when K = 1); picked dev int64 [K] or NULL receives the indices.  K dependent steps, all on the stream. */
int lds_kmeans_seed(const float* X, int64_t N, int D, int K, int64_t first_index, const float* uniforms, float* C, int64_t* picked, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- units retrieval: exact k-NN over a speaker's unit pool and the blend of the nearest rows (csrc/knn.hip) -----------------------------
 * The reference has no retrieval step; this replaces the host-side approximate faiss index ("units index", index.search + the inverse-square
 * weighting of the squared distances) that the Diffusion-SVC / RVC tool chains the reference was forked from run on the units before
 * Unit2Mel (reference tools/infer_tools.py:83-117 is where the units pass; 22_infer_tts.py:43-52,106 the codebook gather they follow in TTS).
 * Here the search is exact and on the device.  Stateless helpers: X dev [N][D] queries and P dev [M][D] the pool, plain row-major fp32,
 * 16-byte aligned.
 *   score(n, m) = x_n . p_m - h_m, h_m = |p_m|^2 / 2: lds_kmeans_assign's score on the fp32 MFMA (its arg-max is the arg-min of the squared
 *   distance).  Every score of a query row is the same fmaf chain whatever N, the row's position, the slab or the split: duplicated pool rows
 *   tie exactly, and a row's neighbours depend on that row and the pool only.  The k best come in descending score order, the LOWER pool
 *   index first among equal scores.  The N x M matrix is never stored.
 * Limits, checked before anything is enqueued (LDS_EINVAL with a message): D a multiple of 8 in 8 .. 4096, 1 <= k <= 8 and k <= M,
 * 1 <= M <= 16,777,216 (indices are int32; the pool is addressed in slabs of at most 2^31 bytes), 1 <= N <= 2,147,483,000, ratio in [0, 1]
 * and not NaN, no NULL pointer except where noted; a workspace smaller than lds_knn_workspace_bytes(N, M, D, k) gives LDS_ENOMEM.  The
 * contents of the workspace on entry do not matter.  Nothing synchronises.  No floating-point atomics: every call is bit-identical on repeat. */
/* h dev [M] = |p_m|^2 / 2 (once per pool) */
int lds_knn_prepare(const float* P, int64_t M, int D, float* h, void* stream);
/* cosine: h dev [M] = r(p_m).  Replaces kNN-VC's normalised copy of the matching set (its fast_cosine_dist's norms) */
int lds_knn_prepare_metric(const float* P, int64_t M, int D, int metric, float* h, void* stream);
int lds_knn_workspace_bytes(int64_t N, int64_t M, int D, int k, size_t* out);
/* idx dev int32 [N][k] = the k nearest pool rows of every query, nearest first; score dev [N][k] or NULL = their scores
 * (|x_n|^2 - 2 score = squared distance).  A query without k comparable scores (a NaN row) gets -1 in the missing places. */
int lds_knn_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int32_t* idx, float* score, void* ws,
                   size_t ws_bytes, void* stream);
/* cosine: the k rows of highest cosine similarity, score = the similarities (-inf in a missing place).  Replaces kNN-VC's
 * fast_cosine_dist(...).topk(k, largest=False) */
int lds_knn_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int metric, int32_t* idx, float* score,
                          void* ws, size_t ws_bytes, void* stream);
/* Y dev [N][D]: the search, then for the k winners d_j = sum_c (x_c - p_jc)^2 recomputed directly (not from |x|^2 - 2 score) in fp32 in one
 * fixed order, d_j = max(d_j, 1e-12), w_j = (1 / d_j)^2 normalised by their sum taken for j ascending, z = sum_j w_j p_j (fmaf, j ascending),
 * y_n = (1 - ratio) x_n + ratio z.  ratio = 0 gives x bit for bit, ratio = 1 with k = 1 the pool row bit for bit.  idx dev int32 [N][k] and
 * dist dev [N][k] (the floored d_j), either may be NULL.  Every gathered index is clamped into [0, M) before it forms an address. */
int lds_knn_retrieve(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, float ratio, float* Y, int32_t* idx,
                     float* dist, void* ws, size_t ws_bytes, void* stream);
/* the search by `metric`, the distances by `metric` (cosine: 1 - cos as above; h is then read by the blend too), the weights by `weights`, and
 * the unchanged blend y = (1 - ratio) x + ratio sum_j w_j p_j over the ORIGINAL pool rows, j ascending, with fmaf.  A query without
 * neighbours (a NaN row) has found = 0.  cosine + uniform + ratio 1 + k 4 replaces kNN-VC's match (the mean of the matched rows) */
int lds_knn_retrieve_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, int metric, int weights, float ratio,
                            float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);
/* the same over a ragged batch X dev [B][T][D]: lengths host int32 [B] (B <= 64, 0 <= lengths[b] <= T); rows t >= lengths[b] get y = 0,
 * idx = -1 and dist = 0 whatever they hold.  Workspace of N = B * T. */
int lds_knn_retrieve_ragged(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                            float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);
/* the ragged form of lds_knn_retrieve_metric (kNN-VC's match per clip) */
int lds_knn_retrieve_ragged_metric(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                                   int metric, int weights, float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);

/* ---- units retrieval through an IVF coarse index: probe nprobe lists, not the pool (csrc/knn.hip) ------------------
 * What faiss IndexIVFFlat is to the RVC / Diffusion-SVC tool chains (index.nprobe = 1 .. 16 there; IndexIVFFlat::train / add build the
 * lists, IndexIVFFlat::search probes them): the pool's rows are grouped by their nearest coarse centre and a query is scored against the
 * rows of its nprobe best centres only.  Each entry takes the arguments of its lds_knn_* counterpart and adds the index:
 *   C dev [nlist][D], hc dev [nlist] = lds_knn_prepare(C): the coarse centres, 1 <= nlist <= 65,536 (lds_kmeans_assign's codebook limit;
 *     pool row m belongs to the list lds_kmeans_assign gives it).  faiss: the quantizer of IndexIVFFlat.
 *   offsets dev int64 [nlist + 1], order dev int32 [M]: list l holds the pool rows order[offsets[l] .. offsets[l + 1]), in ascending original
 *     index; offsets[0] = 0, offsets[nlist] = M.  faiss: the inverted lists' ids.
 *   PL dev [copy_rows][D], hl dev [copy_rows]: the pool and its h in list order, every list padded to whole 128-row blocks (list l starts
 *     at row 128 sum_{j < l} ceil(len_j / 128); what the padding rows hold does not matter), copy_rows = 128 sum_l ceil(len_l / 128): at
 *     most M + 127 nlist rows, one more pool.  faiss: the inverted lists' codes.  The original P stays: the blend reads it by original index.
 *   nprobe in 1 .. min(8, nlist).
 * A query's probed lists are lds_knn_search(X, C, hc, k = nprobe), its candidates the rows of those lists, its result the k best candidates
 * by lds_knn_search's score and order (every score is the same fmaf chain as there), the lower ORIGINAL index first among equal scores;
 * indices are original pool indices.  A query with fewer than k candidates gets -1 / -inf in the missing places of the search; the blend
 * gives such places the weight 0 and normalises over the ones found.  Distances, weights, blend and the ragged form are lds_knn_retrieve's.
 * lds_ivf_search does not read P and h (they may be NULL); lds_ivf_retrieve* do not read h.
 * Limits as for lds_knn_* (LDS_EINVAL with a message before anything is enqueued), and: nlist <= M; copy_rows a multiple of 128 in
 * M .. M + 127 nlist; N D 4 <= 2,147,418,112 bytes (the gathered query operand sits behind one buffer descriptor: split longer inputs);
 * C and PL 16-byte aligned.  A workspace smaller than lds_ivf_workspace_bytes gives LDS_ENOMEM naming the size.  On the device the offsets
 * are checked (start at 0, never decrease, end at M, and pad to exactly copy_rows rows): a table that fails gives every query -1
 * everywhere; every value read from `order` is clamped into [0, M) -- nothing a corrupt table holds leads outside the buffers.  The (query,
 * list) pairs are grouped by list with integer atomics; no result depends on the slot a pair lands in, there are no floating-point atomics
 * and every call is bit-identical on repeat.  The contents of the workspace on entry do not matter.  Nothing synchronises.  A long list is
 * walked in up to 8 block ranges by separate workgroups; the workspace holds 8 nprobe result lists per query. */
int lds_ivf_workspace_bytes(int64_t N, int64_t M, int D, int k, int nlist, int nprobe, size_t* out);
/* replaces IndexIVFFlat::search */
int lds_ivf_search(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, const float* C, const float* hc, int nlist,
                   const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe, int32_t* idx,
                   float* score, void* ws, size_t ws_bytes, void* stream);
/* replaces IndexIVFFlat::search + the tool chains' inverse-square weighting of the rows it returns */
int lds_ivf_retrieve(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, const float* C, const float* hc, int nlist,
                     const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe, float ratio,
                     float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);
int lds_ivf_retrieve_ragged(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                            const float* C, const float* hc, int nlist, const int64_t* offsets, const int32_t* order, const float* PL,
                            const float* hl, int64_t copy_rows, int nprobe, float ratio, float* Y, int32_t* idx, float* dist, void* ws,
                            size_t ws_bytes, void* stream);
/* The same three with the metric (and the weights): C / hc, PL / hl and P / h are then one index built for that metric -- hc, hl and h from
 * lds_knn_prepare_metric, the lists assigned by lds_kmeans_assign_metric.  In cosine mode lds_ivf_retrieve*_metric READ h (the blend's r_j).
 * replaces IndexIVFFlat::search over an inner-product quantizer on normalised rows (faiss METRIC_INNER_PRODUCT), without the normalised copy */
int lds_ivf_search_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, const float* C, const float* hc, int nlist,
                          const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe, int metric,
                          int32_t* idx, float* score, void* ws, size_t ws_bytes, void* stream);
/* replaces that search + kNN-VC's mean (or the tool chains' inverse-square weighting) of the rows it returns */
int lds_ivf_retrieve_metric(const float* X, int64_t N, const float* P, const float* h, int64_t M, int D, int k, const float* C, const float* hc, int nlist,
                            const int64_t* offsets, const int32_t* order, const float* PL, const float* hl, int64_t copy_rows, int nprobe, int metric,
                            int weights, float ratio, float* Y, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);
int lds_ivf_retrieve_ragged_metric(const float* X, int B, int T, const int32_t* lengths, const float* P, const float* h, int64_t M, int D, int k,
                                   const float* C, const float* hc, int nlist, const int64_t* offsets, const int32_t* order, const float* PL,
                                   const float* hl, int64_t copy_rows, int nprobe, int metric, int weights, float ratio, float* Y, int32_t* idx,
                                   float* dist, void* ws, size_t ws_bytes, void* stream);

/* ---- polyphase sinc resampler in front of the audio encoders (reference torchaudio.transforms.Resample(orig_freq, new_freq) with its
 *      defaults sinc_interp_hann / lowpass_filter_width 6 / rolloff 0.99, i.e. torchaudio's _get_sinc_resample_kernel +
 *      _apply_sinc_resample_kernel; called from tools/tools.py:78-84 Units_Encoder.encode, diffusion/vocoder.py:24-27 Vocoder.extract and
 *      batch_proccessor/semantic_extract.py:49-68) ------------------------------------------------------------------------------------
 * Stateless.  With O = orig / gcd, N = new / gcd a clip x[0 .. len) (zero outside) gives ceil(N len / O) samples
 *   y[m] = sum_n x[n] g(n / O - m / N) = sum_{k < taps} x[(m / N) O + first[m % N] + k] bankT[k][m % N]
 * bankT dev [taps][N] fp32 (tap-major) and first dev int32 [N] are the filter of one (orig, new, width, rolloff), evaluated in float64 on the
 * host and rounded once (lds/arch.py resample_bank): first[i] = the first sample, relative to (m / N) O, inside the filter's support at
 * phase i; the columns outside the support are left out (each below 1e-30).  One fmaf chain per output in tap order, all index arithmetic in
 * integers (64-bit where m O needs it), no atomics: y[b] depends on x[b, :len] alone and is bit-identical on repeat, at any batch position
 * and in either entry.  Nothing synchronises, no workspace.  Limits, checked before anything is enqueued (LDS_EINVAL with a message):
 * 1 <= O, N <= 384,000; 1 <= taps <= 1024; N taps <= 2^24; 1 <= L <= 2^30; at most 2^31 - 1 output samples per clip; B <= 65,535
 * (lds_resample) or B <= 64 (lds_resample_ragged); no NULL pointer except new_lengths.  A bank of more than 8192 entries is read from
 * global memory instead of LDS (16000 -> 44101: 44,101 x 13); a pair whose 64 outputs need more than 8192 input samples runs a
 * one-thread-per-output kernel (same bits). */
/* x dev [B][L] -> y dev [B][M], M = ceil(N L / O) exactly (anything else is LDS_EINVAL) */
int lds_resample(const float* x, float* y, const float* bankT, const int32_t* first, int O, int N, int taps, int B, int64_t L, int64_t M,
                 void* stream);
/* Ragged batch: lengths host int32 [B] (B <= 64, 0 <= lengths[b] <= L) = every clip's own sample count inside x [B][L].  Clip b is
 * resampled as if alone: samples at and beyond lengths[b] are never read into a result (NaN / Inf included), y[b][m] = 0 for
 * m >= ceil(N lengths[b] / O); M >= the largest of those is the row length of y.  new_lengths host int64 [B] or NULL receives
 * ceil(N lengths[b] / O).  With every length equal to L and M = ceil(N L / O) the result is lds_resample's, bit for bit. */
int lds_resample_ragged(const float* x, const int32_t* lengths, float* y, int64_t* new_lengths, const float* bankT, const int32_t* first, int O,
                        int N, int taps, int B, int64_t L, int64_t M, void* stream);

/* ---- long-audio conversion: slicing, volume mask, per-clip alignment and the cross-fading join (csrc/svc.hip) -------------------------
 * The device side of DiffusionSVC.infer_from_long_audio (reference tools/infer_tools.py:83-117).  fp32 in and out, no atomics: a repeat
 * gives the same bits; nothing synchronises; a bad argument is LDS_EINVAL with a message before anything is enqueued.  The two mean
 * squares (lds_frame_rms, lds_volume_extract) are summed in fp64 and rounded to fp32 once, after the root.
 *
 * lds_frame_rms: librosa.feature.rms(y, frame_length, hop_length, center=True) as the slicer calls it (reference tools/slicer.py:40):
 * rms[t] = sqrt(mean_{i < fl} xp[t hop + i]^2), xp = x padded by fl / 2 on both sides with zeros (pad_mode 0, librosa >= 0.10's
 * default) or by reflection (pad_mode 1); n = 1 + (L + 2 (fl / 2) - fl) / hop exactly.  x dev [L] -> rms dev [n].  Every frame is summed
 * in a fixed order; a workgroup squares its samples once, whatever the overlap of the frames. */
int lds_frame_rms(const float* x, float* rms, int64_t L, int frame_length, int hop_length, int pad_mode, int64_t n, void* stream);
/* Volume_Extractor.extract (reference tools/tools.py:23-33): x dev [L] -> volume dev [n], n = int(L // hop) + 1 exactly with Python's
 * float floor division; volume[k] = sqrt(mean(x2p[int(k hop) : int((k + 1) hop)])), x2p = x^2 reflect-padded by
 * (int(hop // 2), int((hop + 1) // 2)), the slice's end clipped to the padded length, the bounds computed in fp64 as Python does.
 * hop_size: host pointer to the hop as a double (block_size * sr / model_sampling_rate: fractional when the rates differ), >= 1.
 * L > int((hop + 1) // 2). */
int lds_volume_extract(const float* x, float* volume, int64_t L, const double* hop_size, int64_t n, void* stream);
/* get_mask_from_volume + upsample (reference tools/tools.py:35-41, 225-229): volume dev [n] -> mask dev [n * factor];
 * m[k] = volume[k] > threshold, M[k] = max m[max(k - 4, 0) .. min(k + 4, n - 1)] (the reference's edge-replicated window of 9),
 * mask[j] = M[i] (1 - f) + M[min(i + 1, n - 1)] f with i = j / factor, f = (j % factor) / factor. */
int lds_volume_mask(const float* volume, float* mask, int64_t n, int factor, float threshold, void* stream);
/* lds_resample_frames per clip (units_forced_alignment, reference tools/tools.py:193-223, on a ragged batch): in dev [B,Tin,C], host int32
 * tin[B] (1 .. Tin) and tout[B] (0 .. Tout), B <= 64 -> out dev [B,Tout,C]: out[b,i,:] = in[b, min((int)floorf(i step_b), tin[b] - 1), :]
 * for i < tout[b], zeros beyond; step_b = (float)tin[b] / (float)tout[b].  Rows of `in` at and beyond tin[b] are never read. */
int lds_resample_frames_ragged(const float* in, const int32_t* tin, const int32_t* tout, float* out, int B, int Tin, int Tout, int C,
                               void* stream);
/* The mask product, the zero gaps and cross_fade of the reference's loop (tools/infer_tools.py:105-115, tools/tools.py:231-238) in one
 * pass.  segs dev [segs_len]: the S segments packed; table int64 [3][S] = offset (into segs), start (in the result) and len of every
 * segment, given twice: host_tab is validated, dev_tab (the same values on the device) is what the kernel reads.  mask dev [mask_len] or
 * NULL; out dev [N], N = start[S-1] + len[S-1] exactly.  Defined by the sequential loop: R = the result so far,
 * v_s = seg_s * mask[start_s : start_s + len_s]; start_s >= |R|: R is extended by zeros up to start_s, then by v_s; else with
 * F = |R| - start_s and k_i = i / (F - 1) (0 when F = 1): R[start_s + i] = (1 - k_i) R[start_s + i] + k_i v_s[i] for i < F, and the rest
 * of v_s is appended.  Preconditions (LDS_EINVAL naming the segment): start never decreases; F <= len_s;
 * start_s >= start_{s-2} + len_{s-2}; offset_s + len_s <= segs_len; mask_len >= N.  At most two segments then meet at a sample, and every
 * output sample evaluates the loop's closed form on its own. */
int lds_overlap_assemble(const float* segs, int64_t segs_len, const int64_t* host_tab, const int64_t* dev_tab, int S, const float* mask,
                         int64_t mask_len, float* out, int64_t N, void* stream);

/* ---- CTC heads on the speech encoders: transcribe, score, align (csrc/ctc.hip; tests/ctc_numpy.py is the float64 restatement) -----------
 * The reference has no CTC code; this replaces transformers' Wav2Vec2ForCTC / HubertForCTC / WavLMForCTC head (lm_head over the last hidden
 * state, .logits / .loss), torch.nn.functional.ctc_loss, the greedy collapse of Wav2Vec2CTCTokenizer and torchaudio-style forced alignment.
 * Stateless helpers, all fp32:
 *   X dev [B][T][D]: units in the encode_ragged layout; n_frames host int32 [B], B <= 64, 0 <= n_frames[b] <= T.  Rows t >= n_frames[b]
 *     are never read, whatever they hold (NaN included).
 *   W dev [V][D], bias dev [V]: HF's lm_head.weight / lm_head.bias; blank in [0, V): HF's config.pad_token_id.
 * Limits, checked before anything is enqueued (LDS_EINVAL with a message): D a multiple of 8 in 8 .. 4096, 2 <= V <= 65,536, 1 <= T,
 * B * T <= 2^31 - 1000, 1 <= Lmax <= 511 (a batch of empty transcripts passes Lmax = 1), no NULL pointer except where noted; a workspace
 * smaller than the entry's *_workspace_bytes gives LDS_ENOMEM with the size needed in the message.  Nothing synchronises.  No
 * floating-point atomics: every call is bit-identical on repeat whatever the workspace held.
 *   head    z[n][v] = x_n . w_v + b_v, exact fp32 on the MFMA (one fmaf chain per (n, v), the same for all).  Per valid frame:
 *           arg = the argmax over v, the LOWEST id among exactly equal logits; m = z[arg]; lse = m + log sum_v exp(z_v - m).  exp never
 *           sees a positive argument; the (max, rescaled sum) pairs of column tiles and column splits merge in one fixed order that
 *           depends on V alone, so a frame's outputs depend on that frame and the head only: not on B, T, its position or other rows.
 *           Padded rows: arg = -1, m = lse = 0.  The N x V matrix is never stored unless logprobs_out (dev [B][T][V]) is given: then
 *           z - lse is also written, zeros in padded rows.
 *   greedy  collapse runs of equal arg, drop blank.  Per clip: tokens int64 [T] padded with pad_id, n_tokens, and per emitted token
 *           start (first frame of its run), length (run length), logprob (the mean of m - lse over the run, summed in double); beyond
 *           n_tokens: start = -1, length = 0, logprob = 0.  It reads lds_ctc_head's outputs and needs no workspace.
 *   score   labels dev int64 [B][Lmax], label_len host int32 [B] (0 <= label_len[b] <= Lmax): nll[b] = -log p(labels_b | X_b) by the CTC
 *           forward recursion in log space = F.ctc_loss(log_probs, .., blank, reduction='none', zero_infinity=False).  Infeasible
 *           (n_frames < L + the number of adjacent equal labels): +inf.  L = 0: -sum_t logp(blank).  n_frames = 0: 0 if L = 0, else +inf.
 *           A label outside [0, V) or equal to blank: that clip's nll is +inf and nothing outside W is read.  The emissions are computed
 *           for the clip's L + 1 distinct columns only (W's rows gathered by label).
 *   align   the Viterbi path of the same trellis (states 0 .. 2 L: blank, label 0, blank, ..; a path starts in state 0 or 1 and ends in
 *           state 2 L or 2 L - 1).  Ties between predecessors: prefer STAY, then STEP (from the state below), then SKIP (from two below,
 *           allowed into a label that differs from the label before); equal final states: the blank.  path_score[b] = the path's
 *           log-probability (-inf if infeasible or a bad label); frame_label int32 [B][T] = index into the clip's labels, -1 on blank
 *           frames and beyond n_frames; segments int32 [B][Lmax][2] = (first frame, one past the last frame) of each label's non-blank
 *           frames, (-1, -1) if infeasible or beyond label_len; label_logprob [B][Lmax] = the mean emission over those frames (0 where
 *           there are none). */
int lds_ctc_head_workspace_bytes(int B, int T, int V, int D, size_t* out);
int lds_ctc_head(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int32_t* arg, float* m, float* lse,
                 float* logprobs_out, void* ws, size_t ws_bytes, void* stream);
/* arg, m, lse dev [B][T]: lds_ctc_head's outputs (any int32 ids in general); every output dev [B][T] but n_tokens dev int32 [B] */
int lds_ctc_greedy(const int32_t* arg, const float* m, const float* lse, int B, int T, const int32_t* n_frames, int blank, int64_t pad_id, int64_t* tokens,
                   int32_t* n_tokens, int32_t* start, int32_t* length, float* logprob, void* stream);
int lds_ctc_score_workspace_bytes(int B, int T, int V, int D, int Lmax, size_t* out);
int lds_ctc_score(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int blank, const int64_t* labels,
                  const int32_t* label_len, int Lmax, float* nll, void* ws, size_t ws_bytes, void* stream);
int lds_ctc_align_workspace_bytes(int B, int T, int V, int D, int Lmax, size_t* out);
int lds_ctc_align(const float* X, int B, int T, const int32_t* n_frames, const float* W, const float* bias, int V, int D, int blank, const int64_t* labels,
                  const int32_t* label_len, int Lmax, float* path_score, int32_t* frame_label, int32_t* segments, float* label_logprob, void* ws,
                  size_t ws_bytes, void* stream);

/* ---- x-vector speaker embeddings (csrc/xvector.hip; tests/xvector_numpy.py is the float64 restatement) -------------------------------------
 * The reference has no speaker-verification code; this replaces the head of transformers' WavLMForXVector / Wav2Vec2ForXVector (transformers
 * 5.15 modeling_wavlm.py: TDNNLayer.forward 1491-1498; WavLMForXVector.forward 1591-1621 -- projector and the tdnn loop 1599-1602, the
 * statistics pooling without an attention_mask 1605-1607, feature_extractor and classifier 1620-1621; _get_tdnn_output_lengths 1541-1554 is the
 * masked path that is not reproduced) and torch.nn.functional.cosine_similarity.  The AM-softmax objective (AMSoftmaxLoss, 1446) is training: not built.
 *   X dev [B][T][d_in]: hidden states in the encode_ragged layout (the last hidden state, or lds_wavlm_encode_layersum's output when the
 *     checkpoint has use_weighted_layer_sum); n_frames host int32 [B], B <= 64, n_frames[b] <= T <= 32,768.  Rows t >= n_frames[b] are never
 *     read, whatever they hold (NaN included).  Every clip is treated as if given alone with attention_mask = None.  HF's batched masked path
 *     is NOT reproduced: its _get_tdnn_output_lengths ignores the dilations, so it pools T - 8 frames of a tensor that holds T - 14 valid ones.
 *   projector   x = h W^T + b, Linear(d_in -> tdnn_dim[0]), no activation.
 *   tdnn.{i}    y[t][o] = relu(b[o] + sum_{j < ks} sum_{c < Cin} x[t + j d][c] W[o][j Cin + c]), W = tdnn.{i}.kernel.weight [out][ks Cin] as
 *               stored; valid convolution: T_out = T_in - (ks - 1) d.  (TDNNLayer.forward: conv1d of the transposed, viewed weight.)
 *   pooling     per channel the mean and the unbiased standard deviation (torch.std, ddof 1) over the clip's T_out frames of the last layer,
 *               concatenated [2 tdnn_dim[-1]].  The last layer's output is never stored: every 64-frame run becomes (mean, M2) in frame
 *               order and the runs are combined in order by Chan's update.  A clip needs T_out >= 2 (16 frames with the default geometry,
 *               5,200 samples): fewer is LDS_EINVAL naming the count, never a NaN.  A constant channel has a standard deviation of exactly 0.
 *   tail        emb = feature_extractor(stats) [xvector_dim]; logits = classifier(emb) [n_labels = numel(classifier.bias)].
 *   cosine      out[i][j] = a_i . b_j / (max(|a_i|, 1e-8) max(|b_j|, 1e-8)), a dev [N][dim], b dev [M][dim], out dev [N][M].
 * Every GEMM is exact fp32 on the MFMA, one fmaf chain per output in k order; no floating-point atomics.  A clip's embedding is bit-identical
 * alone, at any batch position, with any other clips, for any T and on repeat, whatever the workspace held.
 * Tensor names are the head's keys in *ForXVector.state_dict(): projector.{weight,bias}, tdnn.{i}.kernel.{weight,bias},
 * feature_extractor.{weight,bias} (top level: not the encoder's <prefix>.feature_extractor.conv_layers.*), classifier.{weight,bias}; objective.* and
 * other names are not read.  LDS_EMISSING names a missing tensor.
 * Limits, checked before anything is enqueued (LDS_EINVAL with a message): 1 <= n_tdnn <= 8; d_in and every layer's input width a multiple of
 * 32 (the K-step: a K-block may not span two taps) up to 4096; every tdnn_dim and xvector_dim a multiple of 4 up to 4096; kernels and
 * dilations in 1 .. 8; no NULL pointer except logits.  A workspace smaller than lds_xvector_workspace_bytes gives LDS_ENOMEM naming the size.
 * Nothing synchronises. */
typedef struct lds_xvector lds_xvector;
typedef struct lds_xvector_cfg { int d_in, n_tdnn, tdnn_dim[8], tdnn_kernel[8], tdnn_dilation[8], xvector_dim; } lds_xvector_cfg;
int  lds_xvector_create(const lds_xvector_cfg* cfg, int n_tensors, const char* const* names, const float* const* host_ptrs, const int64_t* numel, lds_xvector** out);
void lds_xvector_destroy(lds_xvector* h);
int  lds_xvector_n_labels(const lds_xvector* h);
int  lds_xvector_workspace_bytes(const lds_xvector* h, int B, int T, size_t* out);
/* emb dev [B][xvector_dim]; logits dev [B][n_labels] or NULL */
int  lds_xvector_embed(lds_xvector* h, const float* X, const int32_t* n_frames, float* emb, float* logits, void* ws, size_t ws_bytes, int B, int T, void* stream);
int  lds_xvector_cosine(const float* a, int N, const float* b, int M, int dim, float* out, void* stream);

/* ---- per-launch HIP-event timing for bench.py's roofline leg (off by default) ------------------
 * lds_prof_enable(1) clears and starts recording one event pair per kernel launch on the launch
 * stream; lds_prof_summary synchronises them and writes a JSON list of
 * {name,count,ms,flops,bytes} aggregates (algorithmic flops/bytes per kernel family). */
int lds_prof_enable(int on);
int lds_prof_summary(char* buf, size_t cap);

/* ---- exact-fp32 vs split-operand GEMMs on the 16-bit matrix pipe (csrc/conv_bf3.hip, csrc/k8b3.h) ------------------------------------
 * mode 0 (default, what bench.py's `value` is measured in): every convolution / linear layer of the UNet on the exact-fp32 MFMA (a k-ordered
 * fmaf chain).
 * mode 1 (three bf16 terms per operand, lossless, six products) was a whole-UNet mode in round 3 and is REMOVED: it met the tolerances and ran no
 * faster than mode 0; lds_unet_set_gemm_mode(1) returns LDS_EINVAL.  The kernel format survives for the single-op probes
 * (include/lds_test.h lds_test_dconv_split, tools/split_bf16_probe.py).
 * mode 2 (opt-in, experimental, never a default): two fp16 terms per operand -- 22 significand bits, NARROWER than the reference's fp32 -- three
 * products, fp32 accumulate; weights carry a per-layer power-of-two scale.  PRECONDITION on the activations: every tensor between kernels must
 * stay below 65,504 in magnitude (an overflow becomes an infinity, then a NaN: loud) and should live at a scale of 2^-3 or more: below that
 * the second fp16 term is subnormal and the tensor keeps fewer than 22 bits (down to 11 at 6e-5), silently.  Attention probabilities are
 * exempt (formed times 2^12 inside the kernel).  UNet1DConditionModel.check_split_f16_ranges (Python) reports every tensor's range for given
 * inputs and raises outside [2^-3, 2^15].  The first switch packs the split weights (host work + upload); later switches only flip the flag.
 * Switching modes is not thread-safe against concurrent forwards on the same handle (one mode per handle lifetime is the supported use). */
#define LDS_GEMM_F32 0
#define LDS_GEMM_SPLIT_BF16 1      /* removed: LDS_EINVAL */
#define LDS_GEMM_SPLIT_F16 2
int lds_unet_set_gemm_mode(lds_unet* u, int mode);
int lds_unet_get_gemm_mode(const lds_unet* u);

/* ---- latency mode (off by default): the one-sentence caller (reference 22_infer_tts.py:100-114 synthesises one utterance per call) ----
 * By default every tile / split choice is made at the nominal per-GPU batch of 16, so that an utterance's result is bit-identical
 * alone, inside any batch and for any shard count -- at the price that one utterance occupies 1/16 of the chip.  With the mode on the
 * choices follow the ACTUAL batch: smaller tiles, and for deep reductions a cluster of up to 16 workgroups per output tile, each
 * reducing a share of the K range and the last one to arrive summing the partial tiles in a fixed order (deterministic; csrc/conv_dma.hip
 * cluster_join).  Same tolerances against the reference; results are NOT bit-identical with the default mode's.  The workspace grows by
 * 16 MB (lds_unet_workspace_bytes / lds_sampler_workspace_bytes report it).  Applies to every GEMM mode. */
int lds_unet_set_latency_mode(lds_unet* u, int on);
int lds_unet_get_latency_mode(const lds_unet* u);

#ifdef __cplusplus
}
#endif
#endif /* LDS_H */
