"""ctypes binding of liblds.so (include/lds.h).  PyTorch is used only to own device memory and
the HIP stream; every arithmetic op of the hot path runs inside the library.  There is no CPU
fallback: if the shared object is missing or a tensor is not on a HIP device the call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblds.so")
_lib = None

METHODS = {"dpm-solver": 1, "unipc": 2, "ddpm": 3, "ddim": 4, "pndm": 5}
TABLE_STRIDE = 16


class UNetCfg(C.Structure):
    _fields_ = [("out_dims", C.c_int), ("n_hidden", C.c_int), ("n_layers", C.c_int), ("n_heads", C.c_int),
                ("norm_groups", C.c_int), ("n_blocks", C.c_int), ("block_out_channels", C.c_int * 8)]


class VocoderCfg(C.Structure):
    _fields_ = [("inter_channels", C.c_int), ("upsample_initial_channel", C.c_int), ("n_ups", C.c_int),
                ("upsample_rates", C.c_int * 8), ("upsample_kernel_sizes", C.c_int * 8), ("resblock", C.c_int),
                ("n_kernels", C.c_int), ("resblock_kernel_sizes", C.c_int * 4), ("n_dil", C.c_int),
                ("resblock_dilation_sizes", (C.c_int * 4) * 4)]


class LMCfg(C.Structure):
    _fields_ = [("hidden", C.c_int), ("heads", C.c_int), ("inter", C.c_int), ("enc_layers", C.c_int), ("dec_layers", C.c_int),
                ("text_vocab", C.c_int), ("type_vocab", C.c_int), ("sem_vocab", C.c_int), ("n_spk_rows", C.c_int), ("max_pos", C.c_int),
                ("eps", C.c_float), ("sem_bos", C.c_int), ("sem_eos", C.c_int), ("sem_pad", C.c_int)]


class LMDecodeOpts(C.Structure):
    _fields_ = [("do_sample", C.c_int), ("top_k", C.c_int), ("top_p", C.c_float), ("temperature", C.c_float), ("repetition_penalty", C.c_float),
                ("no_repeat_ngram_size", C.c_int), ("num_beams", C.c_int), ("early_stopping", C.c_int)]


class WhisperCfg(C.Structure):
    _fields_ = [("n_mels", C.c_int), ("n_state", C.c_int), ("n_head", C.c_int), ("n_layer", C.c_int), ("n_ctx", C.c_int)]


class WhisperDecoderCfg(C.Structure):
    _fields_ = [("n_vocab", C.c_int), ("n_text_ctx", C.c_int), ("n_state", C.c_int), ("n_head", C.c_int), ("n_layer", C.c_int),
                ("n_audio_ctx", C.c_int)]


class WhisperDecodeOpts(C.Structure):
    _fields_ = [("max_new_tokens", C.c_int), ("eos", C.c_int), ("pad", C.c_int), ("no_repeat_ngram_size", C.c_int), ("suppress", C.c_void_p),
                ("begin_suppress", C.c_void_p), ("n_suppress", C.c_int), ("n_begin_suppress", C.c_int), ("num_beams", C.c_int),
                ("temperature", C.c_float)]


EARLY_STOPPING = {True: 1, False: 0, "never": 2}


class ConvTest(C.Structure):
    _fields_ = [("x1", C.c_void_p), ("x2", C.c_void_p), ("C1", C.c_int), ("C2", C.c_int), ("Tsrc", C.c_int),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("Co", C.c_int), ("K", C.c_int), ("pad", C.c_int), ("dil", C.c_int),
                ("act_in", C.c_int), ("slope", C.c_float), ("res", C.c_void_p), ("epilogue", C.c_int), ("tile", C.c_int)]


class DConvTest(C.Structure):
    _fields_ = [("x1", C.c_void_p), ("x2", C.c_void_p), ("C1", C.c_int), ("C2", C.c_int), ("T", C.c_int),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("Co", C.c_int), ("K", C.c_int), ("stride", C.c_int),
                ("pad", C.c_int), ("ups", C.c_int), ("res", C.c_void_p), ("epilogue", C.c_int), ("plain_out", C.c_int),
                ("v_split", C.c_int), ("cfg", C.c_int)]


class DConvExTest(C.Structure):
    _fields_ = [("x1", C.c_void_p), ("x2", C.c_void_p), ("C1", C.c_int), ("C2", C.c_int), ("T", C.c_int),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("Co", C.c_int), ("K", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
                ("res", C.c_void_p), ("epilogue", C.c_int), ("lengths", C.c_void_p), ("lvl_in", C.c_int), ("lvl_out", C.c_int),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("tile_batch", C.c_int), ("fmt", C.c_int),
                ("v_split", C.c_int), ("cfg", C.c_int)]


# The C ABI, one line per entry point: name, return kind ':' argument kinds in the header's order.
# Arguments: p pointer (any sort, c_void_p), i int, z size_t, f float, q int64_t, u uint32_t.  Returns: i int, v void, s const char*.
_KIND = {"p": C.c_void_p, "i": C.c_int, "z": C.c_size_t, "f": C.c_float, "q": C.c_int64, "u": C.c_uint32}
_RETURN = {"i": C.c_int, "v": None, "s": C.c_char_p}
_PUBLIC = """
lds_last_error                   s:
lds_version                      i:
lds_unet_create                  i:pipppp
lds_unet_destroy                 v:p
lds_unet_workspace_bytes         i:piip
lds_unet_forward                 i:ppppppziip
lds_sampler_run                  i:piipppppziip
lds_sampler_workspace_bytes      i:piip
lds_unet_forward_ragged          i:pppppppziip
lds_sampler_run_ragged           i:piippppppziip
lds_embed_create                 i:iiipppp
lds_embed_destroy                v:p
lds_embed_workspace_bytes        i:piip
lds_embed_forward                i:pppppziip
lds_transpose                    i:ppiiifp
lds_gather_rows                  i:pppiiip
lds_resample_frames              i:ppiiiifp
lds_axpby                        i:pppffqp
lds_q_sample_rows                i:ppppppipiqp
lds_loss_reduce_workspace_bytes  i:qp
lds_loss_reduce                  i:ppqippzp
lds_stft_mel_workspace_bytes     i:iiiiqp
lds_stft_mel                     i:ppppiiiiiifippziqp
lds_vocoder_create               i:pipppp
lds_vocoder_destroy              v:p
lds_vocoder_workspace_bytes      i:piip
lds_vocoder_forward              i:ppppziip
lds_vocoder_forward_ragged       i:pppppziip
lds_vae_encoder_create           i:pipppp
lds_vae_encoder_destroy          v:p
lds_vae_encoder_workspace_bytes  i:piqp
lds_vae_encoder_forward          i:pppppipziqp
lds_vae_encoder_forward_ragged   i:ppppppipziqp
lds_whisper_create               i:pippppp
lds_whisper_destroy              v:p
lds_whisper_workspace_bytes      i:piqp
lds_whisper_logmel               i:pppppziqp
lds_whisper_encode_mel           i:pppppziip
lds_whisper_encode               i:pppppziqp
lds_hubert_create                i:pipppp
lds_hubert_destroy               v:p
lds_hubert_workspace_bytes       i:piqip
lds_hubert_features              i:pppppziqip
lds_hubert_encode                i:ppppiipziqip
lds_w2v_create                   i:pipppp
lds_w2v_destroy                  v:p
lds_w2v_workspace_bytes          i:piqp
lds_w2v_features                 i:pppppziqp
lds_w2v_encode                   i:pppppziqp
lds_wavlm_create                 i:pipppp
lds_wavlm_destroy                v:p
lds_wavlm_workspace_bytes        i:piqp
lds_wavlm_features               i:ppppipziqp
lds_wavlm_encode                 i:ppppiipziqp
lds_w2vbert_create               i:pipppp
lds_w2vbert_destroy              v:p
lds_w2vbert_workspace_bytes      i:piqp
lds_w2vbert_fbank                i:pppppziqp
lds_w2vbert_encode_features      i:pppppziip
lds_w2vbert_encode               i:pppppziqp
lds_lm_create                    i:pipppp
lds_lm_destroy                   v:p
lds_lm_workspace_bytes           i:piiip
lds_lm_encode                    i:pppppppziip
lds_lm_generate                  i:pppiiiiifffpppppzp
lds_lm_workspace_bytes_opts      i:piiiip
lds_lm_generate_opts             i:pppiiippppppzp
lds_lm_workspace_bytes_prompt    i:piiiip
lds_lm_generate_prompt           i:pppiiipppipppppzp
lds_lm_score_workspace_bytes     i:piiip
lds_lm_score                     i:pppiipppippppppzp
lds_llama_create                 i:pipppp
lds_llama_destroy                v:p
lds_llama_workspace_bytes        i:piiip
lds_llama_generate               i:pppiiippppppzp
lds_llama_beam_workspace_bytes   i:piiiip
lds_llama_generate_beam          i:pppiiippppzp
lds_llama_score_workspace_bytes  i:piip
lds_llama_score                  i:ppppiippppppzp
lds_whisper_decoder_create       i:pipppp
lds_whisper_decoder_destroy      v:p
lds_whisper_decoder_workspace_bytes i:piiip
lds_whisper_decoder_cross        i:pppiipzp
lds_whisper_decoder_logits       i:ppppiiippppppzp
lds_whisper_decoder_generate     i:pppiiiipppppppzp
lds_kmeans_workspace_bytes       i:qiip
lds_kmeans_prepare               i:piipp
lds_kmeans_prepare_metric        i:piiipp
lds_kmeans_assign                i:pqppiipppzp
lds_kmeans_assign_metric         i:pqppiiipppzp
lds_kmeans_assign_ragged         i:piipqppiipppzp
lds_kmeans_assign_ragged_metric  i:piipqppiiipppzp
lds_kmeans_update                i:ppqpppiippzp
lds_kmeans_update_metric         i:ppqpppiiippzp
lds_kmeans_seed                  i:pqiiqppppzp
lds_knn_prepare                  i:pqipp
lds_knn_prepare_metric           i:pqiipp
lds_knn_workspace_bytes          i:qqiip
lds_knn_search                   i:pqppqiipppzp
lds_knn_search_metric            i:pqppqiiipppzp
lds_knn_retrieve                 i:pqppqiifppppzp
lds_knn_retrieve_metric          i:pqppqiiiifppppzp
lds_knn_retrieve_ragged          i:piipppqiifppppzp
lds_knn_retrieve_ragged_metric   i:piipppqiiiifppppzp
lds_ivf_workspace_bytes          i:qqiiiip
lds_ivf_search                   i:pqppqiippippppqipppzp
lds_ivf_search_metric            i:pqppqiippippppqiipppzp
lds_ivf_retrieve                 i:pqppqiippippppqifppppzp
lds_ivf_retrieve_metric          i:pqppqiippippppqiiifppppzp
lds_ivf_retrieve_ragged          i:piipppqiippippppqifppppzp
lds_ivf_retrieve_ragged_metric   i:piipppqiippippppqiiifppppzp
lds_ctc_head_workspace_bytes     i:iiiip
lds_ctc_head                     i:piipppiipppppzp
lds_ctc_greedy                   i:pppiipiqpppppp
lds_ctc_score_workspace_bytes    i:iiiiip
lds_ctc_score                    i:piipppiiippippzp
lds_ctc_align_workspace_bytes    i:iiiiip
lds_ctc_align                    i:piipppiiippipppppzp
lds_wavlm_encode_layersum        i:pppppipziqp
lds_xvector_create               i:pipppp
lds_xvector_destroy              v:p
lds_xvector_n_labels             i:p
lds_xvector_workspace_bytes      i:piip
lds_xvector_embed                i:ppppppziip
lds_xvector_cosine               i:pipiipp
lds_resample                     i:ppppiiiiqqp
lds_resample_ragged              i:ppppppiiiiqqp
lds_frame_rms                    i:ppqiiiqp
lds_volume_extract               i:ppqpqp
lds_volume_mask                  i:ppqifp
lds_resample_frames_ragged       i:ppppiiiip
lds_overlap_assemble             i:pqppipqpqp
lds_prof_enable                  i:i
lds_prof_summary                 i:pz
lds_unet_set_gemm_mode           i:pi
lds_unet_get_gemm_mode           i:p
lds_unet_set_latency_mode        i:pi
lds_unet_get_latency_mode        i:p
"""
# include/lds_test.h: single-op entry points for tests/ and tools/ (not part of the drop-in boundary)
_TEST = """
lds_test_conv                    i:ppip
lds_test_dconv                   i:pppip
lds_bench_dconv                  i:ppiippzp
lds_test_gn_apply                i:ppiiiifpppipip
lds_bench_gn_stream              i:iiiiipp
lds_test_gn_chain_k4p            i:pppppfiippiiiiip
lds_test_ln_chain_k4p            i:pppppfppiiiip
lds_test_attention_k4p           i:ppiiiip
lds_test_conv_transpose          i:ppppiiiiiiifp
lds_test_voc_step                i:pppppiiiiipfppip
lds_test_dconv_bf3               i:pppiip
lds_bench_dconv_bf3              i:ppiiippzp
lds_test_k8b3_roundtrip          i:ppiiip
lds_test_gn_apply_bf3            i:ppiiiifpppipip
lds_test_dconv_split             i:pppiiip
lds_bench_dconv_split            i:ppiiiippzp
lds_test_split_roundtrip         i:ppiiiip
lds_test_gn_apply_split          i:ppiiiifpppipiip
lds_debug_set_split_rule         i:i
lds_test_attention_f16math       i:ppiiiip
lds_test_attention_latency       i:ppiiiiip
lds_test_attention_ragged        i:pppiiiiiip
lds_debug_set_gn_fold            i:i
lds_debug_set_voc_pair           i:i
lds_debug_set_touch_weights      i:i
lds_test_voc_pair                i:pppppiiiipfppip
lds_test_gn_fold_k4p             i:pppppfippppiiiiiiip
lds_bench_dconv_alt              i:ppiipipp
lds_debug_fill_u32               i:pzup
lds_debug_trace                  i:i
lds_debug_trace_count            i:
lds_debug_trace_get              i:ipzpp
lds_debug_unet_plan              i:piipz
lds_test_gn_fold_split           i:pppppfippppiiiiiiiiip
lds_test_cluster_join            i:ppppiiiiiiippppzp
lds_test_lm_sample               i:piiiifffppipp
lds_test_conv_down               i:pppiiiiiifippzp
lds_test_conv_down_ragged        i:pppiiiiiifppippzp
lds_test_lm_beam_step            i:piiiiiifiippppppppppppppppp
lds_test_llama_beam_step         i:piiiiiifiiipppppppppppppppppppp
lds_test_llama_beam_attn         i:pppppiiiiiiiipp
lds_test_llama_generate_beam_poll i:pppiiippppzpi
lds_test_whisper_head            i:ppppiiipippppp
lds_test_dconv_pair              i:pppppppiiiiiipiiipppzp
lds_test_dconv_ex                i:pppipzp
lds_test_dma_magic_div           i:uup
lds_test_dma_tile_order          i:iiiip
lds_test_tap_k4p                 i:pz
lds_test_voc_ups                 i:pppiiiiiipppppzp
lds_test_w2v_conv0               i:ppppppfpiiqp
lds_test_w2v_ln_act              i:ppppfppiiip
lds_test_w2vbert_fbank           i:pppiqp
lds_test_w2vbert_attention       i:pppppiiiiiip
lds_test_w2vbert_dwconv          i:ppppfpppiiiip
lds_test_wavlm_attention         i:pppppiiiiip
lds_test_wavlm_buckets           i:iiip
lds_test_stft_dft                i:pppiiiippiqp
lds_test_knn_search              i:pqppqiiiipppzp
lds_test_knn_search_metric       i:pqppqiiiiipppzp
lds_test_ivf_search              i:pqppqiippippppqiipppzp
lds_test_ivf_search_metric       i:pqppqiippippppqiiipppzp
lds_test_ctc_forward             i:piipppipp
lds_test_ctc_viterbi             i:piipppipppppzp
lds_test_xvector_tdnn            i:piipppiiiiipp
lds_test_xvector_pool_workspace_bytes i:iiip
lds_test_xvector_pool            i:piipppiiiipppzp
lds_test_wino_pack               i:piip
lds_test_wino_conv               i:ppiiipppiippippiipppip
lds_bench_wino                   i:ppiiipppiippipiiiipppzp
lds_test_wino_conv_lvl           i:ppiiipppiippippiiipppip
lds_test_wino_min_T              i:ii
lds_test_wino_pair_pack          i:ppiiip
lds_test_wino_pair               i:pppiiiipppppipppppiiippppip
lds_bench_wino_pair              i:pppiiiipppppippppiiiipppzp
lds_test_wino_pair_min_T         i:ii
"""
SIGNATURES = dict(ln.split() for ln in (_PUBLIC + _TEST).splitlines() if ln)
EXPORTS = [ln.split()[0] for ln in _PUBLIC.splitlines() if ln]
TEST_EXPORTS = [ln.split()[0] for ln in _TEST.splitlines() if ln]


def lib():
    """Load liblds.so (once) and declare restype / argtypes of every name in EXPORTS + TEST_EXPORTS.  Raises if it has not been built
    (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C latent-diffusion-speech_amd/csrc` "
                               "(there is no CPU fallback for the hot path)")
        L = C.CDLL(LIB_PATH)
        for n in EXPORTS + TEST_EXPORTS:
            ret, _, args = SIGNATURES[n].partition(":")
            fn = getattr(L, n)
            fn.restype, fn.argtypes = _RETURN[ret], [_KIND[k] for k in args]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(f"liblds error {rc}: {lib().lds_last_error().decode()}")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=None):
    """Device pointer of a contiguous tensor that must live on the GPU."""
    import torch
    if not t.is_cuda:
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    if not t.is_contiguous():
        raise RuntimeError("liblds needs contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def _host_tensor_table(state):
    """state: name -> fp32 numpy/torch (CPU).  Returns ctypes arrays + keep-alive list."""
    names, ptrs, numel, keep = [], [], [], []
    for k, v in state.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        a = np.ascontiguousarray(a, dtype=np.float32)
        keep.append(a)
        names.append(k.encode())
        ptrs.append(a.ctypes.data)
        numel.append(a.size)
    n = len(names)
    return (n, (C.c_char_p * n)(*names), (C.c_void_p * n)(*ptrs), (C.c_int64 * n)(*numel), keep)


class Workspace:
    """Growable device scratch owned by torch: one buffer per (handle, HIP stream), grown on demand.  The library's handles are immutable
    after create, so calls on different streams may overlap as long as each has its own workspace (include/lds.h) -- which is what keying
    the buffer by the current stream gives (infer_tts.synthesize_ragged runs length buckets on several streams)."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes, device):
        import torch
        key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


def _dev_or_null(t, dtype=None):
    return None if t is None else _dev(t, dtype)


def _host(a):
    """address of a host numpy array (the caller keeps it alive over the call), or NULL"""
    return None if a is None else a.ctypes.data


def _bytes(entry, *args):
    """what the `*_workspace_bytes` entry answers for these arguments"""
    nb = C.c_size_t()
    check(getattr(lib(), entry)(*args, C.byref(nb)))
    return nb.value


def _host_lengths(lengths, B, lo, hi, max_B=None, what=""):
    """the per-item counts of a ragged batch (list / array / tensor) -> host int32 [B], every one in lo .. hi; max_B: the most items (`what`
    names them in the message) that the entry takes"""
    if max_B is not None and B > max_B:
        raise ValueError(f"a ragged {what} batch holds at most {max_B} clips (got {B})")
    a = np.ascontiguousarray(np.asarray(lengths.cpu() if hasattr(lengths, "cpu") else lengths).reshape(-1), dtype=np.int32)
    if a.shape != (B,) or a.min() < lo or a.max() > hi:
        raise ValueError(f"lengths must be {B} integers in {lo} .. {hi}")
    return a


def _dense_or_ragged(name, *lengths, suffix=""):
    """(the entry `name`, ()) without lengths, else (its `_ragged` twin, the host addresses of the lengths arrays -- which the caller keeps
    alive over the call).  The C entries stay two: a ragged one refuses a null `lengths`.  suffix: what follows `_ragged` in the name."""
    if lengths[0] is None:
        return getattr(lib(), name + suffix), ()
    return getattr(lib(), name + "_ragged" + suffix), tuple(a.ctypes.data for a in lengths)


# the metric / weights choices of the clustering stack (include/lds.h LDS_METRIC_*, LDS_WEIGHTS_*)
METRICS = {"l2": 0, "cosine": 1}
WEIGHTS = {"inverse_square": 0, "uniform": 1}


def metric_code(metric, what="metric", table=None):
    """the C value of a metric (or, with table=WEIGHTS, a weights) name; anything else is a ValueError -- before any device work"""
    table = METRICS if table is None else table
    if not isinstance(metric, str) or metric not in table:
        raise ValueError(f"{what} must be one of {sorted(table)} (got {metric!r})")
    return table[metric]


class _Handle:
    """What the handle classes share: `h` from lds_<KIND>_create, destroyed with the object, and `ws`, the scratch of its calls."""
    KIND = None

    def _create(self, *args):
        self.h, self.ws = C.c_void_p(), Workspace()
        check(getattr(lib(), f"lds_{self.KIND}_create")(*args, C.byref(self.h)))

    def _create_weights(self, cfg, state, *more):
        n, names, ptrs, numel, keep = _host_tensor_table(state)
        self._create(C.byref(cfg), n, names, ptrs, numel, *more)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            getattr(_lib, f"lds_{self.KIND}_destroy")(self.h)
            self.h = None

    def _workspace(self, entry, device, *dims):
        """the buffer of the current stream, grown to what `entry` asks for a call of these dimensions"""
        return self.ws.get(_bytes(entry, self.h, *dims), device)


class UNet(_Handle):
    """Handle on the packed denoiser (lds_unet_*)."""
    KIND = "unet"

    def __init__(self, cfg, state):
        c = UNetCfg()
        c.out_dims, c.n_hidden = cfg["out_channels"], cfg["cond_channels"]
        c.n_layers, c.n_heads, c.norm_groups = cfg["layers_per_block"], cfg["heads"], cfg["groups"]
        boc = cfg["block_out_channels"]
        c.n_blocks = len(boc)
        for i, v in enumerate(boc):
            c.block_out_channels[i] = v
        self._create_weights(c, state)
        self.M, self.H = c.out_dims, c.n_hidden

    def set_gemm_mode(self, mode):
        """0 / "f32": exact-fp32 MFMA (default); 2 / "split_f16": two fp16 terms per operand (opt-in; include/lds.h)"""
        m = {"f32": 0, "split_bf16": 1, "split_f16": 2}.get(mode, mode)      # (1 is refused by the library: removed mode)
        check(lib().lds_unet_set_gemm_mode(self.h, int(m)))

    def gemm_mode(self):
        return int(lib().lds_unet_get_gemm_mode(self.h))

    def set_latency_mode(self, on):
        """Tile / split choices from the actual batch (one or two utterances fill the chip); include/lds.h"""
        check(lib().lds_unet_set_latency_mode(self.h, 1 if on else 0))

    def latency_mode(self):
        return int(lib().lds_unet_get_latency_mode(self.h))

    @staticmethod
    def _lengths(lengths, B, T):
        """per-utterance frame counts of a ragged batch -> host int32 [B] (include/lds.h lds_sampler_run_ragged)"""
        return _host_lengths(lengths, B, 1, T)

    def workspace_tensor(self, B, T, device, sampler=False):
        """the caller-owned scratch a forward (or sampler run) of this size on the current stream will use (tests poison it)"""
        return self._workspace("lds_sampler_workspace_bytes" if sampler else "lds_unet_workspace_bytes", device, B, T)

    def plan(self, B, T):
        """[(slot name, offset, bytes)] of the workspace of a forward of this size (include/lds_test.h lds_debug_unet_plan)"""
        buf = C.create_string_buffer(1 << 16)
        check(lib().lds_debug_unet_plan(self.h, B, T, buf, len(buf)))
        return [(a, int(b), int(c)) for a, b, c in (ln.split() for ln in buf.value.decode().splitlines())]

    def forward(self, x, cond, t, lengths=None):
        import torch
        B, M, T = x.shape
        assert M == self.M and cond.shape == (B, self.H, T) and t.shape == (B,)
        ws = self.workspace_tensor(B, T, x.device)
        eps = torch.empty_like(x)
        ln = None if lengths is None else self._lengths(lengths, B, T)
        fn, ln_at = _dense_or_ragged("lds_unet_forward", ln)
        check(fn(self.h, _dev(x, torch.float32), _dev(cond, torch.float32), _dev(t, torch.float32), *ln_at, _dev(eps), _dev(ws), ws.numel(), B, T,
                 _stream()))
        return eps

    def sample(self, method, table, cond, x, noise=None, lengths=None):
        """Run a whole sampler loop in place on x [B,M,T]; table: float32 [n_rows, 16] (host); lengths: the utterances' own frame counts
        (ragged batch) or None."""
        import torch
        B, M, T = x.shape
        table = np.ascontiguousarray(table, dtype=np.float32)
        assert table.ndim == 2 and table.shape[1] == TABLE_STRIDE
        ws = self.workspace_tensor(B, T, x.device, sampler=True)
        ln = None if lengths is None else self._lengths(lengths, B, T)
        fn, ln_at = _dense_or_ragged("lds_sampler_run", ln)
        check(fn(self.h, METHODS[method], table.shape[0], table.ctypes.data, _dev(cond, torch.float32), _dev(x, torch.float32),
                 _dev_or_null(noise, torch.float32), *ln_at, _dev(ws), ws.numel(), B, T, _stream()))
        return x


class Embed(_Handle):
    """unit_embed + spk_embed front end (lds_embed_*)."""
    KIND = "embed"

    def __init__(self, unit_w, unit_b, spk_w=None):
        uw = np.ascontiguousarray(unit_w, dtype=np.float32)
        ub = np.ascontiguousarray(unit_b, dtype=np.float32)
        sw = None if spk_w is None else np.ascontiguousarray(spk_w, dtype=np.float32)
        self.H, self.Cin = uw.shape
        self._create(self.Cin, self.H, 0 if sw is None else sw.shape[0], _host(uw), _host(ub), _host(sw))

    def forward(self, units, spk_id):
        import torch
        B, T, K = units.shape
        assert K == self.Cin
        ws = self._workspace("lds_embed_workspace_bytes", units.device, B, T)
        cond = torch.empty(B, self.H, T, dtype=torch.float32, device=units.device)
        sid = None
        if spk_id is not None:
            sid = spk_id.reshape(B, -1)[:, 0].contiguous().to(torch.int64)
        check(lib().lds_embed_forward(self.h, _dev(units, torch.float32), _dev_or_null(sid), _dev(cond), _dev(ws), ws.numel(), B, T, _stream()))
        return cond


def debug_fill(t, pattern):
    """every 32-bit word of a device tensor = pattern (include/lds_test.h: poisoned-workspace tests)"""
    check(lib().lds_debug_fill_u32(_dev(t), t.numel() * t.element_size() // 4, pattern, _stream()))


def debug_trace(on):
    check(lib().lds_debug_trace(1 if on else 0))


def debug_trace_records():
    """[(name, bytes)] of the stages recorded since debug_trace(True) (host copies of every UNet stage's output)"""
    out = []
    for i in range(lib().lds_debug_trace_count()):
        name = C.create_string_buffer(96)
        ptr, nb = C.c_void_p(), C.c_size_t()
        check(lib().lds_debug_trace_get(i, name, len(name), C.byref(ptr), C.byref(nb)))
        out.append((name.value.decode(), C.string_at(ptr, nb.value)))
    return out


def debug_trace_decode(name, raw, B):
    """one debug-trace record -> (stage name, plain [B, C, T] float32 array; a flat float32 array for records that are not activation tensors)"""
    parts = name.split("|")
    if len(parts) != 4:
        return name, np.frombuffer(raw, dtype=np.float32).copy()
    nm, Cc, T, mode = parts[0], int(parts[1]), int(parts[2]), int(parts[3])
    if mode == 0:      # K4P: [B][C/8][2][T+2][4], channel 8q + 2j + h
        a = np.frombuffer(raw, dtype=np.float32).reshape(B, Cc // 8, 2, T + 2, 4)
        out = np.empty((B, Cc // 8, 8, T), dtype=np.float32)
        for h in range(2):
            for j in range(4):
                out[:, :, 2 * j + h] = a[:, :, h, 1:T + 1, j]
        return nm, out.reshape(B, Cc, T)
    npl = 3 if mode == 1 else 2      # split planes [B][C/8][planes][T+2][8]: bf16 x 3 or fp16 x 2
    if mode == 1:
        a = (np.frombuffer(raw, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).reshape(B, Cc // 8, npl, T + 2, 8)
    else:
        a = np.frombuffer(raw, dtype=np.float16).astype(np.float32).reshape(B, Cc // 8, npl, T + 2, 8)
    v = a[:, :, 0].copy()
    for pl in range(1, npl):
        v = v + a[:, :, pl]
    return nm, np.ascontiguousarray(v[:, :, 1:T + 1].transpose(0, 1, 3, 2)).reshape(B, Cc, T)


def prof_enable(level=1):
    """0 = off, 1 = per kernel family / tile configuration, 2 = names also carry the operand shapes"""
    check(lib().lds_prof_enable(int(level)))


def prof_summary():
    """list of dicts {name,count,ms,flops,bytes}; synchronises the recorded events."""
    import json
    buf = C.create_string_buffer(1 << 16)
    check(lib().lds_prof_summary(buf, len(buf)))
    return json.loads(buf.value.decode())


def axpby(a, b, c0, c1):
    """c0*a + c1*b on the device."""
    import torch
    out = torch.empty_like(a)
    check(lib().lds_axpby(_dev(out), _dev(a, torch.float32), _dev(b, torch.float32), c0, c1, a.numel(), _stream()))
    return out


def q_sample_rows(x0, noise, t, sqrt_ac, sqrt_1m_ac):
    """x0, noise [B, ...] fp32, t int64 [B] (device), the two schedule tables fp32 [n_steps] (device) ->
    (sqrt_ac[t_b] * x0[b] + sqrt_1m_ac[t_b] * noise[b], t as fp32 [B]); include/lds.h lds_q_sample_rows"""
    import torch
    B = x0.shape[0]
    if noise.shape != x0.shape or tuple(t.shape) != (B,) or sqrt_ac.shape != sqrt_1m_ac.shape or sqrt_ac.dim() != 1:
        raise ValueError(f"q_sample_rows: x0 {list(x0.shape)}, noise {list(noise.shape)}, t {list(t.shape)}")
    out = torch.empty_like(x0)
    tf = torch.empty(B, dtype=torch.float32, device=x0.device)
    check(lib().lds_q_sample_rows(_dev(out), _dev(x0, torch.float32), _dev(noise, torch.float32), _dev(t, torch.int64), _dev(sqrt_ac, torch.float32),
                                  _dev(sqrt_1m_ac, torch.float32), sqrt_ac.numel(), _dev(tf), B, x0.numel() // B, _stream()))
    return out, tf


LOSS_TYPES = {"l1": 1, "l2": 2}
_loss_ws = Workspace()


def loss_reduce(a, b, loss_type="l2", ws=None):
    """mean((a - b)^2) ('l2') or mean(|a - b|) ('l1') as a 0-dim device tensor; deterministic (include/lds.h lds_loss_reduce).  `ws`: a caller's
    uint8 workspace (tests poison it), else one kept per stream."""
    import torch
    if a.shape != b.shape or a.numel() < 1:
        raise ValueError(f"loss_reduce: shapes {list(a.shape)} and {list(b.shape)}")
    _dev(a, torch.float32)
    nb = _bytes("lds_loss_reduce_workspace_bytes", a.numel())
    if ws is None:
        ws = _loss_ws.get(nb, a.device)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    check(lib().lds_loss_reduce(_dev(a, torch.float32), _dev(b, torch.float32), a.numel(), LOSS_TYPES[loss_type], _dev(out), _dev(ws), ws.numel(), _stream()))
    return out.reshape(())


def stft_mel(audio, basis, mel_basisT, n_fft_new, win_new, hop_new, n_fft, win, clip_val, F, lengths=None, ws=None):
    """audio [B, L] -> log-mel [B, F, n_mels], frame-major, in one launch (include/lds.h lds_stft_mel).  basis: device float64
    [n_fft_new, bins, 2]; mel_basisT: device fp32 [n_fft // 2 + 1, n_mels]; lengths: every clip's own sample count (host ints) or None;
    F: the rows of the result (at least the longest clip's frames).  `ws`: a caller's uint8 workspace (the launch needs none today)."""
    import torch
    if audio.dim() != 2:
        raise ValueError(f"stft_mel: audio must be [B, L], got {list(audio.shape)}")
    B, L = audio.shape
    n_mels = mel_basisT.shape[1]
    bins = min(n_fft_new // 2 + 1, n_fft // 2 + 1)
    if tuple(basis.shape) != (n_fft_new, bins, 2) or tuple(mel_basisT.shape) != (n_fft // 2 + 1, n_mels):
        raise ValueError(f"stft_mel: basis {list(basis.shape)} / mel basis {list(mel_basisT.shape)} do not fit n_fft_new {n_fft_new}, n_fft {n_fft}")
    ln = None if lengths is None else _host_lengths(lengths, B, 1, L, 64, "log-mel")
    _dev(audio, None)
    nb = _bytes("lds_stft_mel_workspace_bytes", n_fft_new, hop_new, n_mels, B, L)
    if ws is not None and ws.numel() < nb:
        raise ValueError(f"stft_mel: workspace of {ws.numel()} bytes, {nb} needed")
    out = torch.empty(B, F, n_mels, dtype=torch.float32, device=audio.device)
    check(lib().lds_stft_mel(_dev(audio, torch.float32), _host(ln), _dev(basis, torch.float64), _dev(mel_basisT, torch.float32), n_fft_new, win_new, hop_new,
                             n_fft, win, n_mels, clip_val, F, _dev(out), _dev_or_null(ws), 0 if ws is None else ws.numel(), B, L, _stream()))
    return out


def stft_dft_probe(audio, basis, mel_basisT, n_fft_new, hop_new):
    """the framed DFT of csrc/stftmel.hip alone: audio [B, L] -> raw (re, im) sums float64 [B, F, n_fft_new // 2 + 1, 2] (include/lds_test.h)"""
    import torch
    B, L = audio.shape
    F, bins, n_mels = 1 + (L - n_fft_new) // hop_new, n_fft_new // 2 + 1, mel_basisT.shape[1]
    assert tuple(basis.shape) == (n_fft_new, bins, 2) and tuple(mel_basisT.shape) == (bins, n_mels)
    out = torch.empty(B, F, n_mels, dtype=torch.float32, device=audio.device)
    dft = torch.zeros(B, F, bins, 2, dtype=torch.float64, device=audio.device)
    check(lib().lds_test_stft_dft(_dev(audio, torch.float32), _dev(basis, torch.float64), _dev(mel_basisT, torch.float32), n_fft_new, hop_new, n_mels, F,
                                  _dev(out), _dev(dft), B, L, _stream()))
    return dft


def gather_rows(table, idx):
    """table [N, C] fp32, idx int64 [...] -> table[idx] [..., C] on the device (codebook lookup)."""
    import torch
    idx = idx.contiguous()
    N, Cc = table.shape
    out = torch.empty(tuple(idx.shape) + (Cc,), dtype=torch.float32, device=table.device)
    if idx.numel():
        check(lib().lds_gather_rows(_dev(table, torch.float32), _dev(idx, torch.int64), _dev(out), idx.numel(), Cc, N, _stream()))
    return out


def resample_frames(x, n_out, step):
    """x [B, T, C] -> [B, n_out, C]: out[:, i] = x[:, min(floor(i * step), T - 1)] (nearest, fp32 index arithmetic)."""
    import torch
    B, T, Cc = x.shape
    out = torch.empty(B, n_out, Cc, dtype=torch.float32, device=x.device)
    if n_out:
        check(lib().lds_resample_frames(_dev(x, torch.float32), _dev(out), B, T, n_out, Cc, step, _stream()))
    return out


def transpose(x, scale=1.0):
    """[B,R,C] -> [B,C,R] / scale on the device."""
    import torch
    B, R, Cc = x.shape
    out = torch.empty(B, Cc, R, dtype=torch.float32, device=x.device)
    check(lib().lds_transpose(_dev(x, torch.float32), _dev(out), B, R, Cc, scale, _stream()))
    return out


def vocoder_cfg(h):
    """lds_vocoder_cfg of a HiFi-VAEGAN config dict (shared by the decoder and the encoder)."""
    c = VocoderCfg()
    c.inter_channels = h["inter_channels"]
    c.upsample_initial_channel = h["upsample_initial_channel"]
    c.n_ups = len(h["upsample_rates"])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        c.upsample_rates[i], c.upsample_kernel_sizes[i] = u, k
    c.resblock = 1 if str(h["resblock"]) == "1" else 2
    c.n_kernels = len(h["resblock_kernel_sizes"])
    c.n_dil = len(h["resblock_dilation_sizes"][0])
    for j, (k, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
        c.resblock_kernel_sizes[j] = k
        for m, d in enumerate(dil):
            c.resblock_dilation_sizes[j][m] = d
    return c


class Generator(_Handle):
    """HiFi-VAEGAN decoder (lds_vocoder_*)."""
    KIND = "vocoder"

    def __init__(self, h, state):
        c = vocoder_cfg(h)
        self._create_weights(c, state)
        self.hop = int(np.prod(h["upsample_rates"]))
        self.C = c.inter_channels

    def workspace_tensor(self, B, T, device):
        """the caller-owned scratch a forward of this size on the current stream will use (tests poison it)"""
        return self._workspace("lds_vocoder_workspace_bytes", device, B, T)

    def forward(self, z, lengths=None):
        """z [B,C,T] -> wav [B,1,T*hop]; lengths: the utterances' own frame counts (ragged batch, include/lds.h lds_vocoder_forward_ragged)"""
        import torch
        B, Cc, T = z.shape
        assert Cc == self.C
        ws = self.workspace_tensor(B, T, z.device)
        wav = torch.empty(B, 1, T * self.hop, dtype=torch.float32, device=z.device)
        ln = None if lengths is None else UNet._lengths(lengths, B, T)
        fn, ln_at = _dense_or_ragged("lds_vocoder_forward", ln)
        check(fn(self.h, _dev(z, torch.float32), *ln_at, _dev(wav), _dev(ws), ws.numel(), B, T, _stream()))
        return wav


class VaeEncoder(_Handle):
    """HiFi-VAEGAN encoder (lds_vae_encoder_*): audio [B,L] -> (out [B,T,2C], z [B,T,C] or None)."""
    KIND = "vae_encoder"

    def __init__(self, h, state):
        hop = int(np.prod(h["upsample_rates"]))
        if "hop_size" in h and int(h["hop_size"]) != hop:      # extract pads to hop_size; the encoder's frames are prod(upsample_rates) samples
            raise ValueError(f"VaeEncoder: config hop_size {h['hop_size']} != prod(upsample_rates) {hop} = {list(h['upsample_rates'])}")
        c = vocoder_cfg(h)
        self._create_weights(c, state)
        self.hop = hop
        self.C = c.inter_channels

    def workspace_bytes(self, B, L):
        return _bytes("lds_vae_encoder_workspace_bytes", self.h, B, L)

    @staticmethod
    def lengths(lengths, B, L):
        """per-clip sample counts of a ragged batch -> host int32 [B] (include/lds.h lds_vae_encoder_forward_ragged: B <= 64, 1 .. L)"""
        return _host_lengths(lengths, B, 1, L, 64, "encoder")

    def forward(self, audio, noise=None, only_mean=False, ws=None, lengths=None):
        """audio [B,L] (L a multiple of the hop); noise [B,C,T] or None -> (out [B,T,2C], z [B,T,C] or None); `ws`: a caller's uint8
        workspace of at least workspace_bytes(B, L) (tests poison it), else the handle's own; `lengths`: every clip's own sample count
        (host ints, ragged batch: include/lds.h lds_vae_encoder_forward_ragged) or None"""
        import torch
        B, L = audio.shape
        T = L // self.hop
        ln = self.lengths(lengths, B, L) if lengths is not None else None
        if noise is not None and tuple(noise.shape) != (B, self.C, T):
            raise ValueError(f"noise must be [B, C, T] = {[B, self.C, T]}, got {list(noise.shape)}")
        nb = self.workspace_bytes(B, L)
        if ws is None:
            ws = self.ws.get(nb, audio.device)
        out = torch.empty(B, T, 2 * self.C, dtype=torch.float32, device=audio.device)
        z = torch.empty(B, T, self.C, dtype=torch.float32, device=audio.device) if noise is not None else None
        fn, ln_at = _dense_or_ragged("lds_vae_encoder_forward", ln)
        check(fn(self.h, _dev(audio, torch.float32), *ln_at, _dev_or_null(noise, torch.float32), _dev(out), _dev_or_null(z), int(bool(only_mean)),
                 _dev(ws), ws.numel(), B, L, _stream()))
        return out, z


class HubertCfg(C.Structure):
    _fields_ = [("conv_dim", C.c_int), ("n_state", C.c_int), ("n_head", C.c_int), ("n_layer", C.c_int), ("n_ffn", C.c_int), ("n_proj", C.c_int),
                ("pos_kernel", C.c_int), ("pos_groups", C.c_int), ("n_ctx", C.c_int)]


def _w2v_check_dims(d, widths):
    """include/lds.h's limits on the dimensions that HuBERT and wav2vec 2.0 share; `widths`: the fields that are any positive multiple of 64.
    The messages name HuBERT for both, as they always have."""
    for k in ("conv_dim", "n_state"):
        if d[k] < 64 or d[k] % 64 or d[k] > 1024:
            raise ValueError(f"Hubert: {k} {d[k]} must be a multiple of 64 in 64 .. 1024")
    if d["n_head"] < 1 or d["n_state"] != 64 * d["n_head"]:
        raise ValueError(f"Hubert: n_state {d['n_state']} must be 64 * n_head ({d['n_head']})")
    for k in widths:
        if d[k] < 64 or d[k] % 64:
            raise ValueError(f"Hubert: {k} {d[k]} must be a positive multiple of 64")
    if d["pos_kernel"] < 2 or d["pos_kernel"] > 128 or d["pos_kernel"] % 2:
        raise ValueError(f"Hubert: pos_kernel {d['pos_kernel']} must be even in 2 .. 128")
    g = d["pos_groups"]
    if g < 1 or d["n_state"] % g or (d["n_state"] // g) % 16 or d["n_state"] // g > 64:
        raise ValueError(f"Hubert: n_state / pos_groups must be 16, 32, 48 or 64 (got {d['n_state']} / {g})")
    if not 1 <= d["n_layer"] <= 64:
        raise ValueError(f"Hubert: n_layer {d['n_layer']} outside 1 .. 64")
    if not 1 <= d["n_ctx"] <= 1500:
        raise ValueError(f"Hubert: n_ctx {d['n_ctx']} outside 1 .. 1500")


class _UnitsEncoder(_Handle):
    """What the four units encoders' handles share: the path of a call on audio [B, L].  Every limit of include/lds.h is checked first
    (ValueError, before a device is touched), then the per-clip lengths, the device, the workspace, the output and the entry.  A subclass
    states its limits below, `_units_of` (the frame rule) and, per entry, the output's shape and the entry's extra arguments."""
    MIN_SAMPLES = 400           # of a clip without padding
    MAX_BATCH = None            # clips per call; None = any positive count (per-clip lengths allow 64 in every encoder)
    PAD = 0                     # the largest `pad` (zeros added on each side of every clip); 0 = the entries take no pad
    UNIT, CTX, HINT = "frames", "n_ctx", ""      # words of the messages

    @classmethod
    def _pad(cls, pad):
        return cls.PAD if pad is None else pad

    @classmethod
    def lengths(cls, lengths, B, L, pad=None):
        """per-clip sample counts -> host int32 [B] (include/lds.h: B <= 64, MIN_SAMPLES - 2 pad .. L)"""
        return _host_lengths(lengths, B, cls.MIN_SAMPLES - 2 * cls._pad(pad), L, 64, "units")

    def workspace_bytes(self, B, L, pad=None):
        return _bytes(f"lds_{self.KIND}_workspace_bytes", self.h, B, L, *((self._pad(pad),) if self.PAD else ()))

    def _check(self, B, L, pad=None):
        """the limits of a call on B clips in buffers of L samples (ValueError); returns the units (frames, rows) of L samples"""
        name, pad, ctx = type(self).__name__, self._pad(pad), self.dims["n_ctx"]
        if self.MAX_BATCH is None and B < 1:
            raise ValueError(f"{name}: an empty batch")
        if self.MAX_BATCH is not None and not 1 <= B <= self.MAX_BATCH:
            raise ValueError(f"{name}: 1 .. {self.MAX_BATCH} clips per call (got {B})")
        if not 0 <= pad <= self.PAD:
            raise ValueError(f"{name}: pad {pad} outside 0 .. {self.PAD}")
        if L < self.MIN_SAMPLES - 2 * pad:
            raise ValueError(f"{name}: clips need at least {self.MIN_SAMPLES - 2 * pad} samples (got {L}){self.HINT}")
        n = self._units_of(L, pad)
        if n > ctx:
            raise ValueError(f"{name}: {L} samples give {n} {self.UNIT}, more than {self.CTX} {ctx}")
        return n

    def _call(self, entry, audio, lengths, ws, shape, mid=(), pad=None, pre=()):
        """entry(h, audio, lengths, *pre, out, *mid, ws, ws_bytes, B, L, [pad,] stream) -> out [B, *shape(n, L)], n = the units of L samples"""
        import torch
        if audio.dim() != 2:
            raise ValueError(f"{type(self).__name__}: audio must be [B, L], got {list(audio.shape)}")
        B, L = audio.shape
        n = self._check(B, L, pad)
        ln = self.lengths(lengths, B, L, pad) if lengths is not None else None
        _dev(audio, None)
        tail = (self._pad(pad),) if self.PAD else ()
        ws = ws if ws is not None else self.ws.get(self.workspace_bytes(B, L, pad), audio.device)
        out = torch.empty(B, *shape(n, L), dtype=torch.float32, device=audio.device)
        check(getattr(lib(), entry)(self.h, _dev(audio, torch.float32), _host(ln), *pre, _dev(out), *mid, _dev(ws), ws.numel(), B, L, *tail, _stream()))
        return out


class Hubert(_UnitsEncoder):
    """HuBERT units encoder (lds_hubert_*): audio [B,L] at 16 kHz -> the feature extractor's output [B,T,conv_dim] / the transformer's
    [B,T,n_state] after `layer` blocks / units [B,T,n_proj].  `pad` zeros are added on each side of every clip (40: HubertSoft.units,
    T = L // 320).  `lengths`: every clip's own sample count (host ints, 400 - 2 pad .. L, at most 64 clips): each clip is encoded as if
    alone.  Every limit of include/lds.h is checked here first (ValueError, before a device is touched)."""
    KIND = "hubert"
    FIELDS = ("conv_dim", "n_state", "n_head", "n_layer", "n_ffn", "n_proj", "pos_kernel", "pos_groups", "n_ctx")
    PAD = 40

    def __init__(self, dims, state):
        d = {k: int(dims[k]) for k in self.FIELDS}
        self.check_dims(d)
        self._create_weights(HubertCfg(*(d[k] for k in self.FIELDS)), state)
        self.dims = d

    @staticmethod
    def check_dims(d):
        _w2v_check_dims(d, ("n_ffn", "n_proj"))

    @staticmethod
    def frames(n_samples, pad=40):
        """frames of a clip of n_samples padded by `pad` zeros per side (= n_samples // 320 for pad 40)"""
        from . import arch
        return arch.hubert_frames(n_samples, pad)

    _units_of = frames

    def features(self, audio, lengths=None, ws=None, pad=40):
        return self._call("lds_hubert_features", audio, lengths, ws, lambda n, L: (n, self.dims["conv_dim"]), pad=pad)

    def encode(self, audio, lengths=None, layer=None, proj=False, ws=None, pad=40):
        """layer: the blocks to run (None = all, 0 = the output of `norm`); proj: apply `proj` (all blocks only) -> [B,T,n_proj]"""
        nl = self.dims["n_layer"] if layer is None else int(layer)
        if not 0 <= nl <= self.dims["n_layer"]:
            raise ValueError(f"Hubert: layer {nl} outside 0 .. {self.dims['n_layer']}")
        if proj and nl != self.dims["n_layer"]:
            raise ValueError(f"Hubert: proj follows the last layer (layer {nl} of {self.dims['n_layer']})")
        width = self.dims["n_proj" if proj else "n_state"]
        return self._call("lds_hubert_encode", audio, lengths, ws, lambda n, L: (n, width), mid=(nl, 1 if proj else 0), pad=pad)


class W2vCfg(C.Structure):
    _fields_ = [("conv_dim", C.c_int), ("n_state", C.c_int), ("n_head", C.c_int), ("n_layer", C.c_int), ("n_ffn", C.c_int),
                ("pos_kernel", C.c_int), ("pos_groups", C.c_int), ("n_ctx", C.c_int)]


class Wav2Vec2(_UnitsEncoder):
    """wav2vec 2.0 units encoder in its layer-norm flavour, XLSR-53 (lds_w2v_*): audio [B,L] at 16 kHz, taken as it is -> the feature
    extractor's output [B,T,conv_dim] / the encoder's [B,T,n_state].  `state`: fairseq-named tensors (lds.arch.w2v_param_shapes).
    `lengths`: every clip's own sample count (host ints, 400 .. L, at most 64 clips): each clip is encoded as if alone.  Every limit of
    include/lds.h is checked here first (ValueError, before a device is touched)."""
    KIND = "w2v"
    FIELDS = ("conv_dim", "n_state", "n_head", "n_layer", "n_ffn", "pos_kernel", "pos_groups", "n_ctx")

    def __init__(self, dims, state):
        d = {k: int(dims[k]) for k in self.FIELDS}
        self.check_dims(d)
        self._create_weights(W2vCfg(*(d[k] for k in self.FIELDS)), state)
        self.dims = d

    @staticmethod
    def check_dims(d):
        _w2v_check_dims(d, ("n_ffn",))      # (the limits are HuBERT's; there is no proj here)

    @staticmethod
    def frames(n_samples):
        from . import arch
        return arch.w2v_frames(n_samples)

    def _units_of(self, n_samples, pad=0):
        return self.frames(n_samples)

    def features(self, audio, lengths=None, ws=None):
        return self._call("lds_w2v_features", audio, lengths, ws, lambda n, L: (n, self.dims["conv_dim"]))

    def encode(self, audio, lengths=None, ws=None):
        return self._call("lds_w2v_encode", audio, lengths, ws, lambda n, L: (n, self.dims["n_state"]))


class WavlmCfg(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("conv_dim", "n_state", "n_head", "n_layer", "n_ffn", "pos_kernel", "pos_groups", "num_buckets", "max_distance",
                                       "stable_layer_norm", "n_ctx")]


class WavLM(_UnitsEncoder):
    """WavLM units encoder (lds_wavlm_*): audio [B,L] at 16 kHz -> the feature extractor's output [B,T,conv_dim] / WavLMModel's
    hidden_states[layer] [B,T,n_state] (layer None = last_hidden_state).  `state`: transformers-named tensors (lds.arch.wavlm_param_shapes).
    `normalize`: every clip is set to zero mean and unit variance over its own samples first (WavLM-Large's feature extractor).  `lengths`:
    every clip's own sample count (host ints, 400 .. L): each clip is encoded as if alone.  At most 64 clips per call.  Every limit of
    include/lds.h is checked here first (ValueError, before a device is touched)."""
    KIND = "wavlm"
    FIELDS = ("conv_dim", "n_state", "n_head", "n_layer", "n_ffn", "pos_kernel", "pos_groups", "num_buckets", "max_distance", "stable_layer_norm", "n_ctx")
    MAX_BATCH = 64

    def __init__(self, dims, state):
        d = {k: int(dims[k]) for k in self.FIELDS}
        self.check_dims(d)
        self._create_weights(WavlmCfg(*(d[k] for k in self.FIELDS)), state)
        self.dims = d

    @staticmethod
    def check_dims(d):
        _w2v_check_dims(d, ("n_ffn",))      # (the skeleton's limits are HuBERT's)
        nb, md = d["num_buckets"], d["max_distance"]
        if nb < 4 or nb % 4 or nb > 4096:
            raise ValueError(f"WavLM: num_buckets {nb} must be a multiple of 4 in 4 .. 4096")
        if not nb // 4 < md <= 1 << 20:
            raise ValueError(f"WavLM: max_distance {md} outside num_buckets / 4 + 1 = {nb // 4 + 1} .. 2^20")
        if d["stable_layer_norm"] not in (0, 1):
            raise ValueError(f"WavLM: stable_layer_norm {d['stable_layer_norm']} (0 or 1)")

    @staticmethod
    def frames(n_samples):
        from . import arch
        return arch.wavlm_frames(n_samples)

    def _units_of(self, n_samples, pad=0):
        return self.frames(n_samples)

    def features(self, audio, lengths=None, normalize=False, ws=None):
        return self._call("lds_wavlm_features", audio, lengths, ws, lambda n, L: (n, self.dims["conv_dim"]), mid=(1 if normalize else 0,))

    def encode(self, audio, lengths=None, layer=None, normalize=False, ws=None, layer_weights=None):
        """layer: the blocks to run = the index into WavLMModel's hidden_states (None = all: last_hidden_state).  layer_weights (n_layer + 1
        finite host floats, already soft-maxed; not with `layer`): the weighted sum of all hidden states instead (lds_wavlm_encode_layersum)"""
        if layer_weights is not None:
            if layer is not None:
                raise ValueError("WavLM: layer_weights sums every hidden state; it does not go with layer=")
            lw = np.ascontiguousarray(np.asarray(layer_weights.detach().cpu() if hasattr(layer_weights, "detach") else layer_weights, dtype=np.float32).reshape(-1))
            if lw.shape != (self.dims["n_layer"] + 1,) or not np.isfinite(lw).all():
                raise ValueError(f"WavLM: layer_weights must be {self.dims['n_layer'] + 1} finite numbers (one per hidden state)")
            return self._call("lds_wavlm_encode_layersum", audio, lengths, ws, lambda n, L: (n, self.dims["n_state"]), mid=(1 if normalize else 0,), pre=(_host(lw),))
        nl = self.dims["n_layer"] if layer is None else int(layer)
        if not 0 <= nl <= self.dims["n_layer"]:
            raise ValueError(f"WavLM: layer {nl} outside 0 .. {self.dims['n_layer']}")
        return self._call("lds_wavlm_encode", audio, lengths, ws, lambda n, L: (n, self.dims["n_state"]), mid=(nl, 1 if normalize else 0))


class W2vBertCfg(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n_mels", "stride", "n_state", "n_head", "n_ffn", "n_layer", "left_max", "right_max", "dw_kernel", "n_ctx")] + \
               [("eps", C.c_float)]


class Wav2Vec2Bert(_UnitsEncoder):
    """w2v-BERT 2.0 units encoder (lds_w2vbert_*): audio [B,L] at 16 kHz -> SeamlessM4TFeatureExtractor's input_features [B,R,n_mels*stride] /
    Wav2Vec2BertModel's last_hidden_state [B,R,n_state], R = the rows of L samples (lds.arch.w2vbert_frames).  `state`: transformers-named
    tensors (lds.arch.w2vbert_param_shapes).  `lengths`: every clip's own sample count (host ints, 560 .. L, at most 64 clips): each clip is
    encoded as if alone.  A clip with an odd frame count n keeps its masked last row (row n // 2) in the result, as the reference does.
    Every limit of include/lds.h is checked here first (ValueError, before a device is touched)."""
    KIND = "w2vbert"
    FIELDS = ("n_mels", "stride", "n_state", "n_head", "n_ffn", "n_layer", "left_max", "right_max", "dw_kernel", "n_ctx")
    MIN_SAMPLES, MAX_BATCH = 560, 64
    UNIT, HINT = "rows", "; pad them as Units_Encoder.encode does"

    def __init__(self, dims, state):
        d = self.check_dims(dims)
        self._create_weights(W2vBertCfg(*(d[k] for k in self.FIELDS), d["eps"]), state)
        self.dims = d

    @classmethod
    def check_dims(cls, dims):
        """include/lds.h's limits (ValueError); returns the fields as ints (eps a float)"""
        d = {k: int(dims[k]) for k in cls.FIELDS}
        d["eps"] = float(dims.get("eps", 1e-5))
        fd = d["n_mels"] * d["stride"]
        if not (8 <= d["n_mels"] <= 128 and 1 <= d["stride"] <= 8 and fd % 32 == 0 and fd <= 1024):
            raise ValueError(f"Wav2Vec2Bert: n_mels {d['n_mels']} x stride {d['stride']} must be a multiple of 32 up to 1024")
        if not (64 <= d["n_state"] <= 1024 and d["n_state"] % 64 == 0 and d["n_state"] == 64 * d["n_head"]):
            raise ValueError(f"Wav2Vec2Bert: n_state {d['n_state']} must be a multiple of 64 in 64 .. 1024 and 64 x n_head ({d['n_head']})")
        if d["n_ffn"] < 64 or d["n_ffn"] % 64:
            raise ValueError(f"Wav2Vec2Bert: n_ffn {d['n_ffn']} must be a positive multiple of 64")
        if not 1 <= d["n_layer"] <= 64:
            raise ValueError(f"Wav2Vec2Bert: n_layer {d['n_layer']} outside 1 .. 64")
        if d["left_max"] < 0 or d["right_max"] < 0 or d["left_max"] + d["right_max"] + 1 > 80:
            raise ValueError(f"Wav2Vec2Bert: left_max {d['left_max']} + right_max {d['right_max']} + 1 distances exceed 80")
        if not (1 <= d["dw_kernel"] <= 31 and d["dw_kernel"] % 2 == 1):
            raise ValueError(f"Wav2Vec2Bert: dw_kernel {d['dw_kernel']} must be odd in 1 .. 31")
        if not 1 <= d["n_ctx"] <= 1500:
            raise ValueError(f"Wav2Vec2Bert: n_ctx {d['n_ctx']} outside 1 .. 1500")
        if not 0.0 < d["eps"] < 1.0:
            raise ValueError(f"Wav2Vec2Bert: eps {d['eps']} outside (0, 1)")
        return d

    def rows(self, n_samples):
        n = 1 + (int(n_samples) - 400) // 160
        return (n + self.dims["stride"] - 1) // self.dims["stride"]

    def _units_of(self, n_samples, pad=0):
        return self.rows(n_samples)

    def fbank(self, audio, lengths=None, ws=None):
        return self._call("lds_w2vbert_fbank", audio, lengths, ws, lambda n, L: (n, self.dims["n_mels"] * self.dims["stride"]))

    def encode(self, audio, lengths=None, ws=None):
        return self._call("lds_w2vbert_encode", audio, lengths, ws, lambda n, L: (n, self.dims["n_state"]))

    def encode_features(self, feats, n_frames=None, ws=None):
        """feats [B, R, n_mels * stride] (input_features) -> [B, R, n_state]; n_frames: every clip's frame count n (host ints, 2 .. stride R;
        rows at and beyond n // stride are masked), None = stride R"""
        import torch
        st, fd = self.dims["stride"], self.dims["n_mels"] * self.dims["stride"]
        if feats.dim() != 3 or feats.shape[2] != fd:
            raise ValueError(f"Wav2Vec2Bert: features must be [B, R, {fd}], got {list(feats.shape)}")
        B, R = feats.shape[0], feats.shape[1]
        if not 1 <= B <= self.MAX_BATCH:
            raise ValueError(f"Wav2Vec2Bert: 1 .. {self.MAX_BATCH} clips per call (got {B})")
        if not 1 <= R <= self.dims["n_ctx"]:
            raise ValueError(f"Wav2Vec2Bert: {R} rows outside 1 .. n_ctx {self.dims['n_ctx']}")
        nf = None
        if n_frames is not None:
            nf = _host_lengths(n_frames, B, max(2, st), st * R, self.MAX_BATCH, "units")
        _dev(feats, None)
        ws = ws if ws is not None else self.ws.get(self.workspace_bytes(B, 400 + 160 * (st * R - 1)), feats.device)
        out = torch.empty(B, R, self.dims["n_state"], dtype=torch.float32, device=feats.device)
        check(lib().lds_w2vbert_encode_features(self.h, _dev(feats, torch.float32), _host(nf), _dev(out), _dev(ws), ws.numel(), B, R, _stream()))
        return out


class Whisper(_UnitsEncoder):
    """Whisper units encoder (lds_whisper_*): audio [B,L] at 16 kHz -> log-mel [B,n_mels,L//160] / units [B,T,n_state], T = (L//160 - 1)//2 + 1.
    `lengths`: every clip's own sample count (host ints, 400 .. L, at most 64 clips): each clip is encoded as if alone."""
    KIND = "whisper"
    HOP, N_FFT = 160, 400
    CTX, HINT = "n_audio_ctx", "; pad them as Units_Encoder.encode does"

    def __init__(self, n_mels, n_state, n_head, n_layer, n_ctx, state, mel_filters):
        if n_mels not in (80, 128):
            raise ValueError(f"Whisper: n_mels {n_mels} (80 or 128)")
        if n_state % 64 or n_head < 1 or n_state != 64 * n_head:
            raise ValueError(f"Whisper: n_state {n_state} must be 64 * n_head ({n_head})")
        if n_layer < 1 or n_ctx < 1:
            raise ValueError(f"Whisper: n_layer {n_layer} and n_ctx {n_ctx} must be positive")
        mf = np.ascontiguousarray(mel_filters, dtype=np.float32)
        if mf.shape != (n_mels, 201):
            raise ValueError(f"Whisper: mel_filters must be [{n_mels}, 201], got {list(mf.shape)}")
        self._create_weights(WhisperCfg(n_mels, n_state, n_head, n_layer, n_ctx), state, _host(mf))
        self.n_mels, self.n_state, self.n_ctx = n_mels, n_state, n_ctx
        self.dims = dict(n_mels=n_mels, n_state=n_state, n_ctx=n_ctx)

    def frames(self, n_mel_frames):
        return (int(n_mel_frames) - 1) // 2 + 1

    def _units_of(self, n_samples, pad=0):
        return self.frames(n_samples // self.HOP)

    def logmel(self, audio, lengths=None, ws=None):
        """audio [B,L] -> [B,n_mels,L//160] (frames at and beyond a clip's own count are zeros)"""
        return self._call("lds_whisper_logmel", audio, lengths, ws, lambda n, L: (self.n_mels, L // self.HOP))

    def encode_mel(self, mel, n_frames=None, ws=None):
        """mel [B,n_mels,F] -> units [B,T,n_state]; n_frames: every clip's own mel frame count (host ints) or None"""
        import torch
        B, M, F = mel.shape
        if M != self.n_mels:
            raise ValueError(f"Whisper: mel has {M} channels, the model {self.n_mels}")
        if B < 1 or F < 1 or self.frames(F) > self.n_ctx:
            raise ValueError(f"Whisper: {F} mel frames give {self.frames(F)} frames, outside 1 .. n_audio_ctx {self.n_ctx}")
        nf = _host_lengths(n_frames, B, 1, F, 64, "units") if n_frames is not None else None
        ws = ws if ws is not None else self.ws.get(self.workspace_bytes(B, max(F * self.HOP, self.N_FFT)), mel.device)
        units = torch.empty(B, self.frames(F), self.n_state, dtype=torch.float32, device=mel.device)
        check(lib().lds_whisper_encode_mel(self.h, _dev(mel, torch.float32), _host(nf), _dev(units), _dev(ws), ws.numel(), B, F, _stream()))
        return units

    def encode(self, audio, lengths=None, ws=None):
        """audio [B,L] -> units [B,T,n_state] (rows at and beyond a clip's own frame count are zeros)"""
        return self._call("lds_whisper_encode", audio, lengths, ws, lambda n, L: (n, self.n_state))


def _conv_down(x, w, b, stride, slope, tile, cfg, lengths_in=None, lengths_out=None):
    import torch
    B, Ci, T = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    Co, _, K = w.shape
    pad = (K - stride + 1) // 2
    out = torch.empty(B, Co, (T + 2 * pad - K) // stride + 1, dtype=torch.float32, device=x.device)
    bb = np.ascontiguousarray(b, dtype=np.float32) if b is not None else None
    buf = C.create_string_buffer(128)
    fn, ln_at = _dense_or_ragged("lds_test_conv_down", lengths_in, lengths_out)
    check(fn(_dev(x, torch.float32), _host(w), _host(bb), Ci, Co, K, stride, T, B, slope, *ln_at, tile, _dev(out), buf, len(buf), _stream()))
    if cfg is not None:
        cfg.append(buf.value.decode())
    return out


def conv_down(x, w, b, stride, slope=1.0, tile=0, cfg=None):
    """The encoder's convolution alone (lds_test_conv_down): x [B,Ci,T] on the device, w [Co,Ci,K] / b [Co] host arrays ->
    [B,Co,(T + 2 pad - K) // stride + 1] with pad = (K - stride + 1) // 2, LeakyReLU(slope) on the input.  tile: 0 = the product path's
    choice, else 64064 / 64128 / 128128; cfg: a list that receives the configuration that ran."""
    return _conv_down(x, w, b, stride, slope, tile, cfg)


def conv_down_ragged(x, w, b, stride, lengths_in, lengths_out, slope=1.0, tile=0, cfg=None):
    """conv_down over a ragged batch (lds_test_conv_down_ragged): x reads as zeros from lengths_in[b] on, the output is zeros from
    lengths_out[b] on (host ints, B <= 64)"""
    li = np.ascontiguousarray(lengths_in, dtype=np.int32)
    lo = np.ascontiguousarray(lengths_out, dtype=np.int32)
    assert li.shape == lo.shape == (x.shape[0],)
    return _conv_down(x, w, b, stride, slope, tile, cfg, li, lo)


class LM(_Handle):
    """text2semantic RoFormer (lds_lm_*): encoder prefill + cached decode loop."""
    KIND = "lm"

    def __init__(self, cfg, state):
        c = LMCfg()
        c.hidden, c.heads, c.inter = cfg["hidden"], cfg["heads"], cfg["inter"]
        c.enc_layers, c.dec_layers = cfg["enc_layers"], cfg["dec_layers"]
        c.text_vocab, c.type_vocab, c.sem_vocab = cfg["text_vocab"], cfg["type_vocab"], cfg["sem_vocab"]
        c.n_spk_rows = cfg["n_spk"] + 1 if (cfg["n_spk"] is not None and cfg["n_spk"] > 1) else 0
        c.max_pos, c.eps = cfg["max_pos"], cfg["eps"]
        c.sem_bos, c.sem_eos, c.sem_pad = cfg["sem_bos"], cfg["sem_eos"], cfg["sem_pad"]
        self._create_weights(c, state)
        self.cfg = cfg

    def _ws(self, B, L, max_length, device, num_beams=1):
        if num_beams == 1:
            return self._workspace("lds_lm_workspace_bytes", device, B, L, max_length)
        return self._workspace("lds_lm_workspace_bytes_opts", device, B, L, max_length, int(num_beams))

    def encode(self, phone, tone, spk_id=None, enc_len=None):
        """enc_len: int32 [B] on the device (real positions per right-padded row) or None"""
        import torch
        B, L = phone.shape
        ph, tn = phone.contiguous().to(torch.int64), tone.contiguous().to(torch.int64)
        sp = spk_id.contiguous().to(torch.int64) if spk_id is not None else None
        ws = self._ws(B, L, 2, phone.device)
        enc = torch.empty(B, L, self.cfg["hidden"], dtype=torch.float32, device=phone.device)
        check(lib().lds_lm_encode(self.h, _dev(ph, torch.int64), _dev(tn, torch.int64), _dev_or_null(sp, torch.int64), _dev_or_null(enc_len, torch.int32),
                                  _dev(enc), _dev(ws), ws.numel(), B, L, _stream()))
        return enc

    def generate(self, enc, max_length, do_sample, top_k, top_p, temperature, repetition_penalty, uniforms=None, return_logits=False, enc_len=None,
                 num_beams=1, no_repeat_ngram_size=0, early_stopping=True):
        """num_beams > 1: greedy beam search (do_sample False); enc / enc_len stay one row per batch item (include/lds.h lds_lm_decode_opts)"""
        import torch
        B, L, _ = enc.shape
        o = LMDecodeOpts(1 if do_sample else 0, int(top_k or 0), float(top_p), float(temperature), float(repetition_penalty), int(no_repeat_ngram_size),
                         int(num_beams), EARLY_STOPPING.get(early_stopping, -1))
        ws = self._ws(B, L, max_length, enc.device, num_beams)
        tokens = torch.empty(B, max_length, dtype=torch.int64, device=enc.device)
        logits = torch.empty(max_length - 1, B, self.cfg["sem_vocab"], dtype=torch.float32, device=enc.device) if return_logits else None
        n = C.c_int()
        enc, u = enc.contiguous(), uniforms.contiguous() if uniforms is not None else None
        head = (self.h, _dev(enc, torch.float32), _dev_or_null(enc_len, torch.int32), B, L, int(max_length))
        tail = (_dev_or_null(u, torch.float32), _dev(tokens), _dev_or_null(logits), C.byref(n), _dev(ws), ws.numel(), _stream())
        if num_beams == 1 and no_repeat_ngram_size == 0:      # the plain decode (lds_lm_generate_opts' wrapper)
            check(lib().lds_lm_generate(*head, o.do_sample, o.top_k, o.top_p, o.temperature, o.repetition_penalty, *tail))
        else:
            check(lib().lds_lm_generate_opts(*head, C.byref(o), *tail))
        toks = tokens[:, : n.value].contiguous()
        return toks, (logits[: n.value - 1] if logits is not None else None)

    def generate_prompt(self, enc, prompt, prompt_len, max_length, do_sample, top_k, top_p, temperature, repetition_penalty, uniforms=None,
                        return_logits=False, enc_len=None, no_repeat_ngram_size=0):
        """Prompted decode (lds_lm_generate_prompt): prompt int64 [B,P] on the device (BOS first, right-padded), prompt_len a sequence of B
        host ints or None (= P everywhere); max_length counts the prompt.  Returns (tokens [B,n] with the prompt in front, logits [steps,B,V]
        or None): logits[s][b] chose row b's s-th generated token, and steps is the largest number of tokens any row generated (rows of the
        library's buffer behind that were chosen by no row)."""
        import torch
        B, L, _ = enc.shape
        P = int(prompt.shape[1])
        o = LMDecodeOpts(1 if do_sample else 0, int(top_k or 0), float(top_p), float(temperature), float(repetition_penalty), int(no_repeat_ngram_size), 1, 1)
        plen = None if prompt_len is None else (C.c_int32 * B)(*[int(v) for v in prompt_len])
        ws = self._workspace("lds_lm_workspace_bytes_prompt", enc.device, B, L, int(max_length), P)
        tokens = torch.empty(B, max_length, dtype=torch.int64, device=enc.device)
        logits = torch.empty(max_length - 1, B, self.cfg["sem_vocab"], dtype=torch.float32, device=enc.device) if return_logits else None
        n = C.c_int()
        enc, prompt, u = enc.contiguous(), prompt.contiguous(), uniforms.contiguous() if uniforms is not None else None
        check(lib().lds_lm_generate_prompt(self.h, _dev(enc, torch.float32), _dev_or_null(enc_len, torch.int32), B, L, int(max_length), C.byref(o),
                                           _dev(prompt, torch.int64), C.cast(plen, C.c_void_p) if plen is not None else None, P,
                                           _dev_or_null(u, torch.float32), _dev(tokens), _dev_or_null(logits), C.byref(n), _dev(ws), ws.numel(), _stream()))
        toks = tokens[:, : n.value].contiguous()
        if logits is None:
            return toks, None
        # every row's generated count: up to and including its EOS behind the prompt, else to the end of the returned rows
        plen = torch.tensor([P] * B if prompt_len is None else [int(v) for v in prompt_len], device=toks.device)
        stop = (toks == self.cfg["sem_eos"]) & (torch.arange(n.value, device=toks.device)[None] >= plen[:, None])
        end = torch.where(stop.any(1), stop.int().argmax(1) + 1, torch.full_like(plen, n.value))
        return toks, logits[: int((end - plen).max())]

    def score(self, enc, semantic, sem_len=None, labels=None, enc_len=None, return_logits=False):
        """Teacher-forced scoring (lds_lm_score): enc [B,L,hidden] from `encode`, semantic / labels [B,T] int64 (labels None = semantic),
        sem_len / enc_len int32 [B] on the device or None.  Returns (logprobs [B,T-1], ranks int32 [B,T-1], loss [], n_counted int32 [],
        logits [B,T,V] or None), all on the device; nothing synchronises."""
        import torch
        B, L, _ = enc.shape
        if semantic.dim() != 2 or semantic.shape[0] != B:
            raise ValueError(f"semantic must be [B, T] with B = {B}, got {tuple(semantic.shape)}")
        T = int(semantic.shape[1])
        if labels is not None and tuple(labels.shape) != (B, T):
            raise ValueError(f"labels must have semantic's shape {(B, T)}, got {tuple(labels.shape)}")
        enc, sem = enc.contiguous(), semantic.contiguous()
        lab = labels.contiguous() if labels is not None else None
        ws = self._workspace("lds_lm_score_workspace_bytes", enc.device, B, L, T)
        lp = torch.empty(B, T - 1, dtype=torch.float32, device=enc.device)
        ranks = torch.empty(B, T - 1, dtype=torch.int32, device=enc.device)
        loss = torch.empty((), dtype=torch.float32, device=enc.device)
        n = torch.empty((), dtype=torch.int32, device=enc.device)
        logits = torch.empty(B, T, self.cfg["sem_vocab"], dtype=torch.float32, device=enc.device) if return_logits else None
        check(lib().lds_lm_score(self.h, _dev(enc, torch.float32), _dev_or_null(enc_len, torch.int32), B, L, _dev(sem, torch.int64),
                                 _dev_or_null(sem_len, torch.int32), _dev_or_null(lab, torch.int64), T, _dev(lp), _dev(ranks), _dev(loss), _dev(n),
                                 _dev_or_null(logits), _dev(ws), ws.numel(), _stream()))
        return lp, ranks, loss, n, logits


class LlamaCfg(C.Structure):
    _fields_ = [("hidden", C.c_int), ("heads", C.c_int), ("kv_heads", C.c_int), ("head_dim", C.c_int), ("inter", C.c_int), ("layers", C.c_int),
                ("vocab", C.c_int), ("max_pos", C.c_int), ("eps", C.c_float), ("rope_theta", C.c_float), ("first_free_id", C.c_int), ("bos", C.c_int),
                ("eos", C.c_int), ("pad", C.c_int)]


class Llama(_Handle):
    """text2semantic Llama (lds_llama_*): causal prefill of the prompts + cached decode loop."""
    KIND = "llama"

    def __init__(self, cfg, state):
        """cfg: arch.llama_config; state: Llama.state_dict() (+ llama.model.rotary_emb.inv_freq, HF's inverse frequencies)"""
        c = LlamaCfg()
        c.hidden, c.heads, c.kv_heads, c.head_dim, c.inter, c.layers = cfg["hidden"], cfg["heads"], cfg["kv_heads"], cfg["head_dim"], cfg["inter"], cfg["layers"]
        c.vocab, c.max_pos, c.eps, c.rope_theta = cfg["vocab"], cfg["max_pos"], cfg["eps"], cfg["rope_theta"]
        c.first_free_id, c.bos, c.eos, c.pad = cfg["shift"], cfg["bos"], cfg["eos"], cfg["pad"]
        self._create_weights(c, state)
        self.cfg = cfg

    def generate(self, input_ids, in_len, max_length, do_sample, top_k, top_p, temperature, repetition_penalty, uniforms=None, return_logits=False,
                 no_repeat_ngram_size=0, num_beams=1):
        """input_ids int64 [B,P] on the device (right-padded), in_len a sequence of B host ints or None (= P everywhere); max_length counts the
        prompt.  Returns (tokens [B,n], ids of the model's vocabulary with the prompt in front, logits [steps,B,vocab - shift] or None):
        logits[s][b] chose row b's s-th generated token; steps is the largest number of tokens any row generated."""
        import torch
        B, P = input_ids.shape
        o = LMDecodeOpts(1 if do_sample else 0, int(top_k or 0), float(top_p), float(temperature), float(repetition_penalty), int(no_repeat_ngram_size),
                         int(num_beams), 1)
        plen = None if in_len is None else (C.c_int32 * B)(*[int(v) for v in in_len])
        ws = self._workspace("lds_llama_workspace_bytes", input_ids.device, B, P, int(max_length))
        tokens = torch.empty(B, max_length, dtype=torch.int64, device=input_ids.device)
        V = self.cfg["vocab"] - self.cfg["shift"]
        logits = torch.empty(max_length - 1, B, V, dtype=torch.float32, device=input_ids.device) if return_logits else None
        n = C.c_int()
        ids, u = input_ids.contiguous(), uniforms.contiguous() if uniforms is not None else None
        check(lib().lds_llama_generate(self.h, _dev(ids, torch.int64), C.cast(plen, C.c_void_p) if plen is not None else None, B, P, int(max_length), C.byref(o),
                                       _dev_or_null(u, torch.float32), _dev(tokens), _dev_or_null(logits), C.byref(n), _dev(ws), ws.numel(), _stream()))
        toks = tokens[:, : n.value].contiguous()
        if logits is None:
            return toks, None
        plen = torch.tensor([P] * B if in_len is None else [int(v) for v in in_len], device=toks.device)
        stop = (toks == self.cfg["eos"]) & (torch.arange(n.value, device=toks.device)[None] >= plen[:, None])
        end = torch.where(stop.any(1), stop.int().argmax(1) + 1, torch.full_like(plen, n.value))
        return toks, logits[: int((end - plen).max())]

    def generate_beam(self, input_ids, in_len, max_length, num_beams, repetition_penalty=1.0, no_repeat_ngram_size=0, early_stopping=True):
        """Greedy beam search (lds_llama_generate_beam): input_ids / in_len / max_length as `generate`, one row per item; early_stopping True,
        False or "never".  Returns tokens [B,n]: every item's prompt and best finished hypothesis (EOS kept, PAD after it), n the longest row."""
        import torch
        B, P = input_ids.shape
        o = LMDecodeOpts(0, 0, 1.0, 1.0, float(repetition_penalty), int(no_repeat_ngram_size), int(num_beams), EARLY_STOPPING.get(early_stopping, -1))
        plen = None if in_len is None else (C.c_int32 * B)(*[int(v) for v in in_len])
        ws = self._workspace("lds_llama_beam_workspace_bytes", input_ids.device, B, P, int(max_length), int(num_beams))
        tokens = torch.empty(B, max_length, dtype=torch.int64, device=input_ids.device)
        n = C.c_int()
        ids = input_ids.contiguous()
        check(lib().lds_llama_generate_beam(self.h, _dev(ids, torch.int64), C.cast(plen, C.c_void_p) if plen is not None else None, B, P, int(max_length),
                                            C.byref(o), _dev(tokens), C.byref(n), _dev(ws), ws.numel(), _stream()))
        return tokens[:, : n.value].contiguous()

    def score(self, input_ids, ids_len=None, labels=None, return_logits=False):
        """Teacher-forced scoring (lds_llama_score): input_ids / labels int64 [B,S] on the device (labels None = input_ids), ids_len int32 [B]
        on the device or None.  Returns (logprobs [B,S-1], ranks int32 [B,S-1], loss [], n_counted int32 [], logits [B,S,vocab] or None), all
        on the device; nothing synchronises."""
        import torch
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, S], got {tuple(input_ids.shape)}")
        B, S = (int(v) for v in input_ids.shape)
        if labels is not None and tuple(labels.shape) != (B, S):
            raise ValueError(f"labels must have input_ids' shape {(B, S)}, got {tuple(labels.shape)}")
        ids = input_ids.contiguous()
        lab = labels.contiguous() if labels is not None else None
        ws = self._workspace("lds_llama_score_workspace_bytes", ids.device, B, S)
        lp = torch.empty(B, S - 1, dtype=torch.float32, device=ids.device)
        ranks = torch.empty(B, S - 1, dtype=torch.int32, device=ids.device)
        loss = torch.empty((), dtype=torch.float32, device=ids.device)
        n = torch.empty((), dtype=torch.int32, device=ids.device)
        logits = torch.empty(B, S, self.cfg["vocab"], dtype=torch.float32, device=ids.device) if return_logits else None
        check(lib().lds_llama_score(self.h, _dev(ids, torch.int64), _dev_or_null(ids_len, torch.int32), _dev_or_null(lab, torch.int64), B, S, _dev(lp),
                                    _dev(ranks), _dev(loss), _dev(n), _dev_or_null(logits), _dev(ws), ws.numel(), _stream()))
        return lp, ranks, loss, n, logits


class WhisperDecoder(_Handle):
    """Whisper's text decoder (lds_whisper_decoder_*): cross keys / values once per batch of clips, then teacher-forced logits / scores or
    the greedy cached decode over them."""
    KIND = "whisper_decoder"

    def __init__(self, n_vocab, n_text_ctx, n_state, n_head, n_layer, n_audio_ctx, state):
        """state: OpenAI Whisper's checkpoint keys ("decoder.token_embedding.weight", ...) -> fp32 CPU tensors / arrays"""
        c = WhisperDecoderCfg(int(n_vocab), int(n_text_ctx), int(n_state), int(n_head), int(n_layer), int(n_audio_ctx))
        self._create_weights(c, state)
        self.n_vocab, self.n_text_ctx, self.n_state, self.n_audio_ctx = int(n_vocab), int(n_text_ctx), int(n_state), int(n_audio_ctx)
        self._cross = None      # (device, stream, B, T) of the batch whose cross keys / values the workspace holds

    def workspace_bytes(self, B, T, S):
        return _bytes("lds_whisper_decoder_workspace_bytes", self.h, int(B), int(T), int(S))

    def _ws(self, device, B, T, S):
        """the current stream's buffer, large enough for S positions.  A buffer that had to grow has lost the cross part: it is recomputed
        from the units of the last `cross` call."""
        import torch
        key = (str(device), int(torch.cuda.current_stream(device).cuda_stream), B, T)
        if self._cross is None or self._cross[0] != key:
            raise RuntimeError("WhisperDecoder: call cross(units, n_frames) for this batch (and on this stream) first")
        ws = self.ws.get(self.workspace_bytes(B, T, S), device)
        if ws.data_ptr() != self._cross[1]:
            self._run_cross(ws, *self._cross[2:])
        return ws

    def _run_cross(self, ws, units, nf):
        B, T, _ = units.shape
        check(lib().lds_whisper_decoder_cross(self.h, _dev(units, _f32()), _host(nf), B, T, _dev(ws), ws.numel(), _stream()))
        self._cross = (self._cross[0], ws.data_ptr(), units, nf)

    def cross(self, units, n_frames=None, S=None):
        """units fp32 [B,T,n_state] on the device (the audio encoder's output), n_frames B host ints (1 .. T) or None.  S: the text positions
        the later calls will need (default n_text_ctx), so that the buffer does not have to grow behind the cross part."""
        import torch
        if units.dim() != 3 or units.shape[2] != self.n_state:
            raise ValueError(f"units must be [B, T, {self.n_state}], got {tuple(units.shape)}")
        B, T = int(units.shape[0]), int(units.shape[1])
        nf = None if n_frames is None else _host_lengths(n_frames, B, 1, T, 64, "decoder")
        units = units.contiguous()
        ws = self.ws.get(self.workspace_bytes(B, T, self.n_text_ctx if S is None else int(S)), units.device)
        self._cross = ((str(units.device), int(torch.cuda.current_stream(units.device).cuda_stream), B, T), None, None, None)
        self._run_cross(ws, units, nf)

    def logits(self, tokens, tok_len=None, labels=None, return_logits=True, score=False):
        """tokens int64 [B,S] on the device, tok_len int32 [B] on the device or None.  Returns logits [B,S,n_vocab] (return_logits), or with
        score=True the tuple (logprobs [B,S-1], ranks int32 [B,S-1], loss [], n_counted int32 [], logits or None)."""
        import torch
        if tokens.dim() != 2:
            raise ValueError(f"tokens must be [B, S], got {tuple(tokens.shape)}")
        B, S = (int(v) for v in tokens.shape)
        if labels is not None and tuple(labels.shape) != (B, S):
            raise ValueError(f"labels must have tokens' shape {(B, S)}, got {tuple(labels.shape)}")
        if self._cross is None:
            raise RuntimeError("WhisperDecoder: call cross(units, n_frames) first")
        T = self._cross[0][3]
        if self._cross[0][2] != B:
            raise ValueError(f"tokens hold {B} rows, the cross keys {self._cross[0][2]}")
        dev = tokens.device
        ids = tokens.contiguous()
        lab = labels.contiguous() if labels is not None else None
        lg = torch.empty(B, S, self.n_vocab, dtype=torch.float32, device=dev) if return_logits else None
        lp = ranks = loss = n = None
        if score:
            lp = torch.empty(B, S - 1, dtype=torch.float32, device=dev)
            ranks = torch.empty(B, S - 1, dtype=torch.int32, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            n = torch.empty((), dtype=torch.int32, device=dev)
        ws = self._ws(dev, B, T, S)
        check(lib().lds_whisper_decoder_logits(self.h, _dev(ids, torch.int64), _dev_or_null(tok_len, torch.int32), _dev_or_null(lab, torch.int64), B, S, T,
                                               _dev_or_null(lg), _dev_or_null(lp), _dev_or_null(ranks), _dev_or_null(loss), _dev_or_null(n), _dev(ws),
                                               ws.numel(), _stream()))
        return (lp, ranks, loss, n, lg) if score else lg

    def generate(self, prompt, prompt_len, max_new_tokens, eos, pad, suppress=None, begin_suppress=None, return_logits=False, cap=None,
                 no_repeat_ngram_size=0, num_beams=1, temperature=0.0):
        """Greedy decode.  prompt int64 [B,P] on the device, prompt_len B host ints (1 .. P); suppress / begin_suppress: id lists or None.
        cap: the sequences' capacity (default min(max(prompt_len) + max_new_tokens, n_text_ctx)).  Returns (tokens [B,n] with the prompt in
        front, EOS kept, PAD after it; token_logprob [B,max_new_tokens]; sum_logprob [B]; logits [steps,B,n_vocab] or None)."""
        import torch
        if prompt.dim() != 2:
            raise ValueError(f"prompt must be [B, P], got {tuple(prompt.shape)}")
        B, P = (int(v) for v in prompt.shape)
        if self._cross is None:
            raise RuntimeError("WhisperDecoder: call cross(units, n_frames) first")
        T = self._cross[0][3]
        if self._cross[0][2] != B:
            raise ValueError(f"prompt holds {B} rows, the cross keys {self._cross[0][2]}")
        pl = _host_lengths(prompt_len, B, 1, P)
        max_new = int(max_new_tokens)
        if cap is None:
            cap = min(int(pl.max()) + max(max_new, 1), self.n_text_ctx)
        cap = int(cap)
        dev = prompt.device
        lists = [None if v is None or len(v) == 0 else torch.as_tensor(list(v), dtype=torch.int32).to(dev) for v in (suppress, begin_suppress)]
        o = WhisperDecodeOpts(max_new, int(eos), int(pad), int(no_repeat_ngram_size), lists[0].data_ptr() if lists[0] is not None else None,
                              lists[1].data_ptr() if lists[1] is not None else None, 0 if lists[0] is None else lists[0].numel(),
                              0 if lists[1] is None else lists[1].numel(), int(num_beams), float(temperature))
        ids = prompt.contiguous()
        tokens = torch.empty(B, max(cap, 1), dtype=torch.int64, device=dev)
        tlp = torch.empty(B, max(max_new, 1), dtype=torch.float32, device=dev)
        slp = torch.empty(B, dtype=torch.float32, device=dev)
        lg = torch.empty(max(max_new, 1), B, self.n_vocab, dtype=torch.float32, device=dev) if return_logits else None
        n = C.c_int()
        # (the shape refusals come from the library, before anything is enqueued; the workspace is sized only for shapes it takes)
        ok = 1 <= B <= 64 and 2 <= cap <= self.n_text_ctx
        ws = self._ws(dev, B, T, cap) if ok else torch.empty(256, dtype=torch.uint8, device=dev)
        check(lib().lds_whisper_decoder_generate(self.h, _dev(ids, torch.int64), _host(pl), B, P, T, cap, C.byref(o), _dev(tokens), _dev(tlp), _dev(slp),
                                                 _dev_or_null(lg), C.byref(n), _dev(ws), ws.numel(), _stream()))
        toks = tokens[:, : n.value].contiguous()
        steps = max(1, n.value - int(pl.min()))
        return toks, tlp, slp, (lg[:steps] if lg is not None else None)


def _f32():
    import torch
    return torch.float32


def whisper_head_test(x, ln_g, ln_b, et, suppress=None, return_logits=False):
    """lds_test_whisper_head: x [N,K], ln_g / ln_b [K], et [K,V] fp32 on the device, suppress an id list or None ->
    (token int64 [N], logprob [N], lse [N], logits [N,V] or None)"""
    import torch
    N, K = (int(v) for v in x.shape)
    V = int(et.shape[1])
    dev = x.device
    sup = None if suppress is None or len(suppress) == 0 else torch.as_tensor(list(suppress), dtype=torch.int32).to(dev)
    tok = torch.empty(N, dtype=torch.int64, device=dev)
    lp = torch.empty(N, dtype=torch.float32, device=dev)
    lse = torch.empty(N, dtype=torch.float32, device=dev)
    lg = torch.empty(N, V, dtype=torch.float32, device=dev) if return_logits else None
    check(lib().lds_test_whisper_head(_dev(x.contiguous(), torch.float32), _dev(ln_g.contiguous(), torch.float32), _dev(ln_b.contiguous(), torch.float32),
                                      _dev(et.contiguous(), torch.float32), N, K, V, _dev_or_null(sup, torch.int32), 0 if sup is None else sup.numel(),
                                      _dev(tok), _dev(lp), _dev(lse), _dev_or_null(lg), _stream()))
    return tok, lp, lse, lg


# ---- k-means semantic tokenizer (lds_kmeans_*): thin wrappers; X [N, D] and C [K, D] contiguous fp32 device tensors ----
_kmeans_ws = Workspace()


def kmeans_workspace_bytes(N, K, D):
    return _bytes("lds_kmeans_workspace_bytes", int(N), int(K), int(D))


def _kmeans_ws_for(ws, N, K, D, device):
    if device.type != "cuda":
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    return ws if ws is not None else _kmeans_ws.get(kmeans_workspace_bytes(N, K, D), device)


def kmeans_prepare(centers, metric="l2"):
    """h [K] = |c_k|^2 / 2 of a codebook [K, D] (once per codebook); metric="cosine": the row constants 1 / max(|c_k|, 1e-12)"""
    import torch
    m = metric_code(metric)
    K, D = centers.shape
    h = torch.empty(K, dtype=torch.float32, device=centers.device)
    if m == 0:
        check(lib().lds_kmeans_prepare(_dev(centers, torch.float32), K, D, _dev(h), _stream()))
    else:
        check(lib().lds_kmeans_prepare_metric(_dev(centers, torch.float32), K, D, m, _dev(h), _stream()))
    return h


def kmeans_assign(x, centers, h, return_best=False, ws=None, lengths=None, pad_id=0, metric="l2"):
    """x [N, D] -> labels int64 [N] (the nearest centre, lowest index among ties) and optionally the winning score x.c - h.
    lengths (host ints [B], 0 .. T) with x [B, T, D]: the ragged form, labels [B, T] with pad_id at and beyond every clip's length.
    metric="cosine" (h from kmeans_prepare(.., "cosine")): the centre of highest cosine similarity, and that similarity as the score."""
    import torch
    m = metric_code(metric)
    K, D = centers.shape
    if x.shape[-1] != D or x.dim() != (3 if lengths is not None else 2):
        raise ValueError(f"kmeans_assign: x {list(x.shape)} against a codebook {[K, D]}")
    N = x.numel() // D
    ws = _kmeans_ws_for(ws, N, K, D, x.device)
    labels = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    best = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if return_best else None
    ln = None if lengths is None else _host_lengths(lengths, x.shape[0], 0, x.shape[1])
    fn, ln_at = _dense_or_ragged("lds_kmeans_assign", ln, suffix="_metric" if m else "")
    rows = (N,) if ln is None else (x.shape[0], x.shape[1], *ln_at, int(pad_id))
    check(fn(_dev(x, torch.float32), *rows, _dev(centers, torch.float32), _dev(h, torch.float32), K, D, *((m,) if m else ()), _dev(labels),
             _dev_or_null(best), _dev(ws), ws.numel(), _stream()))
    return (labels, best) if return_best else labels


def kmeans_update(x, labels, centers, h, num_points, ws=None, metric="l2"):
    """one Lloyd step in place on centers / h / num_points (include/lds.h lds_kmeans_update); returns the error as a device scalar.
    metric decides only what h is refreshed to (kmeans_prepare's)"""
    import torch
    m = metric_code(metric)
    K, D = centers.shape
    N = x.shape[0]
    if x.dim() != 2 or x.shape[1] != D or labels.shape != (N,) or num_points.shape != (K,) or h.shape != (K,):
        raise ValueError("kmeans_update: shapes of x, labels, centers, h, num_points do not agree")
    ws = _kmeans_ws_for(ws, N, K, D, x.device)
    err = torch.empty((), dtype=torch.float32, device=x.device)
    fn = lib().lds_kmeans_update_metric if m else lib().lds_kmeans_update
    check(fn(_dev(x, torch.float32), _dev(labels, torch.int64), N, _dev(centers, torch.float32), _dev(h, torch.float32), _dev(num_points, torch.float32),
             K, D, *((m,) if m else ()), _dev(err), _dev(ws), ws.numel(), _stream()))
    return err


def kmeans_seed(x, K, first_index, uniforms, ws=None):
    """k-means++ seeding: x [N, D], uniforms fp32 device [K - 1] -> (centers [K, D], picked int64 [K]) on the device"""
    import torch
    N, D = x.shape
    ws = _kmeans_ws_for(ws, N, K, D, x.device)
    centers = torch.empty(K, D, dtype=torch.float32, device=x.device)
    picked = torch.empty(K, dtype=torch.int64, device=x.device)
    if K > 1 and uniforms.numel() != K - 1:
        raise ValueError(f"kmeans_seed: {K - 1} uniforms needed, got {uniforms.numel()}")
    check(lib().lds_kmeans_seed(_dev(x, torch.float32), N, D, int(K), int(first_index), _dev(uniforms, torch.float32) if K > 1 else None, _dev(centers),
                                _dev(picked), _dev(ws), ws.numel(), _stream()))
    return centers, picked


# ---- units retrieval (lds_knn_*): thin wrappers; x [N, D] (or [B, T, D] with lengths) and pool [M, D] contiguous fp32 device tensors ----
_knn_ws = Workspace()


def knn_workspace_bytes(N, M, D, k):
    return _bytes("lds_knn_workspace_bytes", int(N), int(M), int(D), int(k))


def _knn_ws_for(ws, N, M, D, k, device):
    if device.type != "cuda":
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    return ws if ws is not None else _knn_ws.get(knn_workspace_bytes(N, M, D, k), device)


def knn_prepare(pool, metric="l2"):
    """h [M] = |p_m|^2 / 2 of a pool [M, D] (once per pool); metric="cosine": the row constants 1 / max(|p_m|, 1e-12)"""
    import torch
    m = metric_code(metric)
    M, D = pool.shape
    h = torch.empty(M, dtype=torch.float32, device=pool.device)
    if m == 0:
        check(lib().lds_knn_prepare(_dev(pool, torch.float32), M, D, _dev(h), _stream()))
    else:
        check(lib().lds_knn_prepare_metric(_dev(pool, torch.float32), M, D, m, _dev(h), _stream()))
    return h


def knn_search(x, pool, h, k, ws=None, slab_rows=None, splits=None, metric="l2"):
    """x [N, D] -> (idx int32 [N, k], score [N, k]): the k nearest pool rows, nearest first, the lower index among equal scores.
    slab_rows / splits (both or neither): the pool's cut forced through lds_test_knn_search; `ws` must then be given.
    metric="cosine" (h from knn_prepare(.., "cosine")): by cosine similarity, which is then the score"""
    import torch
    m = metric_code(metric)
    mm, sfx = ((m,) if m else ()), ("_metric" if m else "")
    M, D = pool.shape
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"knn_search: x {list(x.shape)} against a pool {[M, D]}")
    N = x.shape[0]
    idx = torch.empty(N, k, dtype=torch.int32, device=x.device)
    score = torch.empty(N, k, dtype=torch.float32, device=x.device)
    head = (_dev(x, torch.float32), N, _dev(pool, torch.float32), _dev(h, torch.float32), M, D, int(k))
    if slab_rows is None:
        ws = _knn_ws_for(ws, N, M, D, k, x.device)
        check(getattr(lib(), "lds_knn_search" + sfx)(*head, *mm, _dev(idx), _dev(score), _dev(ws), ws.numel(), _stream()))
    else:
        check(getattr(lib(), "lds_test_knn_search" + sfx)(*head, *mm, int(slab_rows), int(splits), _dev(idx), _dev(score), _dev(ws), ws.numel(), _stream()))
    return idx, score


def _metric_args(metric, weights):
    """((metric, weights) codes for a *_metric entry or () for its namesake, the entry's suffix): l2 with inverse_square is the namesake"""
    m, w = metric_code(metric), metric_code(weights, "weights", WEIGHTS)
    return ((m, w), "_metric") if (m or w) else ((), "")


def knn_retrieve(x, pool, h, k, ratio, lengths=None, ws=None, metric="l2", weights="inverse_square"):
    """x [N, D], or [B, T, D] with lengths (host ints [B], 0 .. T) -> (y like x, idx int32 [.., k], dist [.., k]): every row blended with its
    k nearest pool rows (include/lds.h lds_knn_retrieve); rows at and beyond a clip's length: y = 0, idx = -1, dist = 0.
    metric / weights: include/lds.h lds_knn_retrieve_metric (cosine: dist = 1 - cos; uniform: the plain mean of the rows found)"""
    import torch
    mw, sfx = _metric_args(metric, weights)
    M, D = pool.shape
    if x.shape[-1] != D or x.dim() != (3 if lengths is not None else 2):
        raise ValueError(f"knn_retrieve: x {list(x.shape)} against a pool {[M, D]}")
    N = x.numel() // D
    ws = _knn_ws_for(ws, N, M, D, k, x.device)
    y = torch.empty_like(x)
    idx = torch.empty(*x.shape[:-1], k, dtype=torch.int32, device=x.device)
    dist = torch.empty(*x.shape[:-1], k, dtype=torch.float32, device=x.device)
    ln = None if lengths is None else _host_lengths(lengths, x.shape[0], 0, x.shape[1], max_B=64, what="retrieval")
    fn, ln_at = _dense_or_ragged("lds_knn_retrieve", ln, suffix=sfx)
    rows = (N,) if ln is None else (x.shape[0], x.shape[1], *ln_at)
    check(fn(_dev(x, torch.float32), *rows, _dev(pool, torch.float32), _dev(h, torch.float32), M, D, int(k), *mw, float(ratio), _dev(y), _dev(idx),
             _dev(dist), _dev(ws), ws.numel(), _stream()))
    return y, idx, dist


# ---- units retrieval through an IVF coarse index (lds_ivf_*): `ivf` is the tuple (centres [nlist, D], hc [nlist], offsets int64 [nlist + 1],
# order int32 [M], copy [copy_rows, D], hl [copy_rows]) on the device (cluster.index.UnitsIndex.build_ivf makes it) ----
_ivf_ws = Workspace()


def ivf_workspace_bytes(N, M, D, k, nlist, nprobe):
    return _bytes("lds_ivf_workspace_bytes", int(N), int(M), int(D), int(k), int(nlist), int(nprobe))


def _ivf_args(ivf, nprobe):
    import torch
    centres, hc, offsets, order, copy, hl = ivf
    return (_dev(centres, torch.float32), _dev(hc, torch.float32), centres.shape[0], _dev(offsets, torch.int64), _dev(order, torch.int32),
            _dev(copy, torch.float32), _dev(hl, torch.float32), copy.shape[0], int(nprobe))


def _ivf_ws_for(ws, N, M, D, k, ivf, nprobe, device):
    if device.type != "cuda":
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    return ws if ws is not None else _ivf_ws.get(ivf_workspace_bytes(N, M, D, k, ivf[0].shape[0], nprobe), device)


def ivf_search(x, pool, h, k, ivf, nprobe, ws=None, slab_rows=None, metric="l2"):
    """x [N, D] -> (idx int32 [N, k], score [N, k]): the k best rows among the query's nprobe probed lists (include/lds.h lds_ivf_search);
    -1 / -inf where the lists hold fewer than k rows.  slab_rows: the copy's cut forced through lds_test_ivf_search.
    metric: the one the whole index (h, hc, hl, the lists) was built for"""
    import torch
    m = metric_code(metric)
    mm, sfx = ((m,) if m else ()), ("_metric" if m else "")
    M, D = pool.shape
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"ivf_search: x {list(x.shape)} against a pool {[M, D]}")
    N = x.shape[0]
    ws = _ivf_ws_for(ws, N, M, D, k, ivf, nprobe, x.device)
    idx = torch.empty(N, k, dtype=torch.int32, device=x.device)
    score = torch.empty(N, k, dtype=torch.float32, device=x.device)
    head = (_dev(x, torch.float32), N, _dev(pool, torch.float32), _dev(h, torch.float32), M, D, int(k), *_ivf_args(ivf, nprobe))
    tail = (_dev(idx), _dev(score), _dev(ws), ws.numel(), _stream())
    if slab_rows is None:
        check(getattr(lib(), "lds_ivf_search" + sfx)(*head, *mm, *tail))
    else:
        check(getattr(lib(), "lds_test_ivf_search" + sfx)(*head, *mm, int(slab_rows), *tail))
    return idx, score


def ivf_retrieve(x, pool, h, k, ratio, ivf, nprobe, lengths=None, ws=None, metric="l2", weights="inverse_square"):
    """knn_retrieve over the rows of every query's nprobe probed lists (include/lds.h lds_ivf_retrieve); idx = -1 (weight 0) where the
    lists hold fewer than k rows.  metric (the index's) / weights: include/lds.h lds_ivf_retrieve_metric"""
    import torch
    mw, sfx = _metric_args(metric, weights)
    M, D = pool.shape
    if x.shape[-1] != D or x.dim() != (3 if lengths is not None else 2):
        raise ValueError(f"ivf_retrieve: x {list(x.shape)} against a pool {[M, D]}")
    N = x.numel() // D
    ws = _ivf_ws_for(ws, N, M, D, k, ivf, nprobe, x.device)
    y = torch.empty_like(x)
    idx = torch.empty(*x.shape[:-1], k, dtype=torch.int32, device=x.device)
    dist = torch.empty(*x.shape[:-1], k, dtype=torch.float32, device=x.device)
    ln = None if lengths is None else _host_lengths(lengths, x.shape[0], 0, x.shape[1], max_B=64, what="retrieval")
    fn, ln_at = _dense_or_ragged("lds_ivf_retrieve", ln, suffix=sfx)
    rows = (N,) if ln is None else (x.shape[0], x.shape[1], *ln_at)
    check(fn(_dev(x, torch.float32), *rows, _dev(pool, torch.float32), _dev(h, torch.float32), M, D, int(k), *_ivf_args(ivf, nprobe), *mw, float(ratio),
             _dev(y), _dev(idx), _dev(dist), _dev(ws), ws.numel(), _stream()))
    return y, idx, dist


# ---- polyphase resampler (lds_resample*): the filter of one (orig, new, width, rolloff) is built once on the host (arch.resample_bank) and
# uploaded once per device ----
_resample_tables = {}


# ---- CTC heads (lds_ctc_*): thin wrappers; units [B, T, D], weight [V, D], bias [V] contiguous fp32 device tensors ----
_ctc_ws = Workspace()
CTC_MAX_LABELS = 511


def _ctc_ws_for(ws, entry, dims, device):
    if device.type != "cuda":
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    nb = _bytes(entry, *dims)
    if ws is not None and ws.numel() < nb:
        raise ValueError(f"{entry[:-16]}: workspace of {ws.numel()} bytes, {nb} needed")
    return ws if ws is not None else _ctc_ws.get(nb, device)


def _ctc_units(units, n_frames, weight):
    if units.dim() != 3 or weight.dim() != 2 or units.shape[-1] != weight.shape[1]:
        raise ValueError(f"ctc: units {list(units.shape)} against a head {list(weight.shape)}")
    B, T, D = units.shape
    if T < 1:
        raise ValueError("ctc: no frames")
    return B, T, D, weight.shape[0], _host_lengths(n_frames, B, 0, T, 64, "CTC")


def ctc_head(units, n_frames, weight, bias, return_logprobs=False, ws=None):
    """units [B, T, D], n_frames (host ints [B], 0 .. T) -> (arg int32 [B, T], m, lse fp32 [B, T][, log-probs [B, T, V]]): per valid frame
    the arg-max of the logits (lowest id among ties), its logit and the log-sum-exp (include/lds.h lds_ctc_head)"""
    import torch
    B, T, D, V, nf = _ctc_units(units, n_frames, weight)
    ws = _ctc_ws_for(ws, "lds_ctc_head_workspace_bytes", (B, T, V, D), units.device)
    arg = torch.empty(B, T, dtype=torch.int32, device=units.device)
    m, lse = torch.empty(B, T, dtype=torch.float32, device=units.device), torch.empty(B, T, dtype=torch.float32, device=units.device)
    lp = torch.empty(B, T, V, dtype=torch.float32, device=units.device) if return_logprobs else None
    check(lib().lds_ctc_head(_dev(units, torch.float32), B, T, _host(nf), _dev(weight, torch.float32), _dev(bias, torch.float32), V, D, _dev(arg), _dev(m),
                             _dev(lse), _dev_or_null(lp), _dev(ws), ws.numel(), _stream()))
    return (arg, m, lse, lp) if return_logprobs else (arg, m, lse)


def ctc_greedy(arg, m, lse, n_frames, blank, pad_id=-1):
    """ctc_head's outputs -> (tokens int64 [B, T], n_tokens int32 [B], start, length int32 [B, T], logprob fp32 [B, T]): runs of equal arg
    collapsed, blank dropped (include/lds.h lds_ctc_greedy)"""
    import torch
    B, T = arg.shape
    nf = _host_lengths(n_frames, B, 0, T, 64, "CTC")
    dev = arg.device
    tokens = torch.empty(B, T, dtype=torch.int64, device=dev)
    n_tokens = torch.empty(B, dtype=torch.int32, device=dev)
    start, length = torch.empty(B, T, dtype=torch.int32, device=dev), torch.empty(B, T, dtype=torch.int32, device=dev)
    logprob = torch.empty(B, T, dtype=torch.float32, device=dev)
    check(lib().lds_ctc_greedy(_dev(arg, torch.int32), _dev(m, torch.float32), _dev(lse, torch.float32), B, T, _host(nf), int(blank), int(pad_id), _dev(tokens),
                               _dev(n_tokens), _dev(start), _dev(length), _dev(logprob), _stream()))
    return tokens, n_tokens, start, length, logprob


def _ctc_labels(labels, label_len, B):
    """labels int64 [B, Lmax] (device), label_len host ints -> (labels, host int32 [B], Lmax); an empty label matrix becomes one unused column"""
    import torch
    if labels.dim() != 2 or labels.shape[0] != B:
        raise ValueError(f"ctc: labels {list(labels.shape)} for {B} clips")
    if labels.shape[1] > CTC_MAX_LABELS:
        raise ValueError(f"ctc: at most {CTC_MAX_LABELS} labels per clip (got {labels.shape[1]})")
    ll = _host_lengths(label_len, B, 0, labels.shape[1])
    if labels.shape[1] == 0:
        labels = torch.zeros(B, 1, dtype=torch.int64, device=labels.device)
    return labels, ll, labels.shape[1]


def ctc_score(units, n_frames, weight, bias, blank, labels, label_len, ws=None):
    """nll fp32 [B] = -log p(labels_b | units_b) by the CTC forward recursion (include/lds.h lds_ctc_score)"""
    import torch
    B, T, D, V, nf = _ctc_units(units, n_frames, weight)
    labels, ll, Lmax = _ctc_labels(labels, label_len, B)
    ws = _ctc_ws_for(ws, "lds_ctc_score_workspace_bytes", (B, T, V, D, Lmax), units.device)
    nll = torch.empty(B, dtype=torch.float32, device=units.device)
    check(lib().lds_ctc_score(_dev(units, torch.float32), B, T, _host(nf), _dev(weight, torch.float32), _dev(bias, torch.float32), V, D, int(blank),
                              _dev(labels, torch.int64), _host(ll), Lmax, _dev(nll), _dev(ws), ws.numel(), _stream()))
    return nll


def _ctc_align_outputs(B, T, Lmax, device):
    import torch
    return (torch.empty(B, dtype=torch.float32, device=device), torch.empty(B, T, dtype=torch.int32, device=device),
            torch.empty(B, Lmax, 2, dtype=torch.int32, device=device), torch.empty(B, Lmax, dtype=torch.float32, device=device))


def ctc_align(units, n_frames, weight, bias, blank, labels, label_len, ws=None):
    """the Viterbi alignment: (path_score [B], frame_label int32 [B, T], segments int32 [B, Lmax, 2], label_logprob [B, Lmax])
    (include/lds.h lds_ctc_align)"""
    import torch
    B, T, D, V, nf = _ctc_units(units, n_frames, weight)
    labels, ll, Lmax = _ctc_labels(labels, label_len, B)
    ws = _ctc_ws_for(ws, "lds_ctc_align_workspace_bytes", (B, T, V, D, Lmax), units.device)
    ps, fl, seg, llp = _ctc_align_outputs(B, T, Lmax, units.device)
    check(lib().lds_ctc_align(_dev(units, torch.float32), B, T, _host(nf), _dev(weight, torch.float32), _dev(bias, torch.float32), V, D, int(blank),
                              _dev(labels, torch.int64), _host(ll), Lmax, _dev(ps), _dev(fl), _dev(seg), _dev(llp), _dev(ws), ws.numel(), _stream()))
    return ps, fl, seg, llp


def ctc_test_forward(E, n_frames, labels, label_len):
    """the forward recursion alone on ready emissions E [B, T, Lmax + 1] (include/lds_test.h)"""
    import torch
    B, T, W1 = E.shape
    nf = _host_lengths(n_frames, B, 0, T, 64, "CTC")
    ll = _host_lengths(label_len, B, 0, W1 - 1)
    assert tuple(labels.shape) == (B, W1 - 1)
    nll = torch.empty(B, dtype=torch.float32, device=E.device)
    check(lib().lds_test_ctc_forward(_dev(E, torch.float32), B, T, _host(nf), _dev(labels, torch.int64), _host(ll), W1 - 1, _dev(nll), _stream()))
    return nll


def ctc_test_viterbi(E, n_frames, labels, label_len, ws=None):
    """the Viterbi recursion and backtrace alone on ready emissions E [B, T, Lmax + 1] (include/lds_test.h)"""
    import torch
    B, T, W1 = E.shape
    nf = _host_lengths(n_frames, B, 0, T, 64, "CTC")
    ll = _host_lengths(label_len, B, 0, W1 - 1)
    assert tuple(labels.shape) == (B, W1 - 1)
    if ws is None:
        ws = _ctc_ws.get(B * T * 256, E.device)
    ps, fl, seg, llp = _ctc_align_outputs(B, T, W1 - 1, E.device)
    check(lib().lds_test_ctc_viterbi(_dev(E, torch.float32), B, T, _host(nf), _dev(labels, torch.int64), _host(ll), W1 - 1, _dev(ps), _dev(fl), _dev(seg),
                                     _dev(llp), _dev(ws), ws.numel(), _stream()))
    return ps, fl, seg, llp


# ---- x-vector speaker head (lds_xvector_*): hidden states [B, T, d_in] contiguous fp32 device tensors, per-clip frame counts on the host ----
XVECTOR_K_STEP = 32       # every layer's input width is a multiple of it (a K-block of the TDNN GEMM may not span two taps)
XVECTOR_MAX_T = 32768


class XVectorCfg(C.Structure):
    _fields_ = [("d_in", C.c_int), ("n_tdnn", C.c_int), ("tdnn_dim", C.c_int * 8), ("tdnn_kernel", C.c_int * 8), ("tdnn_dilation", C.c_int * 8),
                ("xvector_dim", C.c_int)]


def xvector_check_layer(Cin, Cout, ks, dil, what="xvector"):
    """the limits of one TDNN / linear layer (include/lds.h), as ValueErrors before a device is touched"""
    if Cin < XVECTOR_K_STEP or Cin > 4096 or Cin % XVECTOR_K_STEP:
        raise ValueError(f"{what}: input width {Cin} must be a multiple of the K-step {XVECTOR_K_STEP} in {XVECTOR_K_STEP} .. 4096")
    if Cout < 4 or Cout > 4096 or Cout % 4:
        raise ValueError(f"{what}: output width {Cout} must be a multiple of 4 in 4 .. 4096")
    if not 1 <= ks <= 8 or not 1 <= dil <= 8:
        raise ValueError(f"{what}: kernel {ks} / dilation {dil} outside 1 .. 8")


class XVector(_Handle):
    """Handle on an x-vector head (lds_xvector_*).  d_in: the hidden width; tdnn_dim / tdnn_kernel / tdnn_dilation: HF's config keys;
    `state`: the head's tensors under their transformers names (projector.*, tdnn.{i}.kernel.*, feature_extractor.*, classifier.*)."""
    KIND = "xvector"

    def __init__(self, d_in, tdnn_dim, tdnn_kernel, tdnn_dilation, xvector_dim, state):
        dim, ker, dil = [int(v) for v in tdnn_dim], [int(v) for v in tdnn_kernel], [int(v) for v in tdnn_dilation]
        if not 1 <= len(dim) <= 8 or len(ker) != len(dim) or len(dil) != len(dim):
            raise ValueError(f"xvector: 1 .. 8 TDNN layers with one kernel and one dilation each (got {len(dim)}, {len(ker)}, {len(dil)})")
        xvector_check_layer(int(d_in), dim[0], 1, 1, "xvector projector")
        for i in range(len(dim)):
            xvector_check_layer(dim[i - 1] if i else dim[0], dim[i], ker[i], dil[i], f"xvector tdnn.{i}")
        if xvector_dim < 4 or xvector_dim > 4096 or xvector_dim % 4:
            raise ValueError(f"xvector: xvector_dim {xvector_dim} must be a multiple of 4 in 4 .. 4096")
        pad = [0] * (8 - len(dim))
        cfg = XVectorCfg(int(d_in), len(dim), (C.c_int * 8)(*dim, *pad), (C.c_int * 8)(*ker, *pad), (C.c_int * 8)(*dil, *pad), int(xvector_dim))
        self._create_weights(cfg, state)
        self.d_in, self.xvector_dim, self.span = int(d_in), int(xvector_dim), sum((k - 1) * d for k, d in zip(ker, dil))
        self.n_labels = lib().lds_xvector_n_labels(self.h)

    def embed(self, hidden, n_frames, return_logits=True, ws=None):
        """hidden [B, T, d_in], n_frames (host ints [B]; every clip needs span + 2 frames) -> (embeddings [B, xvector_dim], logits [B, n_labels] or None)"""
        import torch
        if hidden.dim() != 3 or hidden.shape[-1] != self.d_in:
            raise ValueError(f"xvector: hidden states {list(hidden.shape)} against a head over {self.d_in}-wide ones")
        B, T, _ = hidden.shape
        if not 1 <= T <= XVECTOR_MAX_T:
            raise ValueError(f"xvector: T {T} outside 1 .. {XVECTOR_MAX_T}")
        nf = _host_lengths(n_frames, B, 0, T, 64, "x-vector")
        if nf.min() < self.span + 2:
            raise ValueError(f"xvector: a clip of {int(nf.min())} frames leaves {max(int(nf.min()) - self.span, 0)} frames to pool; the unbiased standard "
                             f"deviation needs 2, i.e. at least {self.span + 2} frames")
        _dev(hidden, None)
        if ws is None:
            ws = self._workspace("lds_xvector_workspace_bytes", hidden.device, B, T)
        emb = torch.empty(B, self.xvector_dim, dtype=torch.float32, device=hidden.device)
        logits = torch.empty(B, self.n_labels, dtype=torch.float32, device=hidden.device) if return_logits else None
        check(lib().lds_xvector_embed(self.h, _dev(hidden, torch.float32), _host(nf), _dev(emb), _dev_or_null(logits), _dev(ws), ws.numel(), B, T, _stream()))
        return emb, logits


def xvector_cosine(a, b):
    """a [N, dim], b [M, dim] -> [N, M]: torch.nn.functional.cosine_similarity of every pair (include/lds.h lds_xvector_cosine)"""
    import torch
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or not a.shape[0] or not b.shape[0]:
        raise ValueError(f"xvector_cosine: {list(a.shape)} against {list(b.shape)} are not [N, dim] and [M, dim]")
    _dev(a, None)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    check(lib().lds_xvector_cosine(_dev(a, torch.float32), a.shape[0], _dev(b, torch.float32), b.shape[0], a.shape[1], _dev(out), _stream()))
    return out


def _xvector_layer_args(X, n_frames, W, bias, ks):
    B, T, Cin = X.shape
    Cout = W.shape[0]
    assert tuple(W.shape) == (Cout, ks * Cin) and tuple(bias.shape) == (Cout,)
    return B, T, Cin, Cout, _host_lengths(n_frames, B, 0, T, 64, "x-vector")


def xvector_test_tdnn(X, n_frames, W, bias, ks, dil, relu=True, out=None):
    """one layer (include/lds_test.h lds_test_xvector_tdnn) -> Y [B, T, Cout]; `out`: a preallocated Y (tests put guards behind it)"""
    import torch
    B, T, Cin, Cout, nf = _xvector_layer_args(X, n_frames, W, bias, ks)
    Y = torch.empty(B, T, Cout, dtype=torch.float32, device=X.device) if out is None else out
    check(lib().lds_test_xvector_tdnn(_dev(X, torch.float32), B, T, _host(nf), _dev(W, torch.float32), _dev(bias, torch.float32), Cin, Cout, int(ks), int(dil),
                                      1 if relu else 0, _dev(Y), _stream()))
    return Y


def xvector_test_pool(X, n_frames, W, bias, ks, dil, return_y=False, ws=None):
    """the last layer with the pooling in its epilogue (include/lds_test.h lds_test_xvector_pool) -> stats [B, 2 Cout][, the unfused Y]"""
    import torch
    B, T, Cin, Cout, nf = _xvector_layer_args(X, n_frames, W, bias, ks)
    if ws is None:
        ws = _ctc_ws.get(_bytes("lds_test_xvector_pool_workspace_bytes", B, T, Cout), X.device)
    stats = torch.empty(B, 2 * Cout, dtype=torch.float32, device=X.device)
    Y = torch.empty(B, T, Cout, dtype=torch.float32, device=X.device) if return_y else None
    check(lib().lds_test_xvector_pool(_dev(X, torch.float32), B, T, _host(nf), _dev(W, torch.float32), _dev(bias, torch.float32), Cin, Cout, int(ks), int(dil),
                                      _dev(stats), _dev_or_null(Y), _dev(ws), ws.numel(), _stream()))
    return (stats, Y) if return_y else stats


def resample_tables(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """the cached host tables of a parameter set (no device needed): dict with O, N, taps, bankT fp32 [taps, N], first int32 [N]"""
    key = (orig_freq, new_freq, lowpass_filter_width, float(rolloff))      # (arch.resample_bank refuses what is not an integer)
    t = _resample_tables.get(key)
    if t is None:
        from . import arch
        O, N, taps, bankT, first = arch.resample_bank(*key)
        t = _resample_tables[key] = dict(O=O, N=N, taps=taps, bankT=bankT, first=first, dev={})
    return t


def resample_out_length(length, O, N):
    return -((-int(length) * N) // O)


def resample(x, tables, lengths=None):
    """x [B, L] fp32 on the device, tables from resample_tables -> y [B, M] (include/lds.h lds_resample); with lengths (host ints [B], at most
    64 clips, 0 .. L): every clip resampled as if alone, zeros beyond its own ceil(N len / O) samples; returns (y [B, Mmax], new lengths
    int64 [B] on the host) (lds_resample_ragged)"""
    import torch
    if not x.is_cuda:
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    B, L = x.shape
    O, N = tables["O"], tables["N"]
    dev = tables["dev"].get(str(x.device))
    if dev is None:
        dev = tables["dev"][str(x.device)] = (torch.from_numpy(tables["bankT"]).to(x.device), torch.from_numpy(tables["first"]).to(x.device))
    ln = None if lengths is None else _host_lengths(lengths, B, 0, L, max_B=64, what="resampler")
    M = resample_out_length(L if ln is None else max(int(ln.max()), 1), O, N)
    y = torch.empty((B, M), dtype=torch.float32, device=x.device)
    tail = (_dev(dev[0], torch.float32), _dev(dev[1], torch.int32), O, N, tables["taps"], B, L, M, _stream())
    if ln is None:
        check(lib().lds_resample(_dev(x, torch.float32), _dev(y), *tail))
        return y
    new = np.zeros(B, dtype=np.int64)
    check(lib().lds_resample_ragged(_dev(x, torch.float32), _host(ln), _dev(y), _host(new), *tail))
    return y, torch.from_numpy(new)


# ---- long-audio conversion (lds_frame_rms, lds_volume_*, lds_resample_frames_ragged, lds_overlap_assemble; csrc/svc.hip) ----
def _wave_1d(x, what):
    import torch
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{what} needs the audio as a tensor on a HIP device (no CPU fallback)")
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError(f"{what}: a mono 1-D waveform with at least one sample is needed, got shape {list(x.shape)}")
    return x.float().contiguous()


def frame_rms_length(L, frame_length, hop_length):
    return 1 + (int(L) + 2 * (frame_length // 2) - frame_length) // hop_length


def frame_rms(x, frame_length, hop_length, pad_mode="constant"):
    """x [L] on the device -> librosa.feature.rms(y=x, frame_length, hop_length) [n] on the device; pad_mode 'constant' (zeros) or 'reflect' """
    import torch
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"frame_rms: pad_mode {pad_mode!r} ('constant' or 'reflect')")
    x = _wave_1d(x, "frame_rms")
    n = frame_rms_length(x.numel(), frame_length, hop_length)
    out = torch.empty(max(n, 0), dtype=torch.float32, device=x.device)
    check(lib().lds_frame_rms(_dev(x, torch.float32), _dev(out), x.numel(), int(frame_length), int(hop_length), int(pad_mode == "reflect"), n, _stream()))
    return out


def volume_extract(x, hop):
    """x [L] on the device -> Volume_Extractor.extract's volume [int(L // hop) + 1] on the device; hop: a float, possibly fractional"""
    import torch
    x = _wave_1d(x, "volume_extract")
    hop = float(hop)
    if not hop >= 1.0:
        raise ValueError(f"volume_extract: hop {hop} must be at least 1")
    n = int(x.numel() // hop) + 1
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    h = C.c_double(hop)
    check(lib().lds_volume_extract(_dev(x, torch.float32), _dev(out), x.numel(), C.addressof(h), n, _stream()))
    return out


def volume_mask(volume, factor, threshold):
    """volume [n] on the device -> the dilated, linearly up-sampled mask [n * factor]; threshold: the linear amplitude, rounded to fp32"""
    import torch
    if not torch.is_tensor(volume) or not volume.is_cuda:
        raise RuntimeError("volume_mask needs the volume as a tensor on a HIP device (no CPU fallback)")
    v = volume.reshape(-1).float().contiguous()
    out = torch.empty(v.numel() * int(factor), dtype=torch.float32, device=v.device)
    check(lib().lds_volume_mask(_dev(v, torch.float32), _dev(out), v.numel(), int(factor), float(np.float32(threshold)), _stream()))
    return out


def resample_frames_ragged(x, tin, tout):
    """x [B, Tin, C], every clip's own frame counts in (1 .. Tin) and out (host ints) -> [B, max(tout), C]: clip b's first tin[b] rows
    aligned to tout[b] rows by 'nearest' as resample_frames does alone, zeros beyond"""
    import torch
    B, T, Cc = x.shape
    ti = _host_lengths(tin, B, 1, T, max_B=64, what="frame alignment")
    to = _host_lengths(tout, B, 0, 2 ** 31 - 1)
    n_out = max(int(to.max()), 1)
    out = torch.empty(B, n_out, Cc, dtype=torch.float32, device=x.device)
    check(lib().lds_resample_frames_ragged(_dev(x, torch.float32), _host(ti), _host(to), _dev(out), B, T, n_out, Cc, _stream()))
    return out


def overlap_table(offset, start, length):
    """the three per-segment arrays -> host int64 [3, S] (offset, start, len), as lds_overlap_assemble reads them"""
    tab = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.int64).reshape(-1) for a in (offset, start, length)]))
    if tab.shape[1] < 1:
        raise ValueError("overlap_assemble: no segment")
    return tab


def overlap_assemble(segs, offset, start, length, mask=None):
    """segs [n] on the device: the segments packed; offset / start / length: host ints per segment; mask [>= N] on the device or None ->
    the joined waveform [N], N = start[-1] + length[-1] (include/lds.h lds_overlap_assemble).  The library checks the preconditions on the
    host table before anything is enqueued; its LDS_EINVAL, which names the segment, is raised as ValueError.  The table is uploaded once."""
    import torch
    tab = overlap_table(offset, start, length)
    S = tab.shape[1]
    N = int(tab[1, -1] + tab[2, -1])
    if not torch.is_tensor(segs) or not segs.is_cuda or (mask is not None and not mask.is_cuda):
        raise RuntimeError("liblds needs tensors on a HIP device (no CPU fallback for the hot path)")
    m = None if mask is None else mask.reshape(-1)
    dtab = torch.from_numpy(tab).to(segs.device)
    out = torch.empty(min(max(N, 0), 1 << 33), dtype=torch.float32, device=segs.device)      # (a table that gives another N is refused below)
    rc = lib().lds_overlap_assemble(_dev(segs, torch.float32) if segs.numel() else None, segs.numel(), _host(tab), _dev(dtab, torch.int64), S,
                                    _dev_or_null(m, torch.float32), 0 if m is None else m.numel(), _dev(out) if N > 0 else None, N, _stream())
    if rc == -1:      # LDS_EINVAL: a precondition on the table, the mask or the buffer
        raise ValueError(lib().lds_last_error().decode())
    check(rc)
    return out
