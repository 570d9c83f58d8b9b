"""The pieces of reference tools/tools.py that are built: the encoder-width table, `units_forced_alignment` (and its per-clip form
`units_forced_alignment_ragged`), the units encoders (`Units_Encoder` over `WhisperLargeV3`, reference tools/tools.py:43-126, or over
`HubertUnits`: the reference's encoder/hubert/model.py as 'hubertsoft' / 'contentvec768l12', or over `Audio2xlsr_53_56k`: wav2vec 2.0 XLSR-53,
or over `Wav2Vec2Bert`: w2v-BERT 2.0, or over `WavLMUnits`: WavLM as 'wavlmbase+' / 'wavlmlarge'),
`Volume_Extractor`, `upsample` and `cross_fade` (tools/tools.py:12-41, 225-238) and `Resample`, the torchaudio transform that file imports
(tools/tools.py:9).  'w2v-bert' downloaded from the hub and 'xlsr_53_56k' loaded through fairseq (the reference's defaults) and the schedulers
there are not built."""
import math

import numpy as np
import torch

from encoder.hubert.model import HubertSoft
from encoder.wav2vec2.model import Wav2Vec2, load_checkpoint_state
from encoder.wav2vec2_bert.model import Wav2Vec2BertModel, load_checkpoint_state as load_w2vbert_checkpoint_state
from encoder.wavlm.model import WavLM
from encoder.whisper.model import ModelDimensions, Whisper
from lds import arch, native
from lds.arch import get_encoder_out_channels


def get_encdoer_out_channels(encoder):  # sic: the reference's spelling (tools/tools.py:257-264)
    return get_encoder_out_channels(encoder)


def units_forced_alignment(units, audio=None, sample_rate=None, hop_size=None, n_frames=None, scale_factor=None,
                           units_forced_mode="nearest", device="cpu"):
    """Resample unit frames [B,T,C] (or [T,C]) along time (reference tools/tools.py:193-223).  'nearest' (and the two 'rfa*'
    aliases) = F.interpolate(mode='nearest'): out[i] = units[min(floor(i * s), T-1)] with s = 1/scale_factor (or T/n_frames
    when the size is given) in fp32; 'left' = units[min(round(scale_factor * i), T-1)].  The frame gather runs in liblds, so
    the units must live on a HIP device (22_infer_tts.py:108-110 passes the device tensor).  Other interpolate modes are not
    used by the TTS path."""
    assert (audio is not None and sample_rate is not None and hop_size is not None) or n_frames is not None or scale_factor is not None
    n_frames = int(audio.size(-1) // hop_size + 1) if (n_frames is None and audio is not None) else n_frames
    if isinstance(units, np.ndarray) or not units.is_cuda:
        raise RuntimeError("units_forced_alignment needs the units on a HIP device (no CPU fallback for the hot path)")
    squeeze = units.dim() == 2
    u = (units.unsqueeze(0) if squeeze else units).contiguous().float()
    T = u.shape[1]
    if units_forced_mode == "left":
        assert scale_factor is not None and n_frames is not None
        idx = torch.clamp(torch.round(scale_factor * torch.arange(n_frames, device=u.device)).long(), max=T - 1)
        out = native.gather_rows(u.reshape(-1, u.shape[-1]), (idx[None, :] + T * torch.arange(u.shape[0], device=u.device)[:, None]))
    elif units_forced_mode in ("nearest", "rfa441to512", "rfa512to441"):
        if n_frames is not None and scale_factor is not None:
            raise ValueError("only one of size or scale_factor should be defined")      # F.interpolate's own check
        if n_frames is not None:
            n_out, step = int(n_frames), np.float32(T) / np.float32(n_frames)
        else:
            n_out, step = int(math.floor(float(T) * float(scale_factor))), np.float32(1.0 / float(scale_factor))
        out = native.resample_frames(u, n_out, float(step))
    else:
        raise NotImplementedError(f"units_forced_mode {units_forced_mode!r} is not used on the TTS path")
    return out.squeeze(0) if squeeze else out


def units_forced_alignment_ragged(units, unit_lengths, n_frames):
    """Extension (not in the reference): units_forced_alignment(units[b, :unit_lengths[b]], n_frames=n_frames[b]) in 'nearest' mode for
    every clip of a padded batch [B, T, C] at once (host ints, at most 64 clips) -> [B, max(n_frames), C], each clip bit for bit as if
    aligned alone, zeros beyond its n_frames[b]; rows at and beyond unit_lengths[b] are never read (lds_resample_frames_ragged)"""
    if isinstance(units, np.ndarray) or not units.is_cuda:
        raise RuntimeError("units_forced_alignment_ragged needs the units on a HIP device (no CPU fallback for the hot path)")
    return native.resample_frames_ragged(units.contiguous().float(), unit_lengths, n_frames)


def _device_wave(name, audio, device="cuda"):
    """numpy is moved to the device; a tensor must be there already"""
    if isinstance(audio, np.ndarray):
        audio = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(device)
    if not torch.is_tensor(audio) or not audio.is_cuda:
        raise RuntimeError(f"{name} needs a numpy array or a tensor on a HIP device (no CPU fallback)")
    return audio


class Volume_Extractor:
    """reference tools/tools.py:12-41.  `extract` returns the volume fp32 [n] on the device (the reference: float64 numpy), computed by
    lds_volume_extract; `get_mask_from_volume` thresholds, dilates and up-samples it in one kernel (lds_volume_mask)."""

    def __init__(self, hop_size=512, block_size=None, model_sampling_rate=None):
        """hop_size alone: frames of that many samples.  block_size together with model_sampling_rate: the hop follows the rate of the
        audio that `extract` is given, block_size * sr / model_sampling_rate (one without the other is an AssertionError)"""
        given = [v is not None for v in (block_size, model_sampling_rate)]
        assert all(given) or not any(given)
        self.hop_size, self.block_size, self.model_sampling_rate = hop_size, block_size, model_sampling_rate
        self.hop_size_follow_input = all(given)

    def extract(self, audio, sr=None, device="cuda"):
        """`device` (not in the reference): where a numpy `audio` is moved to"""
        if sr is not None:
            assert self.hop_size_follow_input
            self.hop_size = self.block_size * sr / self.model_sampling_rate
        return native.volume_extract(_device_wave("Volume_Extractor.extract", audio, device), self.hop_size)

    def get_mask_from_volume(self, volume, threhold=-60.0, device='cpu'):
        """volume [n] -> mask [1, n * block_size] on the device the volume lives on (`device` is the reference's parameter: the mask of a
        device volume cannot be anywhere else; a numpy volume goes to `device`, which must be a HIP device)"""
        volume = _device_wave("Volume_Extractor.get_mask_from_volume", volume, device)
        return native.volume_mask(volume, self.block_size, 10 ** (float(threhold) / 20)).unsqueeze(0)


def upsample(signal, factor):
    """reference tools/tools.py:225-229: signal [B, n, C] -> [B, n * factor, C], linear interpolation with the last frame repeated:
    out[j] = s[i] (1 - f) + s[min(i + 1, n - 1)] f, i = j // factor, f = (j % factor) / factor.  The long-audio path does not come here
    (lds_volume_mask holds the same formula); this is the reference's helper for other callers, a gather and a lerp on the signal's device."""
    n = signal.shape[1]
    j = torch.arange(n * factor, device=signal.device)
    i = j // factor
    f = ((j % factor).float() / factor)[None, :, None]
    return signal[:, i] * (1 - f) + signal[:, torch.clamp(i + 1, max=n - 1)] * f


def cross_fade(a, b, idx):
    """reference tools/tools.py:231-238: `a` up to idx, a linear fade from a to b over a's remaining len(a) - idx samples, then the rest of
    b -> [idx + len(b)] on the device = lds_overlap_assemble with two segments and no mask (0 <= len(a) - idx <= len(b))"""
    a, b = _device_wave("cross_fade", a).reshape(-1).float(), _device_wave("cross_fade", b).reshape(-1).float()
    return native.overlap_assemble(torch.cat([a, b]), [0, a.numel()], [0, int(idx)], [a.numel(), b.numel()])


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample with its positional parameters and defaults (the reference imports it at tools/tools.py:9 and
    diffusion/vocoder.py:3): waveform [..., L] on a HIP device -> [..., ceil(new L / orig)], the polyphase kernel of lds_resample
    (include/lds.h).  orig_freq == new_freq returns the input itself.  Built: "sinc_interp_hann" with any integer
    lowpass_filter_width >= 1 and 0 < rolloff <= 1; "sinc_interp_kaiser" raises NotImplementedError; CPU tensors raise (no CPU
    fallback).  The filter is built once per parameter set on the host in float64 and uploaded once per device, so `.to(device)` has
    nothing to move."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99):
        super().__init__()
        if resampling_method == "sinc_interp_kaiser":
            raise NotImplementedError("Resample: the Kaiser window (sinc_interp_kaiser) is not built; sinc_interp_hann is")
        if resampling_method != "sinc_interp_hann":
            raise ValueError(f"Invalid resampling method: {resampling_method}")
        self.orig_freq, self.new_freq = orig_freq, new_freq
        self.resampling_method, self.lowpass_filter_width, self.rolloff = resampling_method, lowpass_filter_width, rolloff
        self.tables = None if orig_freq == new_freq else native.resample_tables(orig_freq, new_freq, lowpass_filter_width, rolloff)

    def _check(self, name, waveform):
        if not torch.is_tensor(waveform) or not waveform.is_cuda:
            raise RuntimeError(f"{name} needs the waveform as a tensor on a HIP device (no CPU fallback)")

    @torch.inference_mode()
    def forward(self, waveform):
        if self.tables is None:
            return waveform
        self._check("Resample.forward", waveform)
        x = waveform.reshape(-1, waveform.shape[-1]).float().contiguous()
        y = torch.cat([native.resample(x[r:r + 65535], self.tables) for r in range(0, x.shape[0], 65535)])      # (the entry's batch limit)
        return y.reshape(*waveform.shape[:-1], y.shape[-1])

    @torch.inference_mode()
    def forward_ragged(self, waveform, lengths):
        """Extension (not in the reference): waveform [B, L] padded to the longest clip + every clip's own sample count (host ints, at
        most 64 clips, 0 .. L) -> (out [B, Mmax], new_lengths int64 [B] on the host): every clip resampled as if alone, whatever lies
        beyond its length (NaN included); new_lengths[b] = ceil(new lengths[b] / orig), zeros beyond; Mmax = the largest of them"""
        if self.tables is None:
            ln = native._host_lengths(lengths, waveform.shape[0], 0, waveform.shape[1], max_B=64, what="resampler")
            return waveform, torch.from_numpy(ln.astype(np.int64))
        self._check("Resample.forward_ragged", waveform)
        return native.resample(waveform.float().contiguous(), self.tables, lengths)


class Units_Encoder:
    """Speech -> units (reference tools/tools.py:43-103).  Built: encoder 'whisper_large_v3' in the 'nearest' / 'left' modes, and the
    HuBERT stack (HubertUnits below) as 'hubertsoft' (256-wide soft units) and 'contentvec768l12' (its 768-wide last layer), and
    'xlsr_53_56k' (Audio2xlsr_53_56k below: wav2vec 2.0 XLSR-53, 1024-wide) and 'w2v-bert' (Wav2Vec2Bert below: w2v-BERT 2.0, 1024-wide),
    and 'wavlmbase+' / 'wavlmlarge' (WavLMUnits below: WavLM-Base+ 768-wide, WavLM-Large 1024-wide; `units_layer=` picks the hidden state,
    default the last), each with `model=` or `checkpoint=`.  Frame counts and the shortest clip come from the model (`frames_of`, `min_samples`):
    (L // 160 - 1) // 2 + 1 and 400 samples for Whisper, L // 320 and 320 for HuBERT, the unpadded level rule (400 samples -> 1 frame) and
    400 for XLSR-53, ceil((1 + (L - 400) // 160) / 2) rows and 560 for w2v-BERT (whose last row is the reference's masked row when the
    frame count is odd: Wav2Vec2Bert's docstring).
    Deviations from the reference, each raising instead of guessing:
      - resampling is opt-in: by default `sample_rate` must equal `encoder_sample_rate` (ValueError naming both), where the reference
        resamples with torchaudio; with `resample=True` (keyword-only, not in the reference) a mismatched rate goes through
        `self.resample_kernel[str(sample_rate)]`, a `Resample(sample_rate, encoder_sample_rate)` made on first use as the reference
        makes it (tools/tools.py:81-84), in encode, encode_ragged and the encode_tokens* forms;
      - the units stay on the device (the reference moves them to the CPU); CPU tensors raise, there is no CPU fallback;
      - 'w2v-bert' with neither `model=` nor `checkpoint=` is the reference's transformers hub download: NotImplementedError;
        'xlsr_53_56k' with neither is the reference's fairseq load of pretrain/xlsr_53_56k.pt: NotImplementedError;
        'wavlmbase+' / 'wavlmlarge' with neither would be a hub download too: NotImplementedError; the 'rfa441to512' / 'rfa512to441' modes
        need librosa's resampler: NotImplementedError.
    `model` (not in the reference): a ready WhisperLargeV3 / HubertUnits / Audio2xlsr_53_56k / Wav2Vec2Bert, e.g.
    WhisperLargeV3.synthetic(...), instead of the checkpoint; `checkpoint` (keyword-only, not in the reference): the file a HuBERT, XLSR-53
    or w2v-BERT encoder loads its state dict from."""

    def __init__(self, encoder, encoder_sample_rate=16000, encoder_hop_size=320, device=None, units_forced_mode='nearest', *, model=None, resample=False, checkpoint=None,
                 units_layer=None):
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.device = device
        self.encoder = encoder
        if units_forced_mode is None:
            units_forced_mode = 'left'
        self.units_forced_mode = units_forced_mode
        if encoder == 'w2v-bert' and model is None and checkpoint is None:
            raise NotImplementedError("Units_Encoder: 'w2v-bert' by default downloads transformers' from_pretrained('facebook/w2v-bert-2.0'), which is "
                                      "not built; pass checkpoint=PATH (the state dict in transformers naming, torch-saved or .safetensors) or model=")
        if encoder == 'xlsr_53_56k' and model is None and checkpoint is None:
            raise NotImplementedError("Units_Encoder: 'xlsr_53_56k' by default loads pretrain/xlsr_53_56k.pt through fairseq, which is not built; "
                                      "pass checkpoint=PATH (a state dict of plain tensors, fairseq or transformers naming) or model=")
        if encoder in WavLMUnits.NAMES and model is None and checkpoint is None:
            raise NotImplementedError(f"Units_Encoder: {encoder!r} without local weights would be a hub download (microsoft/wavlm-*), which is not "
                                      "built; pass checkpoint=PATH (the state dict in transformers naming, torch-saved or .safetensors) or model=")
        if units_layer is not None and encoder not in WavLMUnits.NAMES:
            raise ValueError(f"Units_Encoder: units_layer= belongs to {WavLMUnits.NAMES}, not to {encoder!r}")
        if encoder not in ('whisper_large_v3', 'xlsr_53_56k', 'w2v-bert') + HubertUnits.NAMES + WavLMUnits.NAMES:
            raise ValueError(f"[x] Unknown units encoder: {encoder}")
        if units_forced_mode in ('rfa441to512', 'rfa512to441'):
            raise NotImplementedError(f"units_forced_mode {units_forced_mode!r} resamples with librosa; not built")
        if model is not None:
            self.model = model
            if units_layer is not None:
                self.model.set_units_layer(units_layer)
        elif encoder in WavLMUnits.NAMES:
            self.model = WavLMUnits(encoder, device=device, checkpoint=checkpoint, units_layer=units_layer)
        elif encoder in HubertUnits.NAMES:
            if checkpoint is None:
                raise ValueError(f"Units_Encoder: {encoder!r} needs checkpoint=PATH (a local state dict; nothing is downloaded) or model=")
            self.model = HubertUnits(encoder, device=device, checkpoint=checkpoint)
        elif encoder == 'xlsr_53_56k':
            self.model = Audio2xlsr_53_56k(device=device, checkpoint=checkpoint)
        elif encoder == 'w2v-bert':
            self.model = Wav2Vec2Bert(device=device, checkpoint=checkpoint)
        else:
            self.model = WhisperLargeV3(device=device)
        self.min_samples = getattr(self.model, "min_samples", 400)
        self.resample_kernel = {}
        self.resample = bool(resample)
        self.encoder_sample_rate = encoder_sample_rate
        self.encoder_hop_size = encoder_hop_size

    def _check(self, name, audio, sample_rate):
        """the resampler for this rate (None: the audio is at the encoder's rate already), after the checks of every entry"""
        if sample_rate != self.encoder_sample_rate and not self.resample:
            raise ValueError(f"{name}: audio at {sample_rate} Hz, the encoder runs at {self.encoder_sample_rate} Hz; "
                             "resample the audio first, or pass resample=True / use tools.tools.Resample")
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise RuntimeError(f"{name} needs the audio as a tensor on a HIP device (no CPU fallback)")
        if sample_rate == self.encoder_sample_rate:
            return None
        key_str = str(sample_rate)
        if key_str not in self.resample_kernel:
            self.resample_kernel[key_str] = Resample(sample_rate, self.encoder_sample_rate).to(self.device)
        return self.resample_kernel[key_str]

    def encode(self, audio, sample_rate, padding_mask=None):
        """audio [L] or [1, L] -> units [T, C] on the device (reference tools/tools.py:76-103; padding_mask is ignored as
        WhisperLargeV3.__call__ ignores it); a clip shorter than 400 samples (the model's `min_samples`: 560 with w2v-BERT) is zero-padded to
        that length as the reference pads to 400"""
        rs = self._check("Units_Encoder.encode", audio, sample_rate)
        if rs is not None:
            audio = rs(audio)
        if audio.size(-1) < self.min_samples:
            audio = torch.nn.functional.pad(audio, (0, self.min_samples - audio.size(-1)))
        units = self.model(audio, padding_mask=padding_mask)
        if units.dim() == 3 and units.shape[0] == 1:
            units = units.squeeze(0)
        return units

    def encode_ragged(self, audio, lengths, sample_rate=None, *, pad_short=False):
        """Extension (not in the reference): audio [B, L] padded to the longest clip + every clip's own sample count (host ints, at most 64
        clips) -> (units [B, Tmax, C], n_frames [B] int64 on the host): every clip encoded as if alone, rows beyond its own
        n_frames[b] = (lengths[b] // 160 - 1) // 2 + 1 are zeros.  400 <= lengths[b] <= L (ValueError otherwise: pad a shorter clip with
        zeros to 400 samples first, as encode does).  With resample=True and another `sample_rate`, audio and lengths are at that rate:
        the batch is resampled by Resample.forward_ragged first, and the limits apply to the resampled lengths (a batch whose longest
        resampled clip is below 400 samples is zero-padded to 400 columns).  pad_short=True does encode's padding here: a clip that has
        fewer than 400 samples at the encoder's rate (after resampling, if any) is continued with zeros to 400, whatever the buffer held
        there."""
        rs = self._check("Units_Encoder.encode_ragged", audio, self.encoder_sample_rate if sample_rate is None else sample_rate)
        if rs is not None:
            audio, lengths = rs.forward_ragged(audio, lengths)
        lo = self.min_samples      # (400 with Whisper and XLSR-53; 320 with a HuBERT encoder; 560 with w2v-BERT)
        if (rs is not None or pad_short) and audio.size(-1) < lo:
            audio = torch.nn.functional.pad(audio, (0, lo - audio.size(-1)))
        if pad_short:
            ln = native._host_lengths(lengths, audio.shape[0], 0, audio.shape[1], max_B=64, what="units")
            if (ln < lo).any():
                if rs is None:      # (the resampler has written zeros beyond every clip already)
                    audio = audio.clone()
                    for b in np.nonzero(ln < lo)[0]:
                        audio[b, int(ln[b]):lo] = 0
                lengths = np.maximum(ln, lo)
        return self.model.encode_ragged(audio, lengths)

    def encode_tokens(self, audio, sample_rate, codebook, metric="l2"):
        """Extension: audio -> semantic tokens int64 [T] on the device = encode, then the nearest centre of `codebook` (a model from
        cluster.get_cluster_model) by lds_kmeans_assign, without leaving the device (the reference's steps 16 + 19 go through .npy files);
        metric="cosine": the centre of highest cosine similarity (a codebook fitted by train_cluster(mode="cosine"))"""
        import cluster
        from lds.native import metric_code
        metric_code(metric)      # (a bad metric fails before the encoder runs)
        return cluster.get_cluster_result(codebook, self.encode(audio, sample_rate), metric=metric)

    def encode_tokens_ragged(self, audio, lengths, codebook, pad_id, sample_rate=None, metric="l2"):
        """Extension: encode_ragged + tokens [B, Tmax] int64: rows at and beyond a clip's own n_frames[b] hold pad_id; returns (tokens, n_frames)"""
        import cluster
        from lds.native import metric_code
        metric_code(metric)
        units, n_frames = self.encode_ragged(audio, lengths, sample_rate)
        return cluster.get_cluster_result(codebook, units, lengths=n_frames, pad_id=pad_id, metric=metric), n_frames


class HubertUnits(torch.nn.Module):
    """The HuBERT stack (encoder.hubert.model.HubertSoft) in the role WhisperLargeV3 plays for Units_Encoder.  `name`: 'hubertsoft' -> the
    256-wide soft units (HubertSoft.units: proj of the last layer), 'contentvec768l12' -> the 768-wide output of the last layer of the same
    stack, both of the waveform padded by 40 zeros per side, L // 320 frames.  `checkpoint`: a torch-saved state dict with the keys of the
    reference's HubertSoft (optionally under "model_state_dict", an optional "module." prefix removed); a ContentVec checkpoint in fairseq's
    key naming is NOT handled (rename its keys first).  `dims` + `state` (keyword-only) inject the weights directly."""
    NAMES = ('hubertsoft', 'contentvec768l12')
    min_samples = arch.HUBERT_MIN_SAMPLES
    family = "HuBERT"

    def __init__(self, name='hubertsoft', device='cuda', checkpoint=None, *, dims=None, state=None):
        super().__init__()
        if name not in self.NAMES:
            raise ValueError(f"[x] Unknown units encoder: {name}")
        self.name, self.device, self.proj = name, device, name == 'hubertsoft'
        if state is None:
            if checkpoint is None:
                raise ValueError(f"HubertUnits: {name!r} needs checkpoint=PATH or dims= / state= (nothing is downloaded)")
            print(name)
            state = torch.load(checkpoint, map_location="cpu", weights_only=False)
            state = state.get("model_state_dict", state)
            state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
        model = HubertSoft(dims=dims)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=True)
        self.model = model.eval()
        self.hidden_dim = model.dims["n_proj" if self.proj else "n_state"]
        self.n_ctx = model.dims["n_ctx"]      # the window of one call, in frames

    @classmethod
    def synthetic(cls, name='hubertsoft', dims=None, seed=0, device='cuda'):
        """seeded weights (lds.arch.hubert_init_state) for `dims` (default: HuBERT-base) -- no checkpoint ships"""
        dims = dict(arch.HUBERT_BASE_DIMS if dims is None else dims)
        return cls(name, device=device, dims=dims, state=arch.hubert_init_state(dims, seed))

    @staticmethod
    def frames_of(n_samples):
        return arch.hubert_frames(n_samples)

    @torch.inference_mode()
    def __call__(self, audio, padding_mask=None):
        """audio (any shape, flattened into ONE clip) -> units [T, C] on the device; padding_mask is ignored as WhisperLargeV3 ignores it"""
        if not audio.is_cuda:
            raise RuntimeError("HubertUnits needs the audio on a HIP device (no CPU fallback)")
        return self.model.native().encode(audio.reshape(1, -1).float().contiguous(), proj=self.proj).squeeze(0)

    @torch.inference_mode()
    def encode_ragged(self, audio, lengths):
        return self.model.units_ragged(audio, lengths, proj=self.proj)


class Audio2xlsr_53_56k(torch.nn.Module):
    """reference tools/tools.py Audio2xlsr_53_56k: wav2vec 2.0 XLSR-53, units = extract_features(audio, padding_mask=all False)["x"],
    1024 wide, the waveform taken as it is.  The reference loads `path` through fairseq; here `checkpoint` is a local file holding the
    state dict as plain tensors (bare or under "model"; fairseq or transformers naming, encoder.wav2vec2.model.load_checkpoint_state), or
    `dims` + `state` (keyword-only) inject the weights directly.  Nothing is downloaded."""
    min_samples = arch.W2V_MIN_SAMPLES
    family = "wav2vec 2.0"

    def __init__(self, path='pretrain/xlsr_53_56k.pt', device='cuda', *, checkpoint=None, dims=None, state=None):
        super().__init__()
        self.device = device
        if state is None:
            print('xlsr_53_56k')
            state = load_checkpoint_state(path if checkpoint is None else checkpoint)
        model = Wav2Vec2(dims)
        model.load_state_dict(state)
        self.model = model.eval()
        self.hidden_dim = model.dims["n_state"]
        self.n_ctx = model.dims["n_ctx"]      # the window of one call, in frames

    @classmethod
    def synthetic(cls, dims=None, seed=0, device='cuda'):
        """seeded weights (lds.arch.w2v_init_state) for `dims` (default: XLSR-53's) -- no checkpoint ships"""
        dims = dict(arch.XLSR_53_DIMS if dims is None else dims)
        return cls(device=device, dims=dims, state=arch.w2v_init_state(dims, seed))

    @staticmethod
    def frames_of(n_samples):
        return arch.w2v_frames(n_samples)

    @torch.inference_mode()
    def __call__(self, audio, padding_mask=None):
        """audio (any shape, flattened into ONE clip) -> units [T, C] on the device; padding_mask is ignored (the reference builds an
        all-False one itself)"""
        if not audio.is_cuda:
            raise RuntimeError("Audio2xlsr_53_56k needs the audio on a HIP device (no CPU fallback)")
        return self.model.native().encode(audio.reshape(1, -1).float().contiguous()).squeeze(0)

    @torch.inference_mode()
    def encode_ragged(self, audio, lengths):
        if audio.dim() != 2:
            raise ValueError(f"Audio2xlsr_53_56k.encode_ragged: audio must be [B, L], got {list(audio.shape)}")
        B, L = audio.shape
        ln = native.Wav2Vec2.lengths(lengths, B, L)      # (host-side validation first: a bad length is a ValueError on any device)
        if not audio.is_cuda:
            raise RuntimeError("Audio2xlsr_53_56k.encode_ragged needs the audio on a HIP device (no CPU fallback)")
        units = self.model.native().encode(audio.float().contiguous(), ln)
        return units, torch.from_numpy(np.array([self.frames_of(int(n)) for n in ln], dtype=np.int64))


class Wav2Vec2Bert(torch.nn.Module):
    """reference tools/tools.py Wav2Vec2Bert: w2v-BERT 2.0, units = Wav2Vec2BertModel(**SeamlessM4TFeatureExtractor(audio,
    sampling_rate=16000)).last_hidden_state, 1024 wide.  The reference downloads both from the hub; here `checkpoint` is a local file holding
    the model's state dict in transformers naming (torch-saved plain tensors, or .safetensors;
    encoder.wav2vec2_bert.model.load_checkpoint_state), or `dims` + `state` (keyword-only) inject the weights directly, and the feature
    extractor is the native filter bank (it has no weights).  Nothing is downloaded.
    A clip of n = 1 + (L - 400) // 160 frames gives (n + 1) // 2 rows.  With n odd the last of them is the MASKED ROW: the extractor pads the
    frames to an even count, the model masks the padded row as an attention key and zeroes it behind the feature projection and in front of
    the convolution module, but still returns it -- and so does this class.  A caller who does not want it drops row n // 2 when n is odd."""
    min_samples = arch.W2VBERT_MIN_SAMPLES
    family = "w2v-BERT"

    def __init__(self, device='cuda', *, checkpoint=None, dims=None, state=None):
        super().__init__()
        self.device = device
        if state is None:
            if checkpoint is None:
                raise NotImplementedError("Wav2Vec2Bert: the reference downloads transformers' from_pretrained('facebook/w2v-bert-2.0'), which is "
                                          "not built; pass checkpoint=PATH or dims= / state=")
            print('w2v-bert')
            state = load_w2vbert_checkpoint_state(checkpoint)
        model = Wav2Vec2BertModel(dims)
        model.load_state_dict(state)
        self.model = model.eval()
        self.hidden_dim = model.dims["n_state"]
        self.n_ctx = model.dims["n_ctx"]      # the window of one call, in rows

    @classmethod
    def synthetic(cls, dims=None, seed=0, device='cuda'):
        """seeded weights (lds.arch.w2vbert_init_state) for `dims` (default: w2v-BERT 2.0's) -- no checkpoint ships"""
        dims = dict(arch.W2V_BERT_DIMS if dims is None else dims)
        return cls(device=device, dims=dims, state=arch.w2vbert_init_state(dims, seed))

    @staticmethod
    def frames_of(n_samples):
        """rows of a clip, the masked row of an odd frame count included"""
        return arch.w2vbert_frames(n_samples)[2]

    @torch.inference_mode()
    def __call__(self, audio, padding_mask=None):
        """audio (any shape, flattened into ONE clip) -> units [rows, C] on the device; padding_mask is ignored (the reference ignores it)"""
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise RuntimeError("Wav2Vec2Bert needs the audio as a tensor on a HIP device (no CPU fallback)")
        return self.model.native().encode(audio.reshape(1, -1).float().contiguous()).squeeze(0)

    @torch.inference_mode()
    def encode_ragged(self, audio, lengths):
        if audio.dim() != 2:
            raise ValueError(f"Wav2Vec2Bert.encode_ragged: audio must be [B, L], got {list(audio.shape)}")
        B, L = audio.shape
        ln = native.Wav2Vec2Bert.lengths(lengths, B, L)      # (host-side validation first: a bad length is a ValueError on any device)
        if not audio.is_cuda:
            raise RuntimeError("Wav2Vec2Bert.encode_ragged needs the audio on a HIP device (no CPU fallback)")
        units = self.model.native().encode(audio.float().contiguous(), ln)
        return units, torch.from_numpy(np.array([self.frames_of(int(n)) for n in ln], dtype=np.int64))


class WavLMUnits(torch.nn.Module):
    """WavLM (encoder.wavlm.model.WavLM) in the role WhisperLargeV3 plays for Units_Encoder.  `name`: 'wavlmbase+' -> WavLM-Base+ (768 wide,
    the waveform as it is: so-vits-svc's encoder), 'wavlmlarge' -> WavLM-Large (1024 wide, every clip normalised to zero mean and unit
    variance first, as its feature extractor does: kNN-VC's encoder).  units = hidden_states[units_layer], default the last layer (kNN-VC:
    units_layer=6).  `checkpoint`: a local file holding the state dict in transformers naming (torch-saved plain tensors, or .safetensors),
    or `dims` + `state` (keyword-only) inject the weights directly.  Nothing is downloaded."""
    NAMES = ('wavlmbase+', 'wavlmlarge')
    min_samples = arch.WAVLM_MIN_SAMPLES
    family = "WavLM"

    def __init__(self, name='wavlmbase+', device='cuda', checkpoint=None, *, dims=None, state=None, units_layer=None):
        super().__init__()
        if name not in self.NAMES:
            raise ValueError(f"[x] Unknown units encoder: {name}")
        self.name, self.device = name, device
        if dims is None:
            dims = arch.wavlm_dims("large" if name == 'wavlmlarge' else "base+")
        if state is None:
            if checkpoint is None:
                raise NotImplementedError(f"WavLMUnits: {name!r} without local weights would be a hub download, which is not built; pass "
                                          "checkpoint=PATH or dims= / state=")
            print(name)
            self.model = WavLM(dims, checkpoint=checkpoint, normalize=name == 'wavlmlarge')
        else:
            self.model = WavLM(dims, state=state, normalize=name == 'wavlmlarge')
        self.hidden_dim = self.model.dims["n_state"]
        self.n_ctx = self.model.dims["n_ctx"]      # the window of one call, in frames
        self.set_units_layer(units_layer)

    def set_units_layer(self, units_layer):
        n = self.model.dims["n_layer"]
        self.units_layer = n if units_layer is None else int(units_layer)
        if not 0 <= self.units_layer <= n:
            raise ValueError(f"WavLMUnits: units_layer {units_layer} outside 0 .. {n}")

    @classmethod
    def synthetic(cls, name='wavlmbase+', dims=None, seed=0, device='cuda', units_layer=None):
        """seeded weights (lds.arch.wavlm_init_state) for `dims` (default: the named model's) -- no checkpoint ships"""
        dims = dict(arch.wavlm_dims("large" if name == 'wavlmlarge' else "base+") if dims is None else dims)
        return cls(name, device=device, dims=dims, state=arch.wavlm_init_state(dims, seed), units_layer=units_layer)

    @staticmethod
    def frames_of(n_samples):
        return arch.wavlm_frames(n_samples)

    @torch.inference_mode()
    def __call__(self, audio, padding_mask=None):
        """audio (any shape, flattened into ONE clip) -> units [T, C] on the device; padding_mask is ignored as WhisperLargeV3 ignores it"""
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise RuntimeError("WavLMUnits needs the audio as a tensor on a HIP device (no CPU fallback)")
        return self.model.encode(audio.reshape(1, -1), layer=self.units_layer).squeeze(0)

    encode = __call__

    @torch.inference_mode()
    def encode_ragged(self, audio, lengths):
        if audio.dim() != 2:
            raise ValueError(f"WavLMUnits.encode_ragged: audio must be [B, L], got {list(audio.shape)}")
        B, L = audio.shape
        ln = native.WavLM.lengths(lengths, B, L)      # (host-side validation first: a bad length is a ValueError on any device)
        if not audio.is_cuda:
            raise RuntimeError("WavLMUnits.encode_ragged needs the audio on a HIP device (no CPU fallback)")
        units = self.model.encode(audio, ln, layer=self.units_layer)
        return units, torch.from_numpy(np.array([self.frames_of(int(n)) for n in ln], dtype=np.int64))


class WhisperLargeV3(torch.nn.Module):
    """reference tools/tools.py:105-126.  `checkpoint` (the reference hard-codes this path) holds {"dims", "model_state_dict"};
    `dims` + `state` (not in the reference) inject them directly."""

    def __init__(self, device='cuda', checkpoint='pretrain/large-v3_encoder.pt', *, dims=None, state=None):
        super().__init__()
        self.device = device
        if state is None:
            print('whisper_large_v3')
            ck = torch.load(checkpoint, map_location="cpu", weights_only=False)
            dims, state = ModelDimensions(**ck["dims"]), ck["model_state_dict"]
        model = Whisper(dims)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
        self.hidden_dim = dims
        self.model = model
        self.model.eval()

    min_samples = 400
    family = "Whisper"

    @staticmethod
    def frames_of(n_samples):
        return (n_samples // 160 - 1) // 2 + 1

    @property
    def n_ctx(self):
        """the window of one call, in frames"""
        return self.model.encoder.n_ctx

    @classmethod
    def synthetic(cls, dims=None, seed=0, device='cuda'):
        """seeded weights (lds.arch.whisper_init_state) for `dims` (default: large-v3's) -- no checkpoint ships"""
        if dims is None:
            dims = ModelDimensions(**arch.WHISPER_LARGE_V3_DIMS)
        return cls(device=device, dims=dims, state=arch.whisper_init_state(dims.n_mels, dims.n_audio_state, dims.n_audio_layer, seed))

    @torch.inference_mode()
    def __call__(self, audio, padding_mask=None):
        """audio (any shape, flattened into ONE clip as the reference's audio.view(1, -1) does) -> units [T, C] on the device"""
        if not audio.is_cuda:
            raise RuntimeError("WhisperLargeV3 needs the audio on a HIP device (no CPU fallback)")
        audio = audio.reshape(1, -1).float().contiguous()
        return self.model.encoder.native().encode(audio).squeeze(0)

    @torch.inference_mode()
    def encode_ragged(self, audio, lengths):
        B, L = audio.shape
        enc = self.model.encoder.native()
        ln = enc.lengths(lengths, B, L)      # (host-side validation first: a bad length is a ValueError on any device)
        if not audio.is_cuda:
            raise RuntimeError("WhisperLargeV3.encode_ragged needs the audio on a HIP device (no CPU fallback)")
        units = enc.encode(audio.float().contiguous(), ln)
        return units, torch.from_numpy(self.frames_of(ln.astype(np.int64)))
