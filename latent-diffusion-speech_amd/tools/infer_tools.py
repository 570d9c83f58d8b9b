"""`DiffusionSVC` inference facade: the reference's tools/infer_tools.py:9-117 with call signatures that are consistent with
`Unit2Mel.forward` / `Vocoder.infer` (the reference's own versions raise TypeError before any compute).  What
22_infer_tts.py uses is kept (load_model, __call__, infer, mel2wav), plus `encode_units` on the units encoder (Whisper or HuBERT),
`extract_volume_and_mask` and `infer_from_long_audio`: a recording in, the converted recording out, its segments run as ragged batches.
Not built: key shift and f0 (the reference's `extract_f0` does not exist; the TTS model takes neither)."""
import numpy as np
import torch

from diffusion.unit2mel import load_model_vocoder


class DiffusionSVC:
    def __init__(self, device=None):
        self.device = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        self.model_path = None
        self.model = None
        self.vocoder = None
        self.args = None
        self.units_encoder = None
        self.volume_extractor = None

    def load_model(self, model_path, loaded_vocoder=None, units_encoder_checkpoint=None, *, resample=False, encoder=None, **_ignored):
        """reference infer_tools.py:28-30 (22_infer_tts.py passes extra f0_min/f0_max keywords that the reference's own
        method does not accept; they are accepted and ignored here).  The reference builds its Units_Encoder here (infer_tools.py:31-38);
        this one only when `units_encoder_checkpoint` names the checkpoint of the encoder that args.data.encoder names: the Whisper
        encoder's (large-v3_encoder.pt; also when no encoder is named) or, for 'hubertsoft' / 'contentvec768l12', a HubertSoft state dict
        (tools.tools.HubertUnits), or for 'xlsr_53_56k' a wav2vec 2.0 state dict of plain tensors (tools.tools.Audio2xlsr_53_56k), or for
        'wavlmbase+' / 'wavlmlarge' the WavLM state dict in transformers naming (tools.tools.WavLMUnits).
        `resample` (keyword-only, not in the reference) goes to Units_Encoder: with True, encode_units resamples audio of another rate; `encoder` (keyword-only) overrides the name in args.data.encoder."""
        self.model_path = model_path
        self.model, self.vocoder, self.args = load_model_vocoder(model_path, device=self.device, loaded_vocoder=loaded_vocoder)
        from tools.tools import Volume_Extractor
        self.volume_extractor = Volume_Extractor(hop_size=512, block_size=self.args["data"]["block_size"],      # (reference infer_tools.py:39-43)
                                                 model_sampling_rate=self.args["data"]["sampling_rate"])
        if units_encoder_checkpoint is not None:
            from tools.tools import Audio2xlsr_53_56k, HubertUnits, Units_Encoder, WavLMUnits, WhisperLargeV3
            data = getattr(self.args, "data", None)
            name = encoder if encoder is not None else getattr(data, "encoder", "whisper_large_v3")
            if name in HubertUnits.NAMES:
                model = HubertUnits(name, device=self.device, checkpoint=units_encoder_checkpoint)
            elif name == "xlsr_53_56k":
                model = Audio2xlsr_53_56k(device=self.device, checkpoint=units_encoder_checkpoint)
            elif name in WavLMUnits.NAMES:
                model = WavLMUnits(name, device=self.device, checkpoint=units_encoder_checkpoint)
            else:
                model = WhisperLargeV3(device=self.device, checkpoint=units_encoder_checkpoint)
            self.units_encoder = Units_Encoder(name, getattr(data, "encoder_sample_rate", 16000),
                                               getattr(data, "encoder_hop_size", 320), device=self.device,
                                               units_forced_mode=getattr(data, "units_forced_mode", "nearest"),
                                               model=model, resample=resample)

    def encode_units(self, audio, sr=44100, padding_mask=None):
        """reference infer_tools.py:41-44: audio at `sr` -> units [T, C] on the device (Units_Encoder.encode: `sr` must be the encoder's
        rate unless load_model was given resample=True)"""
        if self.units_encoder is None:
            raise NotImplementedError("no units encoder is loaded: pass units_encoder_checkpoint= to load_model, or set .units_encoder")
        return self.units_encoder.encode(audio, sr, padding_mask=padding_mask)

    def encode_tokens(self, audio, sr, codebook):
        """audio at `sr` -> semantic tokens int64 [T] on the device (Units_Encoder.encode_tokens: units, then the nearest centre of `codebook`)"""
        if self.units_encoder is None:
            raise NotImplementedError("no units encoder is loaded: pass units_encoder_checkpoint= to load_model, or set .units_encoder")
        return self.units_encoder.encode_tokens(audio, sr, codebook)

    @torch.no_grad()
    def extract_volume_and_mask(self, audio, sr=44100, threhold=-60.0):
        """reference infer_tools.py:51-57: audio [L] at `sr` -> (volume [1, n, 1], mask [1, n * block_size]) on the device, n = int(L // hop) + 1
        frames of hop = block_size * sr / sampling_rate samples"""
        assert self.volume_extractor is not None
        volume = self.volume_extractor.extract(audio, sr, device=self.device)
        mask = self.volume_extractor.get_mask_from_volume(volume, threhold=threhold, device=self.device)
        return volume.unsqueeze(-1).unsqueeze(0), mask

    @torch.no_grad()
    def mel2wav(self, mel, f0=None, start_frame=0):
        """reference infer_tools.py:60-67; the vocoder takes the mel only (reference vocoder.py:32)"""
        if start_frame == 0:
            return self.vocoder.infer(mel)
        out_wav = self.vocoder.infer(mel[:, start_frame:, :].contiguous())
        return torch.nn.functional.pad(out_wav, (start_frame * self.vocoder.vocoder_hop_size, 0))

    @torch.no_grad()
    def __call__(self, units, f0=None, volume=None, spk_id=1, aug_shift=0, gt_spec=None, infer_speedup=10, method="unipc", use_tqdm=True, x_T=None):
        """reference infer_tools.py:70-74: units [B,T,C] -> mel [B,T,M]; f0 is unused by the TTS model and must be None"""
        if f0 is not None:
            raise NotImplementedError("the TTS Unit2Mel has no f0 input (22_infer_tts.py passes f0=None)")
        B = units.shape[0]
        if torch.is_tensor(spk_id):
            sid = spk_id.to(self.device).long().reshape(B, -1)
        else:
            sid = torch.LongTensor(np.full((B, 1), int(spk_id))).to(self.device)
        return self.model(units.to(self.device), volume, spk_id=sid, aug_shift=None, gt_spec=gt_spec, infer=True,
                          infer_speedup=infer_speedup, method=method, use_tqdm=use_tqdm, x_T=x_T)

    @torch.no_grad()
    def call_ragged(self, units, lengths, spk_id=1, infer_speedup=10, method="unipc", x_T=None):
        """Extension: a padded ragged batch of units [B,T,C] + per-utterance frame counts -> mel [B,T,M] (Unit2Mel.forward_ragged)"""
        B = units.shape[0]
        sid = spk_id.to(self.device).long().reshape(B, -1) if torch.is_tensor(spk_id) else torch.LongTensor(np.full((B, 1), int(spk_id))).to(self.device)
        return self.model.forward_ragged(units.to(self.device), lengths, spk_id=sid, infer_speedup=infer_speedup, method=method, x_T=x_T)

    @torch.no_grad()
    def infer(self, units, f0=None, volume=None, gt_spec=None, spk_id=1, aug_shift=0, infer_speedup=10, method="unipc", use_tqdm=True, x_T=None):
        """reference infer_tools.py:77-81: units -> waveform [B,1,T*hop]"""
        out_mel = self.__call__(units, f0, volume, spk_id=spk_id, aug_shift=aug_shift, gt_spec=None, infer_speedup=infer_speedup,
                                method=method, use_tqdm=use_tqdm, x_T=x_T)
        return self.mel2wav(out_mel, f0)

    def _plan_long_audio(self, sr, ranges, batch_size):
        """The host-side plan of infer_from_long_audio for the segments `ranges` = [(start_frame, begin, end)] of a recording at `sr`
        (tools.slicer.split_ranges): per segment its model frames n_s = int(len // hop) + 1, and the chunks: segment numbers sorted by
        length (stable), at most batch_size each.  ValueError naming the segment that exceeds the encoder's window.  The frame rule and
        the window are the encoder's: Whisper's (L // 160 - 1) // 2 + 1 frames of n_audio_ctx, a HuBERT encoder's L // 320 of its n_ctx, or XLSR-53's
        unpadded level rule (lds.arch.w2v_frames) of its n_ctx."""
        block_size, rate = self.args["data"]["block_size"], self.args["data"]["sampling_rate"]
        hop_size = block_size * sr / rate
        ue = self.units_encoder
        enc = ue.model      # (tools.tools.WhisperLargeV3, HubertUnits or Audio2xlsr_53_56k: frames_of, n_ctx, family)
        n_frames = []
        for s, (start_frame, begin, end) in enumerate(ranges):
            ln = end - begin
            n_frames.append(int(ln // hop_size) + 1)
            at_enc = -((-ln * ue.encoder_sample_rate) // sr)      # ceil(len * new / orig): what the resampler makes of it
            if enc.frames_of(at_enc) > enc.n_ctx:
                raise ValueError(f"infer_from_long_audio: segment {s} (samples {begin} .. {end}, {ln / sr:.1f} s) exceeds the units encoder's window of "
                                 f"{enc.n_ctx} frames (30 s for {enc.family}); splitting a segment further is not built")
        order = sorted(range(len(ranges)), key=lambda s: ranges[s][2] - ranges[s][1])
        chunks = [order[c:c + int(batch_size)] for c in range(0, len(order), int(batch_size))]
        return dict(hop_size=hop_size, block_size=block_size, n_frames=n_frames, chunks=chunks)

    @torch.no_grad()
    def infer_from_long_audio(self, audio, sr=44100, key=0, spk_id=1, aug_shift=0, infer_speedup=10, method="unipc", use_tqdm=True, threhold=-60,
                              threhold_for_split=-40, min_len=5000, *, batch_size=16, x_T=None, index=None, index_ratio=0.5, index_k=8, index_nprobe=None,
                              index_weights="inverse_square"):
        """reference infer_tools.py:83-117: a mono recording [L] at `sr` (numpy, or a tensor on the device) -> (the converted recording fp32
        [N] on the device, the model's sampling rate).  The recording is cut at its silences (tools.slicer.split_ranges), the volume mask is
        taken from the whole clip, and where the reference loops over the segments -- one encoder call, one sampler run, one vocoder call
        and a host round trip each -- the segments, sorted by length, go through Units_Encoder.encode_ragged,
        units_forced_alignment_ragged, Unit2Mel.forward_ragged and Vocoder.infer_ragged in padded batches of at most `batch_size`
        (1 .. 64; keyword-only, not in the reference), every segment "as if alone"; one lds_overlap_assemble then applies the mask, leaves
        the silences between segments zero and cross-fades the frame by which neighbours overlap.  Nothing but the slicer's frame RMS
        returns to the host on the way.
        Segment s has n_s = int(len_s // hop) + 1 model frames, hop = block_size * sr / sampling_rate: its units are the encoder's own
        frames aligned to n_s by 'nearest'.  Noise: with x_T None one torch.randn((1, 1, M, n_s)) is drawn per segment in the segments' own
        order -- the reference's draw order -- so a torch seed gives the same audio at any batch_size, up to the ragged entries' tolerance;
        x_T may also be the list of those tensors.  key != 0 is NotImplementedError (no f0 path); aug_shift and use_tqdm are accepted and
        unused, as volume and f0 are unused by the model (volume_embed is None).  A segment over the encoder's window and a batch_size
        outside 1 .. 64 are ValueErrors; audio at another rate than the encoder's needs load_model(..., resample=True).
        index (a cluster.index.UnitsIndex; keyword-only, not in the reference): units retrieval -- every chunk's encoder frames are blended
        with their index_k nearest rows of the index's pool at index_ratio (UnitsIndex.retrieve, per-clip lengths) before the alignment;
        index_nprobe (needs an index built with an IVF, UnitsIndex.build_ivf): only the rows of a frame's index_nprobe best lists are searched;
        index_weights ("inverse_square" or "uniform": UnitsIndex.retrieve's weights; the metric is the index's own);
        without an index nothing changes, bit for bit."""
        if key != 0:
            raise NotImplementedError("infer_from_long_audio: key shift needs the f0 path, which is not built (the reference's extract_f0 does not exist); key must be 0")
        if not 1 <= int(batch_size) <= 64:
            raise ValueError(f"infer_from_long_audio: batch_size {batch_size} outside 1 .. 64 (the ragged entries' limit)")
        if self.units_encoder is None:
            raise NotImplementedError("no units encoder is loaded: pass units_encoder_checkpoint= to load_model, or set .units_encoder")
        from lds import native
        from tools.slicer import split_ranges
        from tools.tools import _device_wave, units_forced_alignment_ragged
        audio = _device_wave("infer_from_long_audio", audio, self.device)
        if audio.dim() != 1:
            raise ValueError(f"infer_from_long_audio takes a mono 1-D recording, got shape {list(audio.shape)}")
        audio = audio.float().contiguous()
        rate = self.args["data"]["sampling_rate"]
        ranges = split_ranges(audio, sr, self.args["data"]["block_size"] * sr / rate, db_thresh=threhold_for_split, min_len=min_len)
        if not ranges:
            return torch.zeros(0, device=audio.device), rate
        plan = self._plan_long_audio(sr, ranges, batch_size)
        _, mask = self.extract_volume_and_mask(audio, sr, threhold=float(threhold))
        block, n_frames = plan["block_size"], plan["n_frames"]
        M = self.model.decoder.out_dims
        if x_T is None:
            x_T = [torch.randn((1, 1, M, n), device=audio.device) for n in n_frames]
        if len(x_T) != len(ranges) or any(tuple(x.shape) != (1, 1, M, n) for x, n in zip(x_T, n_frames)):
            raise ValueError(f"x_T must be one [1, 1, {M}, n_s] tensor per segment, n_s = {n_frames}")
        wavs = [None] * len(ranges)
        for idx in plan["chunks"]:
            lens = [ranges[s][2] - ranges[s][1] for s in idx]
            batch = torch.zeros(len(idx), max(lens), device=audio.device)
            for j, s in enumerate(idx):
                batch[j, :ranges[s][2] - ranges[s][1]] = audio[ranges[s][1]:ranges[s][2]]
            units, unit_frames = self.units_encoder.encode_ragged(batch, lens, sample_rate=sr, pad_short=True)
            if index is not None:
                units = index.retrieve(units, k=index_k, ratio=index_ratio, lengths=unit_frames, nprobe=index_nprobe, weights=index_weights)
            nf = [n_frames[s] for s in idx]
            units = units_forced_alignment_ragged(units, unit_frames, nf)
            noise = torch.zeros(len(idx), 1, M, max(nf), device=audio.device)
            for j, s in enumerate(idx):
                noise[j, :, :, :nf[j]] = x_T[s][0]
            mel = self.call_ragged(units, nf, spk_id=spk_id, infer_speedup=infer_speedup, method=method, x_T=noise)
            wav = self.vocoder.infer_ragged(mel, nf)
            for j, s in enumerate(idx):
                wavs[s] = wav[j, 0, :nf[j] * block]
        length = [n * block for n in n_frames]
        offset = np.concatenate([[0], np.cumsum(length)[:-1]])
        out = native.overlap_assemble(torch.cat(wavs), offset, [r[0] * block for r in ranges], length, mask.reshape(-1))
        return out, rate
