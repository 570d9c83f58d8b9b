"""`Vocoder` wrapper with the reference's constructor, attributes, `extract` and `infer` (reference
diffusion/vocoder.py:5-33).  `extract` runs the VAE encoder (`extract_ragged`: a batch of clips of their own
lengths); the resampler in front of it (tools.tools.Resample, the HIP polyphase kernel) is opt-in: set `vocoder.resample = True`."""
import torch

from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN


class Vocoder:
    # Not in the reference: True sends audio of another rate through the resampler (see extract).  An attribute rather than a constructor
    # argument: the constructor keeps the reference's parameters exactly, and an instance made without __init__ reads the default.
    resample = False

    def __init__(self, vocoder_type, vocoder_ckpt, device=None):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = device
        self.vocoder_type = vocoder_type
        if vocoder_type == "hifi-vaegan":
            self.vocoder = Hifi_VAEGAN(vocoder_ckpt, device=device)
        else:
            raise ValueError(f" [x] Unknown vocoder: {vocoder_type}")
        self.resample_kernel = {}
        self.vocoder_sample_rate = self.vocoder.sample_rate()
        self.vocoder_hop_size = self.vocoder.hop_size()
        self.dimension = self.vocoder.dimension()

    def extract(self, audio, sample_rate, keyshift=0, **kwargs):
        """audio [B,L] at `sample_rate` -> latent [B,T,2C] (or z [B,T,C] with only_z=True); kwargs (only_z, only_mean) go to
        Hifi_VAEGAN.extract (reference diffusion/vocoder.py:24-31).  Two deviations from the reference:
          - resampling is opt-in: by default sample_rate must equal the vocoder's rate (ValueError naming both otherwise), where
            the reference resamples with torchaudio; a Vocoder whose `resample` attribute is True sends a mismatched rate through
            self.resample_kernel[str(sample_rate)], a tools.tools.Resample made on first use (reference diffusion/vocoder.py:24-30);
          - keyshift must be 0 (ValueError otherwise): the reference passes keyshift= to Hifi_VAEGAN.extract, which has no such
            parameter, so its extract raises TypeError for every call; the latent of unshifted audio is what it means."""
        rs = self._check_extract("Vocoder.extract", sample_rate, keyshift)
        if rs is not None:
            audio = rs(audio)
        return self.vocoder.extract(audio, **kwargs)

    def extract_ragged(self, audio, sample_rate, lengths, keyshift=0, **kwargs):
        """Extension (not in the reference): a padded batch of clips [B,L] + every clip's own sample count -> [B,T,2C] (or z) with each
        clip encoded as if alone and zeros beyond its ceil(lengths[b] / hop) frames (Hifi_VAEGAN.extract_ragged); sample_rate and
        keyshift as in extract; with `resample` set and another rate, audio and lengths are at that rate and the batch is resampled by
        Resample.forward_ragged first, so the frames are those of the resampled lengths"""
        rs = self._check_extract("Vocoder.extract_ragged", sample_rate, keyshift)
        if rs is not None:
            audio, lengths = rs.forward_ragged(audio, lengths)
        return self.vocoder.extract_ragged(audio, lengths, **kwargs)

    def _check_extract(self, name, sample_rate, keyshift):
        if keyshift != 0:
            raise ValueError(f"{name}: keyshift must be 0 (got {keyshift}); the encoder takes no key shift")
        if sample_rate == self.vocoder_sample_rate:
            return None
        if not self.resample:
            raise ValueError(f"{name}: audio at {sample_rate} Hz, the vocoder runs at {self.vocoder_sample_rate} Hz; "
                             "resample the audio first, or set resample=True / use tools.tools.Resample")
        from tools.tools import Resample
        kernels, key_str = self.__dict__.setdefault("resample_kernel", {}), str(sample_rate)
        if key_str not in kernels:
            kernels[key_str] = Resample(sample_rate, self.vocoder_sample_rate)      # (its filter is uploaded on first use: nothing to move)
        return kernels[key_str]

    def infer(self, mel):
        return self.vocoder(mel)

    def infer_ragged(self, mel, lengths):
        """Extension (not in the reference): a padded ragged batch of mels [B,T,M] + per-utterance frame counts -> wav [B,1,T*hop]"""
        return self.vocoder.forward_ragged(mel, lengths)
