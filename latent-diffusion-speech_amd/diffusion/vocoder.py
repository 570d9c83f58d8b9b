"""`Vocoder` wrapper with the reference's constructor, attributes, `extract` and `infer` (reference
diffusion/vocoder.py:5-33).  `extract` runs the VAE encoder (`extract_ragged`: a batch of clips of their own
lengths); the torchaudio resampler in front of it is not built (see Vocoder.extract)."""
import torch

from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN


class Vocoder:
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
          - resampling is not built: sample_rate must equal the vocoder's rate (ValueError naming both otherwise), where the
            reference resamples with torchaudio;
          - keyshift must be 0 (ValueError otherwise): the reference passes keyshift= to Hifi_VAEGAN.extract, which has no such
            parameter, so its extract raises TypeError for every call; the latent of unshifted audio is what it means."""
        self._check_extract("Vocoder.extract", sample_rate, keyshift)
        return self.vocoder.extract(audio, **kwargs)

    def extract_ragged(self, audio, sample_rate, lengths, keyshift=0, **kwargs):
        """Extension (not in the reference): a padded batch of clips [B,L] + every clip's own sample count -> [B,T,2C] (or z) with each
        clip encoded as if alone and zeros beyond its ceil(lengths[b] / hop) frames (Hifi_VAEGAN.extract_ragged); sample_rate and
        keyshift as in extract"""
        self._check_extract("Vocoder.extract_ragged", sample_rate, keyshift)
        return self.vocoder.extract_ragged(audio, lengths, **kwargs)

    def _check_extract(self, name, sample_rate, keyshift):
        if keyshift != 0:
            raise ValueError(f"{name}: keyshift must be 0 (got {keyshift}); the encoder takes no key shift")
        if sample_rate != self.vocoder_sample_rate:
            raise ValueError(f"{name}: audio at {sample_rate} Hz, the vocoder runs at {self.vocoder_sample_rate} Hz; "
                             "resampling is not built, resample the audio first")

    def infer(self, mel):
        return self.vocoder(mel)

    def infer_ragged(self, mel, lengths):
        """Extension (not in the reference): a padded ragged batch of mels [B,T,M] + per-utterance frame counts -> wav [B,1,T*hop]"""
        return self.vocoder.forward_ragged(mel, lengths)
