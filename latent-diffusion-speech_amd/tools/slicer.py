"""Silence slicer in front of DiffusionSVC.infer_from_long_audio: the reference's tools/slicer.py with its names and signatures.  The
frame RMS (librosa.feature.rms there) runs on the device (include/lds.h lds_frame_rms); one copy of it -- a few thousand floats -- comes
to the host, where the decisions are taken (`Slicer.slice_from_rms`, pure host logic).  Deviations, each raising instead of guessing:
  - mono 1-D waveforms only: a 2-D one is a ValueError (the reference's `len(waveform)` counts channels there);
  - the waveform is a tensor on a HIP device, or a numpy array that is moved there; a CPU tensor raises (no CPU fallback);
  - `cut` and `chunks2audio` load files with librosa / torchaudio: NotImplementedError.
The reference's quirks are recorded, not repaired: the early exit compares a sample count with `min_length`, a frame count; the
pad mode of the RMS is librosa's default (zeros since 0.10; `Slicer.pad_mode = "reflect"` gives the older one)."""
import numpy as np
import torch


class Slicer:
    pad_mode = "constant"

    def __init__(self, sr: int, threshold: float = -40., min_length: int = 5000, min_interval: int = 300, hop_size: int = 20,
                 max_sil_kept: int = 5000):
        """threshold in dB; the four durations in milliseconds.  The attributes hold them as the decisions use them: the threshold as a
        linear amplitude, hop_size and win_size in samples, min_length, min_interval and max_sil_kept in frames of hop_size samples."""
        if not (hop_size <= min_interval <= min_length):
            raise ValueError('The following condition must be satisfied: min_length >= min_interval >= hop_size')
        if max_sil_kept < hop_size:
            raise ValueError('The following condition must be satisfied: max_sil_kept >= hop_size')
        self.threshold = 10 ** (threshold / 20.)
        self.hop_size = round(sr * hop_size / 1000)
        interval_samples = sr * min_interval / 1000
        self.win_size = min(round(interval_samples), 4 * self.hop_size)
        self.min_length, self.min_interval, self.max_sil_kept = (round(v / self.hop_size) for v in
                                                                 (sr * min_length / 1000, interval_samples, sr * max_sil_kept / 1000))

    def _apply_slice(self, waveform, begin, end):
        """frames [begin, end) of a mono waveform, in samples, clipped to its end"""
        first, last = begin * self.hop_size, end * self.hop_size
        return waveform[first: min(waveform.shape[0], last)]

    def _silence_tags(self, rms):
        """[(first, last)] frame ranges to cut out, from the frame RMS (reference tools/slicer.py:41-93)"""
        keep = self.max_sil_kept
        tags = []
        sil_start, clip_start = None, 0

        def lowest(a, b):      # the frame of the smallest RMS in [a, b], clipped to the list as a slice is
            a = max(a, 0)
            return int(np.argmin(rms[a: b + 1])) + a

        for i, level in enumerate(rms):
            if level < self.threshold:
                if sil_start is None:
                    sil_start = i
                continue
            if sil_start is None:
                continue
            leading = sil_start == 0 and i > keep
            middle = i - sil_start >= self.min_interval and i - clip_start >= self.min_length
            if leading or middle:
                gap = i - sil_start
                if gap <= keep:
                    pos = lowest(sil_start, i)
                    tags.append((0, pos) if sil_start == 0 else (pos, pos))
                    clip_start = pos
                else:
                    pos_l, pos_r = lowest(sil_start, sil_start + keep), lowest(i - keep, i)
                    first, last = pos_l, pos_r
                    if gap <= keep * 2:
                        pos = lowest(i - keep, sil_start + keep)
                        first, last = min(pos_l, pos), max(pos_r, pos)
                    if sil_start == 0:
                        first, last = 0, pos_r
                    tags.append((first, last))
                    clip_start = last
            sil_start = None
        total = len(rms)
        if sil_start is not None and total - sil_start >= self.min_interval:
            pos = lowest(sil_start, min(total, sil_start + keep))
            tags.append((pos, total + 1))
        return tags

    def slice_from_rms(self, rms_list, n_samples):
        """The decisions of `slice` from the frame RMS (host array) of a mono waveform of n_samples: the reference's chunk dict
        {"0": {"slice": bool, "split_time": "begin,end"}, ...} in samples; "slice" True marks a silence to drop"""
        n_samples = int(n_samples)
        whole = {"0": {"slice": False, "split_time": f"0,{n_samples}"}}
        if n_samples <= self.min_length:      # (sic: samples against frames, reference tools/slicer.py:38)
            return whole
        tags = self._silence_tags(np.asarray(rms_list).reshape(-1))
        if not tags:
            return whole
        hop, chunks = self.hop_size, []

        def add(silent, begin, end):
            chunks.append({"slice": silent, "split_time": f"{begin},{end}"})
        if tags[0][0]:
            add(False, 0, min(n_samples, tags[0][0] * hop))
        for i, (first, last) in enumerate(tags):
            if i:
                add(False, tags[i - 1][1] * hop, min(n_samples, first * hop))
            add(True, first * hop, min(n_samples, last * hop))
        if tags[-1][1] * hop < n_samples:
            add(False, tags[-1][1] * hop, n_samples)
        return {str(i): c for i, c in enumerate(chunks)}

    def frame_rms(self, waveform):
        """the frame RMS of a mono waveform on the device (lds_frame_rms), fp32 [n] on the device"""
        from lds import native
        return native.frame_rms(_device_mono("Slicer.slice", waveform), self.win_size, self.hop_size, self.pad_mode)

    def slice(self, waveform):
        if len(waveform.shape) > 1:
            raise ValueError(f"Slicer.slice takes a mono 1-D waveform, got shape {list(waveform.shape)} (mix the channels down first)")
        n = int(waveform.shape[0])
        if n <= self.min_length:
            return self.slice_from_rms(None, n)
        return self.slice_from_rms(self.frame_rms(waveform).cpu().numpy(), n)


def _device_mono(name, waveform):
    if isinstance(waveform, np.ndarray):
        waveform = torch.from_numpy(np.ascontiguousarray(waveform, dtype=np.float32)).to("cuda")
    if not torch.is_tensor(waveform) or not waveform.is_cuda:
        raise RuntimeError(f"{name} needs the waveform as a numpy array or a tensor on a HIP device (no CPU fallback)")
    return waveform


def cut(audio_path, db_thresh=-30, min_len=5000, flask_mode=False, flask_sr=None):
    raise NotImplementedError("tools.slicer.cut loads the file with librosa, which is not built: load the audio and call Slicer(sr, db_thresh, min_len).slice")


def chunks2audio(audio_path, chunks):
    raise NotImplementedError("tools.slicer.chunks2audio loads the file with torchaudio, which is not built: slice the loaded audio by the chunks' split_time")


def ranges_from_chunks(chunks, hop_size):
    """chunk dict -> [(start_frame, begin, end)]: the sample ranges [begin, end) that `split` cuts out (reference tools/slicer.py:156-164;
    hop_size may be fractional), silent chunks included, chunks without a whole frame dropped"""
    out = []
    for chunk in dict(chunks).values():
        first, last = (int(t) for t in chunk["split_time"].split(","))
        frames = (int(first // hop_size), int(last // hop_size))      # (an empty chunk has first == last and so no whole frame either)
        if frames[1] > frames[0]:
            out.append((frames[0], int(frames[0] * hop_size), int(frames[1] * hop_size)))
    return out


def split_ranges(audio, sample_rate, hop_size, db_thresh=-40, min_len=5000, rms_list=None):
    """`split` without the cutting: [(start_frame, begin, end)] for the batched path.  rms_list (a host array): the frame RMS if it is known
    already -- then `audio` only gives the length and nothing runs on the device."""
    slicer = Slicer(sr=sample_rate, threshold=db_thresh, min_length=min_len)
    if len(audio.shape) > 1:
        raise ValueError(f"split takes a mono 1-D waveform, got shape {list(audio.shape)}")
    chunks = slicer.slice(audio) if rms_list is None else slicer.slice_from_rms(rms_list, audio.shape[0])
    return ranges_from_chunks(chunks, hop_size)


def split(audio, sample_rate, hop_size, db_thresh=-40, min_len=5000):
    """[(start_frame, segment)] as the reference returns them (tools/slicer.py:149-165); the segments are views of `audio`"""
    return [(start_frame, audio[begin:end]) for start_frame, begin, end in split_ranges(audio, sample_rate, hop_size, db_thresh, min_len)]
